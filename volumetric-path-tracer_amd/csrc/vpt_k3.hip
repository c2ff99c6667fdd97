// K3's instances: the volgrid kernel and its pilot, and the free-flight probe over the same device functions
#include "vpt_volgrid_kernel.hip.h"

// vpt_scene_volgrid_track (include/vpt.h): one lane per record flies one free flight with the kernel's own vg_start and vg_track_step -
// not copies - compiled here, in K3's unit, so that it is the same compiled rule.  The records are read where the tables hold them (K3
// reads its LDS copy of the same bytes); the step counter of vpt_scene_volgrid_stats is not touched.
__global__ void vpt_volgrid_track_kernel(DScene sc, volgrid_args va, int n, const float* __restrict__ rays, const ulonglong2* __restrict__ rng_in,
    int* __restrict__ event, int* __restrict__ instance, float* __restrict__ t, int* __restrict__ steps, ulonglong2* __restrict__ rng_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float*     r    = rays + 6 * (long long)i;
  const f3         ro   = mk3(r[0], r[1], r[2]), rd = mk3(r[3], r[4], r[5]);
  const ulonglong2 r_in = rng_in[i];
  rng_t            rng  = {r_in.x, r_in.y};
  vg_walk          w;
  vg_start(w);
  int mode = V_TRACK;
  while (mode == V_TRACK) mode = vg_track_step(sc, va, va.recs, ro, rd, rng, w);   // bounded by VPT_VOLGRID_MAX_STEPS, as in K3
  const bool collided = mode == V_COLLIDE;
  event[i]    = collided ? 1 : (mode == V_ESCAPE ? 0 : 2);
  instance[i] = collided ? w.hit_g : -1;
  t[i]        = collided ? w.tmax : VPT_FLT_MAX;
  steps[i]    = w.steps;
  if (rng_out) {
    ulonglong2 r_out;
    r_out.x = rng.state, r_out.y = rng.inc;
    rng_out[i] = r_out;
  }
}

template __global__ void vpt_volgrid_kernel<false>(DScene, DParams, volgrid_args, float4* __restrict__, int* __restrict__, ulonglong2* __restrict__, sched_cfg);
template __global__ void vpt_volgrid_kernel<true>(DScene, DParams, volgrid_args, float4* __restrict__, int* __restrict__, ulonglong2* __restrict__, sched_cfg);
