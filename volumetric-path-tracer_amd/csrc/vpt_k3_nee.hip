// K3's NEE variant (include/vpt.h: vpt_scene_set_volgrid_nee): the instances of vpt_volgrid_nee_kernel - the body of
// csrc/vpt_volgrid_kernel.hip.h with NEE set - and the probe of a shadow flight over the same step function.  A unit of its own:
// vpt_k3.o and vpt_k3_color.o stay the objects they were.
#include "vpt_volgrid_kernel.hip.h"

// vpt_scene_volgrid_transmittance (include/vpt.h): one lane per record flies one ratio-tracked shadow flight with vg_transmittance, the
// loop over the kernel's own vg_nee_step, compiled here.  The records are read where the tables hold them (the kernel reads its LDS copy of
// the same bytes); no counter of the handle is touched, the watchdog word neither: a flight at the step bound answers T = 0 with
// steps = VPT_VOLGRID_MAX_STEPS.
__global__ void vpt_volgrid_transmittance_kernel(DScene sc, volgrid_args va, int n, const float* __restrict__ rays, const ulonglong2* __restrict__ rng_in,
    float* __restrict__ T, int* __restrict__ steps, ulonglong2* __restrict__ rng_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float*     r    = rays + 6 * (long long)i;
  const f3         ro   = mk3(r[0], r[1], r[2]), rd = mk3(r[3], r[4], r[5]);
  const ulonglong2 r_in = rng_in[i];
  rng_t            rng  = {r_in.x, r_in.y};
  vg_walk          w;
  bool             aborted;
  T[i]     = vg_transmittance(sc, va, va.recs, ro, rd, rng, w, aborted);
  steps[i] = w.steps;
  if (rng_out) {
    ulonglong2 r_out;
    r_out.x = rng.state, r_out.y = rng.inc;
    rng_out[i] = r_out;
  }
}

template __global__ void vpt_volgrid_nee_kernel<false>(DScene, DParams, volgrid_args, volgrid_nee_args, float4* __restrict__, int* __restrict__,
    ulonglong2* __restrict__, sched_cfg);
template __global__ void vpt_volgrid_nee_kernel<true>(DScene, DParams, volgrid_args, volgrid_nee_args, float4* __restrict__, int* __restrict__,
    ulonglong2* __restrict__, sched_cfg);
