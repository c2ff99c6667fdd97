// K3's coloured variant (include/vpt.h: vpt_scene_set_volgrid_color): the instances of vpt_volgrid_color_kernel - the body
// of csrc/vpt_volgrid_kernel.hip.h with COLOR set - and the probe over the same device functions.  A unit of its own: vpt_k3.o stays the
// object it was, and this one is compiled without the packed float32 instructions, as csrc/vpt_volgrid_aov.hip is.
#include "vpt_volgrid_kernel.hip.h"

// vpt_scene_volgrid_track_color (include/vpt.h): one lane per record flies carrier flights with vg_start and vg_track_step on the coloured
// records and decides every carrier collision with vpt_volgrid_event, from w = (1, 1, 1), as the kernel's shading block does - a pass goes
// on from the collision point in the same direction - until a scatter, an escape or an abort.  Records and chroma rows are read where the
// tables hold them (the kernel reads its LDS copy of the same bytes); no counter of the handle is touched.
__global__ void vpt_volgrid_track_color_kernel(DScene sc, volgrid_args va, volgrid_color_args vc, int n, const float* __restrict__ rays,
    const ulonglong2* __restrict__ rng_in, int* __restrict__ event, int* __restrict__ instance, float* __restrict__ t, float* __restrict__ weight,
    int* __restrict__ passes, int* __restrict__ steps, ulonglong2* __restrict__ rng_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float*     r    = rays + 6 * (long long)i;
  f3               ro   = mk3(r[0], r[1], r[2]);
  const f3         rd   = mk3(r[3], r[4], r[5]);
  const ulonglong2 r_in = rng_in[i];
  rng_t            rng  = {r_in.x, r_in.y};
  float            wv[3] = {1.0f, 1.0f, 1.0f};
  float            flown = 0;   // the world parameter of `ro` on the given ray: the sum of the passed collisions' parameters
  int              np = 0, ev = 2, hit_g = -1;
  long long        nsteps = 0;
  while (true) {   // bounded: a flight by VPT_VOLGRID_MAX_STEPS, the flights by VPT_VOLGRID_MAX_PASSES
    vg_walk w;
    vg_start(w);
    int mode = V_TRACK;
    while (mode == V_TRACK) mode = vg_track_step(sc, va, va.recs, ro, rd, rng, w);
    nsteps += w.steps;
    if (mode == V_ESCAPE) ev = 0;
    if (mode != V_COLLIDE) break;   // an escape, or the step bound: event 2
    const vpt_volgrid_chroma& ch = vc.chroma[w.hit_g];
    const float u    = vpt_volgrid_event_draws(ch.a, wv) ? rand1f(rng) : 0.0f;
    const int   kind = vpt_volgrid_event(ch.a, wv, u, wv, nullptr);
    flown += w.tmax;
    if (kind == VPT_VOLGRID_SCATTER) {
      ev = 1, hit_g = w.hit_g;
      break;
    }
    if (kind == VPT_VOLGRID_END || ++np >= VPT_VOLGRID_MAX_PASSES) break;   // event 2
    ro = ro + rd * w.tmax;
  }
  event[i]    = ev;
  instance[i] = hit_g;
  t[i]        = ev == 1 ? flown : VPT_FLT_MAX;
  for (int c = 0; c < 3; c++) weight[3 * (long long)i + c] = wv[c];
  passes[i] = np;
  steps[i]  = nsteps < 0x7fffffffll ? (int)nsteps : 0x7fffffff;
  if (rng_out) {
    ulonglong2 r_out;
    r_out.x = rng.state, r_out.y = rng.inc;
    rng_out[i] = r_out;
  }
}

template __global__ void vpt_volgrid_color_kernel<false>(DScene, DParams, volgrid_args, volgrid_color_args, float4* __restrict__, int* __restrict__,
    ulonglong2* __restrict__, sched_cfg);
template __global__ void vpt_volgrid_color_kernel<true>(DScene, DParams, volgrid_args, volgrid_color_args, float4* __restrict__, int* __restrict__,
    ulonglong2* __restrict__, sched_cfg);
