// The instances of K1 for the two path tracers (main and pilot kernel, both stack variants, every light-feature set, the short
// triangle records) take most of the library's compile time.  The Makefile's build (-DVPT_SPLIT_TUS) compiles them in translation units of
// their own - vpt_k1_volpath.hip, vpt_k1_path.hip: explicit instantiations - next to vpt_capi.hip, which then only declares them (`make -j`:
// 4.6 -> 2.4 minutes).  Experiment builds (`make variant`) keep everything in one unit: their diagnostic device globals are per unit.
#pragma once
#include "vpt_mesh_kernel.hip.h"
#define VPT_K1_SPLIT_INSTANCES(X, K)                                                                                                        \
  X(vpt_mesh_kernel, K, true, 4) X(vpt_mesh_kernel, K, false, 4) X(vpt_mesh_kernel, K, true, 5) X(vpt_mesh_kernel, K, false, 5)             \
  X(vpt_mesh_kernel, K, true, 7) X(vpt_mesh_kernel, K, false, 7) X(vpt_mesh_kernel, K, true, 12) X(vpt_mesh_kernel, K, false, 12)           \
  X(vpt_mesh_pilot_kernel, K, true, 4) X(vpt_mesh_pilot_kernel, K, false, 4) X(vpt_mesh_pilot_kernel, K, true, 5)                           \
  X(vpt_mesh_pilot_kernel, K, false, 5) X(vpt_mesh_pilot_kernel, K, true, 7) X(vpt_mesh_pilot_kernel, K, false, 7)
// the instances for scenes with points or lines (VPT_FEAT_CURVES on top of every light feature), main and pilot, both stack variants,
// for all five mesh families: compiled in vpt_k1_curves.hip, so adding them left the instances above instruction for instruction as they were
#define VPT_K1_CURVES_INSTANCES(X, K)                                                                                                       \
  X(vpt_mesh_kernel, K, true, 23) X(vpt_mesh_kernel, K, false, 23) X(vpt_mesh_pilot_kernel, K, true, 23) X(vpt_mesh_pilot_kernel, K, false, 23)
// vpt_intersect (vpt_capi.hip) for scenes with points or lines: the traversal of the VPT_FEAT_CURVES instances, compiled in vpt_k1_curves.hip
template <bool SPILL>
__global__ void __launch_bounds__(VPT_BLOCK, VPT_WAVES_PER_SIMD) vpt_intersect_curves_kernel(DScene sc, int n, const float* rays, int instance,
    int* ids, float* uvt, stack_cfg stack) {
  extern __shared__ int lds_stack[];
  const lane_stack2<SPILL> stk = make_lane_stack<SPILL>(lds_stack, stack);
  int i = blockIdx.x * VPT_BLOCK + threadIdx.x;
  const bool live = i < n;
  if (!live) i = 0;
  hit_t h = traverse<false, true>(sc, live, mk3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]), mk3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]), instance, stk);
  if (!live) return;
  ids[2 * i] = h.hit ? h.instance : -1, ids[2 * i + 1] = h.hit ? h.element : -1;
  uvt[3 * i] = h.hit ? h.uv.x : 0, uvt[3 * i + 1] = h.hit ? h.uv.y : 0, uvt[3 * i + 2] = h.hit ? h.distance : 0;
}
#define VPT_K1_DEFINE(NAME, K, S, F) template __global__ void NAME<K, S, F>(DScene, DParams, float4* __restrict__, int* __restrict__, ulonglong2* __restrict__, stack_cfg, sched_cfg);
#define VPT_K1_DECLARE(NAME, K, S, F) extern VPT_K1_DEFINE(NAME, K, S, F)
static_assert((VPT_FEAT_ALL | VPT_FEAT_CURVES) == 23 && (VPT_FEAT_SMALL_LIGHTS | VPT_FEAT_COMPACT_TRIS) == 12 && (VPT_FEAT_SMALL_LIGHTS | VPT_FEAT_LARGE_LIGHTS) == 5 && VPT_FEAT_ALL == 7, "feature sets of the list above");
