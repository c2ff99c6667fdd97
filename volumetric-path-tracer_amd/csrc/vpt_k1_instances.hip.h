// The instances of K1 the host launches, as lists: vpt_launch.h declares them from these lists (VPT_K1_DECLARE) and the K1 units
// define them from the same lists (VPT_K1_DEFINE) - vpt_k1_volpath.hip and vpt_k1_path.hip for the two path tracers, vpt_k1_simple.hip
// for naive, eyelight and the debug shaders, vpt_k1_curves.hip for scenes with points or lines.  The path tracers' instances take
// most of the library's compile time: in units of their own, `make -j` builds them side by side.
#pragma once
#include "vpt_device.h"
// naive, eyelight and the debug shaders: main and pilot kernel, both stack variants, every light-feature set
#define VPT_K1_SIMPLE_INSTANCES(X, K)                                                                                                       \
  X(vpt_mesh_kernel, K, true, 4) X(vpt_mesh_kernel, K, false, 4) X(vpt_mesh_kernel, K, true, 5) X(vpt_mesh_kernel, K, false, 5)             \
  X(vpt_mesh_kernel, K, true, 7) X(vpt_mesh_kernel, K, false, 7)                                                                            \
  X(vpt_mesh_pilot_kernel, K, true, 4) X(vpt_mesh_pilot_kernel, K, false, 4) X(vpt_mesh_pilot_kernel, K, true, 5)                           \
  X(vpt_mesh_pilot_kernel, K, false, 5) X(vpt_mesh_pilot_kernel, K, true, 7) X(vpt_mesh_pilot_kernel, K, false, 7)
// the two path tracers: the same, + the short triangle records (12) for the main kernel
#define VPT_K1_SPLIT_INSTANCES(X, K) VPT_K1_SIMPLE_INSTANCES(X, K) X(vpt_mesh_kernel, K, true, 12) X(vpt_mesh_kernel, K, false, 12)
// the instances for scenes with points or lines (VPT_FEAT_CURVES on top of every light feature), main and pilot, both stack variants,
// for all five mesh families: a unit of their own, so adding them left the instances above instruction for instruction as they were
#define VPT_K1_CURVES_INSTANCES(X, K)                                                                                                       \
  X(vpt_mesh_kernel, K, true, 23) X(vpt_mesh_kernel, K, false, 23) X(vpt_mesh_pilot_kernel, K, true, 23) X(vpt_mesh_pilot_kernel, K, false, 23)
#define VPT_K1_DEFINE(NAME, K, S, F) template __global__ void NAME<K, S, F>(DScene, DParams, float4* __restrict__, int* __restrict__, ulonglong2* __restrict__, stack_cfg, sched_cfg);
#define VPT_K1_DECLARE(NAME, K, S, F) extern VPT_K1_DEFINE(NAME, K, S, F)
static_assert((VPT_FEAT_ALL | VPT_FEAT_CURVES) == 23 && (VPT_FEAT_SMALL_LIGHTS | VPT_FEAT_COMPACT_TRIS) == 12 && (VPT_FEAT_SMALL_LIGHTS | VPT_FEAT_LARGE_LIGHTS) == 5 && VPT_FEAT_ALL == 7, "feature sets of the lists above");
