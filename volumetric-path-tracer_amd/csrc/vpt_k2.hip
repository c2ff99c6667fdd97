// K2's instances: both implicit shaders, for scenes without emissive meshes (VPT_FEAT_SDF_LIGHTS) and with them (VPT_FEAT_ALL)
#include "vpt_implicit_kernel.hip.h"
#define VPT_K2_DEFINE(NAME, K, F) template __global__ void NAME<K, F>(DScene, DParams, float4* __restrict__, int* __restrict__, ulonglong2* __restrict__, int, sched_cfg, unsigned* __restrict__, unsigned long long);
VPT_K2_DEFINE(vpt_render_kernel, K_IMPLICIT, VPT_FEAT_SDF_LIGHTS)
VPT_K2_DEFINE(vpt_render_kernel, K_IMPLICIT, VPT_FEAT_ALL)
VPT_K2_DEFINE(vpt_render_kernel, K_IMPLICIT_NORMAL, VPT_FEAT_SDF_LIGHTS)
VPT_K2_DEFINE(vpt_render_kernel, K_IMPLICIT_NORMAL, VPT_FEAT_ALL)
VPT_K2_DEFINE(vpt_render_pilot_kernel, K_IMPLICIT, VPT_FEAT_SDF_LIGHTS)
VPT_K2_DEFINE(vpt_render_pilot_kernel, K_IMPLICIT, VPT_FEAT_ALL)
VPT_K2_DEFINE(vpt_render_pilot_kernel, K_IMPLICIT_NORMAL, VPT_FEAT_SDF_LIGHTS)
VPT_K2_DEFINE(vpt_render_pilot_kernel, K_IMPLICIT_NORMAL, VPT_FEAT_ALL)
