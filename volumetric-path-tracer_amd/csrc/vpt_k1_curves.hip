// K1's instances for scenes with points or lines, all five mesh families: see vpt_k1_instances.hip.h
#define VPT_INSTANCES_TU
#include "vpt_k1_instances.hip.h"
VPT_K1_CURVES_INSTANCES(VPT_K1_DEFINE, K_VOLPATH)
VPT_K1_CURVES_INSTANCES(VPT_K1_DEFINE, K_PATH)
VPT_K1_CURVES_INSTANCES(VPT_K1_DEFINE, K_NAIVE)
VPT_K1_CURVES_INSTANCES(VPT_K1_DEFINE, K_EYELIGHT)
VPT_K1_CURVES_INSTANCES(VPT_K1_DEFINE, K_DEBUG)
template __global__ void vpt_intersect_curves_kernel<true>(DScene, int, const float*, int, int*, float*, stack_cfg);
template __global__ void vpt_intersect_curves_kernel<false>(DScene, int, const float*, int, int*, float*, stack_cfg);
