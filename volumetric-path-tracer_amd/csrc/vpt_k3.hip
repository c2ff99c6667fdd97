// K3's instances: the volgrid kernel and its pilot
#include "vpt_volgrid_kernel.hip.h"
template __global__ void vpt_volgrid_kernel<false>(DScene, DParams, volgrid_args, float4* __restrict__, int* __restrict__, ulonglong2* __restrict__, sched_cfg);
template __global__ void vpt_volgrid_kernel<true>(DScene, DParams, volgrid_args, float4* __restrict__, int* __restrict__, ulonglong2* __restrict__, sched_cfg);
