// K1's instances for scenes with points or lines, all five mesh families (the list: vpt_k1_instances.hip.h), + vpt_intersect and the
// first-hit pass on such scenes
#include "vpt_aov_kernel.hip.h"
VPT_K1_CURVES_INSTANCES(VPT_K1_DEFINE, K_VOLPATH)
VPT_K1_CURVES_INSTANCES(VPT_K1_DEFINE, K_PATH)
VPT_K1_CURVES_INSTANCES(VPT_K1_DEFINE, K_NAIVE)
VPT_K1_CURVES_INSTANCES(VPT_K1_DEFINE, K_EYELIGHT)
VPT_K1_CURVES_INSTANCES(VPT_K1_DEFINE, K_DEBUG)

// vpt_intersect (vpt_probes.hip) for scenes with points or lines: the traversal of the VPT_FEAT_CURVES instances
template <bool SPILL>
__global__ void vpt_intersect_curves_kernel(DScene sc, int n, const float* rays, int instance, int* ids, float* uvt, stack_cfg stack) {
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
template __global__ void vpt_intersect_curves_kernel<true>(DScene, int, const float*, int, int*, float*, stack_cfg);
template __global__ void vpt_intersect_curves_kernel<false>(DScene, int, const float*, int, int*, float*, stack_cfg);

// vpt_render_aov_device for scenes with points or lines: the first-hit pass over the same traversal
VPT_AOV_DEFINE(true, true)
VPT_AOV_DEFINE(false, true)
