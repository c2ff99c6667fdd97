// K1's instances for naive, eyelight and the debug shaders (normal, texcoord, color) (the list: vpt_k1_instances.hip.h)
#include "vpt_mesh_kernel.hip.h"
VPT_K1_SIMPLE_INSTANCES(VPT_K1_DEFINE, K_NAIVE)
VPT_K1_SIMPLE_INSTANCES(VPT_K1_DEFINE, K_EYELIGHT)
VPT_K1_SIMPLE_INSTANCES(VPT_K1_DEFINE, K_DEBUG)
