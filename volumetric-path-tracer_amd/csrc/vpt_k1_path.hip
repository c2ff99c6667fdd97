// K1's instances for pathtrace (the list: vpt_k1_instances.hip.h)
#include "vpt_mesh_kernel.hip.h"
VPT_K1_SPLIT_INSTANCES(VPT_K1_DEFINE, K_PATH)
