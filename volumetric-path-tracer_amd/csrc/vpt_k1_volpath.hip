// K1's instances for volpathtrace (the list: vpt_k1_instances.hip.h)
#include "vpt_mesh_kernel.hip.h"
VPT_K1_SPLIT_INSTANCES(VPT_K1_DEFINE, K_VOLPATH)
