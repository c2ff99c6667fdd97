// vpt_bvh_rebuild.h — building the BVHs of a resident scene anew (include/vpt.h: vpt_scene_rebuild_bvh): the call
// vpt_capi.hip forwards to.  Kernels and host logic: vpt_bvh_rebuild.hip.
#pragma once
#include "vpt_resident.h"

// the traversal stacks the new trees need: vpt_capi.hip's render side takes them over
struct bvh_rebuild_stacks {
  bool rebuilt = false;   // the call built something (false: an empty request, nothing changed)
  int  stack_cap = 16, stack_lds4 = 8, stack_spill4 = 0;
};

// Validates `what` (nothing is written before it has passed), builds the named shapes' BVHs and the scene BVH on the current
// device into buffers of their own, decides the traversal limits from the new trees (VPT_ERR_UNSUPPORTED: the scene is as it was)
// and only then reorders the leaf records and swaps tables, counts and mirrors.  Returns after the device has finished;
// r.refit.ready is cleared.  The caller runs the light setup afterwards (light_prims follow the leaf records).
int bvh_rebuild_apply(resident& r, const vpt_bvh_rebuild& what, bvh_rebuild_stacks& stacks);
