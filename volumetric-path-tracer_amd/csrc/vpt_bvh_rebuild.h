// vpt_bvh_rebuild.h — building the BVHs of a resident scene anew (include/vpt.h: vpt_scene_rebuild_bvh): the call
// vpt_capi.hip forwards to.  Kernels and host logic: vpt_bvh_rebuild.hip.
#pragma once
#include <vector>

#include "vpt_bvh_build.h"
#include "vpt_resident.h"

// Validates `what` (nothing is written before it has passed), builds the named shapes' BVHs and the scene BVH on the current
// device into buffers of their own, decides the traversal limits from the new trees (VPT_ERR_UNSUPPORTED: the scene is as it was)
// and only then reorders the leaf records and swaps tables, counts and mirrors.  Returns after the device has finished;
// r.refit.ready is cleared.  out: changed and topology with the traversal stacks the new trees need, or - an empty request - untouched;
// the caller runs the light setup afterwards (light_prims follow the leaf records).
// quality: VPT_BVH_MIDDLE or VPT_BVH_SAH for every tree the call builds (another value: VPT_ERR_INVALID_ARG, first of all).
int bvh_rebuild_apply(resident& r, const vpt_bvh_rebuild& what, edit_outcome& out, int quality = VPT_BVH_MIDDLE);

// The scene level of a rebuild, shared with vpt_scene_update_instances (vpt_instance_update.hip): the scene BVH over a table of
// instances, in buffers of the call until scene_level_swap hands them to the scene.
struct scene_level {
  int           num_instances = 0, count = 0;   // count: nodes
  device_buffer inst_box, nodes, prims;         // 2 float4 per instance; vpt_bvh_node[count]; int[num_instances]
  std::vector<vpt_bvh_node> h_nodes;            // the read-back
  std::vector<int>          h_prims, slot_of;
  device_buffer wnodes, enter, d_slot_of;       // the quad-node table (the caller fills it), the enter records, the slot of every instance
};
// instance boxes from `instances` and the root boxes of `shapes` (both on the device), K6's core over them, nodes and primitive order
// into buffers of their own, and the read-back of both (checked: the order is a permutation)
int scene_level_build(resident& r, bvh_build_scratch& core, const DInstance* instances, int num_instances, const DShape* shapes, scene_level& lv, int quality = VPT_BVH_MIDDLE);
// enter records and slot_of_instance: the integer words on the host (prep_enter_tail, from t.shapes and the quad nodes of t), sent,
// then frames and root boxes by the refit's kernel.  inst_shape: the shape of every instance of the table, on the host.
int scene_level_enter(resident& r, scene_level& lv, const scene_tables& t, const int* inst_shape, const DInstance* instances, const DShape* shapes);
// the swap of the scene level: nodes, primitive order, quad-node table, enter records, slots; counts, root reference and box; h.slot_of;
// r.refit.ready = false
void scene_level_swap(resident& r, scene_level& lv, const scene_tables& t);
