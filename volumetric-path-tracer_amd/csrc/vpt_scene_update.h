// vpt_scene_update.h — editing a resident scene (include/vpt.h: vpt_scene_update): the call vpt_capi.hip forwards to.
// Kernels and host logic: vpt_scene_update.hip.
#pragma once
#include "vpt_resident.h"

// Validates `edit` against the scene (nothing is written before it has passed), then rewrites the tables on the current device,
// stream 0; returns after the device has finished.  r.d.scene_root_*, the mirrors of what was edited and r.varying_media follow.
// lights: the caller rebuilds the light tables afterwards (vpt_scene_update_lights, vpt_light_update.h), so an emission that
// switches between zero and non-zero and moved vertices of a light's shape pass validation.
// out.changed: true for every edit that passes validation, one without entries included - the counters of vpt_scene_update_stats start again.
// staged: null, or the second source of moved vertices - per entry of edit.shape_ids the float3 positions and the float3 normals (or
// null) where a caller has ALREADY made them on the device, on stream 0 (vpt_subdiv_update.hip).  edit.shape_positions / shape_normals
// are not read then.  Such a caller has validated its own input and begun the update itself (begin_update, the first event, its own
// launches and sends): the counters go on, and the scatter, the refit and everything behind it run as for an uploaded payload.
struct staged_vertices {
  std::vector<const float*> positions, normals;
};
int scene_update_apply(resident& r, const vpt_scene_edit& edit, edit_outcome& out, bool lights = false, const staged_vertices* staged = nullptr);

// Pieces of the refit that vpt_scene_rebuild_bvh (vpt_bvh_rebuild.hip) runs on tables it has made and not yet handed to the scene:
// the same kernels, launched on stream 0 and counted in r.last_launches.  `shapes`, `shape_nodes`, `enter`: device tables of the
// scene's layout; the instances, lights and leaf records are the scene's own.
//  - upd_element_boxes: the bounds of a shape's elements in element order (6 floats each) from its leaf records, with the bound
//    functions of the leaf refit, and old_slot[element] = the slot (local to the shape) that holds it
//  - upd_shape_roots: DShape::root_box of every shape with nodes from its root node (num_shapes < 0: the scene's count; vpt_scene_update_shapes,
//    vpt_shape_update.hip, hands in a table of another length)
//  - upd_instance_boxes: transform_bbox(frame, shape root box) per instance of `instances` (2 float4: the six floats first), invalidb3f
//    for a shape without nodes
//  - upd_enter_records: frames, root boxes and translation_only of `slots` enter records whose integer words are in place, from `instances`
//    (the scene's own table, or the new one of vpt_scene_update_instances)
//  - upd_light_records: frames and root boxes of the mesh lights' records
int upd_element_boxes(resident& r, const DShape& shape, float* boxes, int* old_slot);
int upd_shape_roots(resident& r, DShape* shapes, const float4* shape_nodes, int num_shapes = -1);
int upd_instance_boxes(resident& r, const DInstance* instances, int num_instances, const DShape* shapes, float4* inst_box);
int upd_enter_records(resident& r, float4* enter, int slots, const DInstance* instances, const DShape* shapes);
int upd_light_records(resident& r, const DShape* shapes);
