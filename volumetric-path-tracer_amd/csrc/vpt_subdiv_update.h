// vpt_subdiv_update.h — the subdivision surfaces of a resident scene (include/vpt.h: vpt_scene_attach_subdiv, vpt_scene_update_subdivs;
// DESIGN.md §25): the calls vpt_capi.hip forwards to.  Kernels and host logic: vpt_subdiv_update.hip.
#pragma once
#include <vector>

#include "vpt_resident.h"

// Validates `plan` against itself and against the resident shape (nothing is sent before it has passed), uploads its tables with the
// plan's scratch in one allocation and puts it into the first free slot of r.subdivs: *id_out.  Current device; returns after the copy.
// The counters of vpt_scene_update_stats are this call's: the bytes sent and read back, no launch.
int subdiv_attach(resident& r, const vpt_subdiv_plan& plan, int* id_out);
// frees the plan's allocation; the slot may be taken by a later attach
int subdiv_detach(resident& r, int id);
// The edit: validation, then per named plan the levels, normals, gather and displacement into the plan's staging buffers (stream 0),
// then scene_update_apply with them as its second source and, when a light's instance uses one of the shapes, light_update_apply.
// out: as scene_update_apply and light_update_apply report.
int subdiv_update_apply(resident& r, const vpt_subdiv_edit& edit, edit_outcome& out);
// After vpt_scene_update_shapes has swapped the shape list (vpt_shape_update.hip): plans whose shape was replaced (is_set, per old shape)
// or removed (new_of_old < 0) are dropped, the others name their shape's new id.
void subdiv_plans_follow_shapes(resident& r, const std::vector<int>& new_of_old, const std::vector<char>& is_set);
