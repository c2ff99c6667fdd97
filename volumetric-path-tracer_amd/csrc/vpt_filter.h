// vpt_filter.h — filtering the voxel grids of a resident scene: remap, blur, noise (include/vpt.h: vpt_scene_filter_volumes; DESIGN.md
// §32): the call vpt_capi.hip forwards to.  Kernels and host logic: vpt_filter.hip, the rule: vpt_filter_rule.h.
#pragma once
#include "vpt_resident.h"

// Validates `edit` (nothing a scene owns is written before it has passed), uploads the ops' records in one copy and launches, per entry
// with a region and ops, in order, on stream 0 of r.device: one kernel per run of pointwise ops, and per BLUR the blur kernel into
// r.d_filter_scratch (grown to the largest blurred region) and the kernel that moves the scratch into place.  Only voxels change: no
// table, no mirror, no light.  r's counters (vpt_scene_update_stats) describe this call; the device has finished when the call returns.
int filter_apply(resident& r, const vpt_filter_edit& edit, edit_outcome& out);
