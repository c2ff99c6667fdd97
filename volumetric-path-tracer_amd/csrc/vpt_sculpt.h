// vpt_sculpt.h — sculpting the voxel grids of a resident scene with analytic SDF brushes (include/vpt.h: vpt_scene_sculpt_volumes;
// DESIGN.md §27): the call vpt_capi.hip forwards to.  Kernel and host logic: vpt_sculpt.hip, the rule: vpt_sculpt_rule.h.
#pragma once
#include "vpt_resident.h"

// Validates `edit` (nothing a scene owns is written before it has passed), uploads the stamps' records in one copy and launches one
// kernel per entry with a region and stamps, in order, on stream 0 of r.device.  Only voxels change: no table, no mirror, no light.
// r's counters (vpt_scene_update_stats) describe this call; the device has finished when the call returns.
int sculpt_apply(resident& r, const vpt_sculpt_edit& edit, edit_outcome& out);
