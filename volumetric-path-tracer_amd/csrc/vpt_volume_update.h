// vpt_volume_update.h — editing the volumes, grid instances and SDFs of a resident scene (include/vpt.h: vpt_scene_update_volumes;
// DESIGN.md §17): the call vpt_capi.hip forwards to.  Kernel and host logic: vpt_volume_update.hip.
#pragma once
#include "vpt_light_update.h"

// Validates `edit` and prepares its bakes (nothing a scene owns is written before both have passed), then writes voxels, the three
// small tables and every SDF record, and - when the SDF lights change - rebuilds the light tables through light_update_apply
// (out.lights_rebuilt).  A voxel pool that grows is allocated anew and takes its predecessor's place in r.tables.  r's counters
// (vpt_scene_update_stats) describe this call.  Stream 0 of r.device; the device has finished when the call returns.
int volume_update_apply(resident& r, const vpt_volume_edit& edit, edit_outcome& out);
