// vpt_volume_set.h — volumes, grid instances and SDFs of a resident scene added and removed (include/vpt.h: vpt_scene_update_volume_set;
// DESIGN.md §30): the call vpt_capi.hip's edit path forwards to.  Kernel and host logic: vpt_volume_set.hip; the layout plan:
// vpt_volume_set_layout.h.
#pragma once
#include "vpt_resident.h"

// Validates the edit against r (nothing is written when it is refused), builds the new pool, tables and records into buffers of the
// call, swaps them in, and has the light tables follow when the SDF lights are others.  out.changed stays false for an edit with all
// counts zero.  Stream 0; the device has finished when the call returns.
int volume_set_apply(resident& r, const vpt_volume_set_edit& edit, edit_outcome& out);
