// vpt_shape_update.h — adding, removing and replacing the shapes of a resident scene (include/vpt.h: vpt_scene_update_shapes;
// DESIGN.md §21): the call vpt_capi.hip forwards to.  Kernels and host logic: vpt_shape_update.hip; the integer layout: vpt_shape_layout.h.
#pragma once
#include "vpt_bvh_rebuild.h"
#include "vpt_resident.h"

// Validates `edit` against the scene (nothing is written before it has passed), lays the pools out for the new shape list, moves the
// untouched shapes' parts device to device, makes vertices, elements, trees and leaf records of the `set` and added shapes on the
// device, decides the traversal limits from the new trees and what the handle keeps of the others (VPT_ERR_UNSUPPORTED: the scene is
// as it was), and only then swaps tables, counts and mirrors; the light tables follow through light_update_apply.  `out` is
// untouched by an edit with all counts zero: nothing was launched or sent.  Returns after the device has finished; r.refit.ready is
// cleared, r.varying_media and r.light_features follow.  The caller runs the light setup and, when the lights were rebuilt, the
// medium setup afterwards.
int shape_update_apply(resident& r, const vpt_shape_edit& edit, edit_outcome& out);
