// vpt_instance_update.h — adding, removing and re-pointing the instances of a resident scene (include/vpt.h:
// vpt_scene_update_instances): the call vpt_capi.hip forwards to.  Kernels and host logic: vpt_instance_update.hip.
#pragma once
#include "vpt_bvh_rebuild.h"
#include "vpt_resident.h"

// Validates `edit` against the scene (nothing is written before it has passed), renumbers the instances on the current device and
// gathers the new instance table, builds the scene BVH over it, decides the traversal limits from the new tree and the shapes' kept
// ones (VPT_ERR_UNSUPPORTED: the scene is as it was), and only then swaps tables, counts and mirrors; the light tables follow through
// light_update_apply.  `out` is untouched by an edit with all counts zero: nothing was launched or sent.  Returns after the
// device has finished; r.refit.ready is cleared, r.varying_media and r.light_features follow.  The caller runs the light setup and,
// when the lights were rebuilt, the medium setup afterwards.
int instance_update_apply(resident& r, const vpt_instance_edit& edit, edit_outcome& out);
