// vpt_scene_update.h — editing a resident scene (include/vpt.h: vpt_scene_update): the call vpt_capi.hip forwards to.
// Kernels and host logic: vpt_scene_update.hip.
#pragma once
#include "vpt_resident.h"

// Validates `edit` against the scene (nothing is written before it has passed), then rewrites the tables on the current device,
// stream 0; returns after the device has finished.  r.d.scene_root_*, the mirrors of what was edited and r.varying_media follow.
// lights: the caller rebuilds the light tables afterwards (vpt_scene_update_lights, vpt_light_update.h), so an emission that
// switches between zero and non-zero and moved vertices of a light's shape pass validation.
int scene_update_apply(resident& r, const vpt_scene_edit& edit, bool lights = false);
