// vpt_texture_update.h — editing the environments and textures of a resident scene (include/vpt.h: vpt_scene_update_textures;
// DESIGN.md §15): the call vpt_capi.hip forwards to.  Kernel and host logic: vpt_texture_update.hip.
#pragma once
#include "vpt_light_update.h"

// Validates `edit` (nothing is written before it has passed), writes texels, texture entries and environment entries, and - when an
// environment's light comes, goes or has to be made anew - rebuilds the light tables through light_update_apply (out.lights_rebuilt).  A texel
// pool that grows is allocated anew and takes its predecessor's place in r.tables.  r's counters (vpt_scene_update_stats) describe
// this call.  Stream 0; the device has finished when the call returns.
int texture_update_apply(resident& r, const vpt_texture_edit& edit, edit_outcome& out);

// one weight per texel of a recomputed environment into the slots its CDF entries will take: max4(texel) * sin_row[row]; one launch, counted
int launch_texel_weights(resident& r, const env_light& env, float* cdf);
