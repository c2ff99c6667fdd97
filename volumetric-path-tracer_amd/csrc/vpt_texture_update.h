// vpt_texture_update.h — editing the environments and textures of a resident scene (include/vpt.h: vpt_scene_update_textures;
// DESIGN.md §15): what a vpt_scene keeps for it and the call vpt_capi.hip forwards to.  Kernel and host logic: vpt_texture_update.hip.
#pragma once
#include <vector>

#include "vpt_device_buffer.h"
#include "vpt_light_update.h"

struct texture_updater {
  // texels of the two pools the device holds now (set at creation; a texture that changes size or format gets room at the end)
  long long num_texels_f = 0, num_texels_b = 0;
  // host copy of DScene::textures, read back on the first edit of a handle (the environments' is scene_updater's: vpt_scene_update
  // writes their frames); a texture is an emitter's when the emission_tex of an environment with non-zero emission names it
  bool ready = false;
  std::vector<vpt_texture> textures;
  device_buffer d_sin;   // sin((j + 0.5f) * pif / height) per row of the recomputed environments, made on the host
};

// Validates `edit` (nothing is written before it has passed), writes texels, texture entries and environment entries, and - when an
// environment's light comes, goes or has to be made anew - rebuilds the light tables through light_update_apply.  A texel pool
// that grows is allocated anew and takes its predecessor's place in `tables`.  u's counters (vpt_scene_update_stats) describe this
// call.  Stream 0; the device has finished when the call returns.
int texture_update_apply(DScene& d, const host_mirrors& h, long long num_shape_nodes, scene_updater& u, light_updater& lu, texture_updater& tu,
    std::vector<device_buffer>& tables, const vpt_texture_edit& edit, int* light_features, bool* rebuilt);

// one weight per texel of a recomputed environment into the slots its CDF entries will take: max4(texel) * sin_row[row]
int launch_texel_weights(const env_light& env, float* cdf);
