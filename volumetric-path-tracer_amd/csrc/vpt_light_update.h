// vpt_light_update.h — rebuilding the light tables of a resident scene (include/vpt.h: vpt_scene_update_lights):
// what a vpt_scene keeps for it and the call vpt_capi.hip forwards to.  Kernels and host logic: vpt_light_update.hip.
#pragma once
#include <vector>

#include "vpt_device_buffer.h"
#include "vpt_scene_update.h"

struct light_updater {
  // entries of the three pooled light tables the device holds now (set at creation, kept by every rebuild)
  long long num_cdf = 0, num_pool = 0, num_guide = 0;
  // host copies of the small tables the list and the layout are decided from, read back on the first rebuild of a handle
  bool ready = false;
  std::vector<DCdfIndex> index;   // DScene::light_index
  std::vector<vpt_sdf>   sdfs;    // DScene::sdfs: material and whd of an SDF light
  device_buffer d_jobs, d_result, d_tags;   // the recomputed lights' descriptors, {sorted, last entry} per job, record tags per light
};

// One environment light of the edited scene, for a rebuild that follows an edit of environments or textures (vpt_scene_update_textures,
// vpt_texture_update.h): what make_lights and build_lights would make of it.
struct env_light {
  int  environment;
  int  cdf_len;     // width * height of its texture; 0 without one
  int  tag;         // VPT_LIGHT_ENV_TEX / VPT_LIGHT_ENV_CONST
  bool recompute;   // its CDF is made from the texels: the light is new, its texture another one, or the texels were edited
  // of a recomputed one, on the device: the texels (float4 or uchar4 by is_float) and sin((j + 0.5f) * pif / height) per row, made on the host
  const void*  texels;
  const float* sin_row;
  int          width, is_float;
  float4       record[8];   // build_lights' record without the CDF's total (r[6].z): lit_records_kernel reads it from the CDF
};

// After scene_update_apply(.., lights = true) has written the edit: the light list of the edited scene (make_lights) from the host
// mirrors, and - when the list changed or an edited shape belongs to one of its lights - every light table on the device rebuilt to
// the bytes vpt_scene_create would upload.  Tables that change are allocated anew and take the place of their predecessor in
// `tables`; d's pointers and num_lights, u's light mirrors and *light_features follow.  *rebuilt: false for an edit without
// consequence for the lights (nothing was launched or sent).  Stream 0; the device has finished when the call returns.
// envs: null for vpt_scene_update_lights - the environments that were lights stay, entries, CDFs and records byte for byte; else the
// environment lights of the edited scene in id order: a recomputed one is a job like a mesh light's, of texel weights instead of areas
// (launch_texel_weights, vpt_texture_update.h), and every one's record is sent.
// sdf_resized: null, or per SDF whether an edit of lu.sdfs (vpt_scene_update_volumes, vpt_volume_update.h) changed its whd: an SDF light
// among them has another CDF entry, so the tables are rebuilt although the list stays.
int light_update_apply(DScene& d, const host_mirrors& h, scene_updater& u, light_updater& lu, std::vector<device_buffer>& tables,
    const vpt_scene_edit& edit, int* light_features, bool* rebuilt, const std::vector<env_light>* envs = nullptr,
    const std::vector<char>* sdf_resized = nullptr);
