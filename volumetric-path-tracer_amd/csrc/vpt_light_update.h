// vpt_light_update.h — rebuilding the light tables of a resident scene (include/vpt.h: vpt_scene_update_lights):
// the call vpt_capi.hip and the texture and volume units forward to.  Kernels and host logic: vpt_light_update.hip.
#pragma once
#include <vector>

#include "vpt_resident.h"

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

// After scene_update_apply(.., lights = true) has written the edit, as part of the same call (the counters of vpt_scene_update_stats go
// on): the light list of the edited scene (make_lights) from the host mirrors, and - when the list changed or an edited shape belongs
// to one of its lights - every light table on the device rebuilt to the bytes vpt_scene_create would upload.  Tables that change are
// allocated anew and take the place of their predecessor in r.tables; r.d's pointers and num_lights, the light mirrors, the pool sizes
// and r.light_features follow.  *rebuilt: false for an edit without consequence for the lights (nothing was launched or sent).
// Stream 0; the device has finished when the call returns.
// edit: of its lists only the shapes matter here - those whose vertices moved (the texture and volume units pass an edit without any).
// envs: null for vpt_scene_update_lights - the environments that were lights stay, entries, CDFs and records byte for byte; else the
// environment lights of the edited scene in id order: a recomputed one is a job like a mesh light's, of texel weights instead of areas
// (launch_texel_weights, vpt_texture_update.h), and every one's record is sent.
// sdf_resized: null, or per SDF whether an edit of r.m.sdfs (vpt_scene_update_volumes, vpt_volume_update.h) changed its whd: an SDF light
// among them has another CDF entry, so the tables are rebuilt although the list stays.
// old_instance: null, or - after vpt_scene_update_instances (vpt_instance_update.h) has renumbered the instances and brought r.d and
// the mirrors up to date, all but the light mirrors - per instance of the new list its id in the old one, -1 for one that is new or
// whose shape is another now: a surviving light keeps its CDF, index and guide table under its new id, and the tables are rebuilt
// whenever a light's instance word moved, even where the list is the same by position.
// old_sdf: null, or - after vpt_scene_update_volume_set (vpt_volume_set.h) has changed the number of SDFs and brought r.d and the
// mirrors up to date, all but the light mirrors - per SDF of the new list its id in the old one, -1 for an added one: a surviving SDF
// light is the old light under its new id, and the tables are rebuilt whenever a light's sdf word moved.
int light_update_apply(resident& r, const vpt_scene_edit& edit, bool* rebuilt, const std::vector<env_light>* envs = nullptr,
    const std::vector<char>* sdf_resized = nullptr, const std::vector<int>* old_instance = nullptr, const std::vector<int>* old_sdf = nullptr);
