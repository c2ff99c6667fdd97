// vpt_scene_update.h — editing a resident scene (include/vpt.h: vpt_scene_update): what a vpt_scene keeps for it and the
// two calls vpt_capi.hip forwards to.  Kernels and host logic: vpt_scene_update.hip.
#pragma once
#include <vector>

#include "vpt_device_buffer.h"
#include "vpt_scene_prep.h"

// The internal nodes of one BVH by depth: nodes of depth l are order[first[l] .. first[l + 1]) of scene_updater::d_order (ids
// local to the BVH).  A refit walks the levels deepest first.
struct bvh_levels {
  std::vector<int> first;        // depth + 1 entries; empty: no internal node
  long long        offset = 0;   // of this BVH's part of d_order
};

// Built on the first update of a handle (from the tables the device holds: topology never changes) and kept.
struct scene_updater {
  bool ready = false;
  // host copies of the small tables validation reads
  std::vector<vpt_material> materials;
  std::vector<vpt_environment> environments;   // kept current by every edit of a frame here and of an entry in vpt_scene_update_textures
  std::vector<char>         textured;        // material bound to a mesh instance: its texture ids are range-checked
  std::vector<DShape>       shapes;
  std::vector<vpt_light>    lights;
  std::vector<int>          light_kind;      // VPT_LIGHT_* of every light record
  std::vector<char>         shape_lit;       // some light's instance uses the shape
  std::vector<int>          inst_material, inst_flags;   // DInstance::material / shape_flags: the light list of an edited scene (vpt_light_update.hip)
  bvh_levels                scene_levels;
  std::vector<bvh_levels>   shape_levels;
  device_buffer d_order;        // int
  device_buffer d_quad_slots;   // int4 per quad node of DScene::scene_wnodes: the binary nodes behind its slots (prep_quad_slots), local to the BVH
  long long     scene_quads = 0;   // quad nodes of the scene BVH (the shapes' follow at DShape::wnode_offset)
  std::vector<long long> shape_quads;   // per shape
  device_buffer d_inst_box;     // 2 float4 per instance: transform_bbox(frame, shape root box)
  device_buffer d_stage;        // the edit's payload on its way to the tables
  size_t        stage_bytes = 0;
  // what the last update did (profiles/tools/scene_update_measure.py)
  int   last_launches = 0;
  long long last_bytes = 0;
  float last_ms = 0;                         // device time from the first to the last launch of the refit (events on stream 0; the payload is on the device before the first)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;   // made on first use, destroyed by vpt_scene_destroy
};

// Validates `edit` against the scene (nothing is written before it has passed), then rewrites the tables on the current device,
// stream 0; returns after the device has finished.  d.scene_root_* are refreshed.  num_shape_nodes: nodes of DScene::shape_nodes.
// lights: the caller rebuilds the light tables afterwards (vpt_scene_update_lights, vpt_light_update.h), so an emission that
// switches between zero and non-zero and moved vertices of a light's shape pass validation.
int scene_update_apply(DScene& d, const host_mirrors& h, long long num_shape_nodes, scene_updater& u, const vpt_scene_edit& edit, bool lights = false);
