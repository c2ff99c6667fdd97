// vpt_resident.h — the part of a vpt_scene that the edits of a resident scene work on (include/vpt.h: vpt_scene_update, _lights,
// _textures, _volumes, and vpt_scene_rebuild_bvh): the tables on the device, their host mirrors, and what an edit keeps between calls.  vpt_scene_handle.h's
// vpt_scene is a `resident` plus its render side (schedule, staging, stacks); the update units and the read-backs of
// vpt_scene_inspect.hip see only this.
#pragma once
#include <algorithm>
#include <vector>

#include "vpt_device_buffer.h"
#include "vpt_scene_prep.h"
#include "vpt_subdiv.h"

// The internal nodes of one BVH by depth: nodes of depth l are order[first[l] .. first[l + 1]) of refit_tables::d_order (ids
// local to the BVH).  A refit walks the levels deepest first.
struct bvh_levels {
  std::vector<int> first;        // depth + 1 entries; empty: no internal node
  long long        offset = 0;   // of this BVH's part of d_order
};

// What a refit needs beyond the scene's own tables.  The one thing built late: by the first edit of a handle that moves an
// instance or a vertex (vpt_scene_update.hip), from the node arrays the device holds, and kept until the topology changes:
// vpt_scene_rebuild_bvh (vpt_bvh_rebuild.hip) clears `ready`, and the next refit makes them from the new trees.
struct refit_tables {
  bool ready = false;
  bvh_levels              scene_levels;
  std::vector<bvh_levels> shape_levels;
  device_buffer d_order;        // int
  device_buffer d_quad_slots;   // int4 per quad node of DScene::scene_wnodes: the binary nodes behind its slots (prep_quad_slots), local to the BVH
  long long     scene_quads = 0;   // quad nodes of the scene BVH (the shapes' follow at DShape::wnode_offset)
  std::vector<long long> shape_quads;   // per shape
  device_buffer d_inst_box;     // 2 float4 per instance: transform_bbox(frame, shape root box)
};

// One attached tesselation plan (include/vpt.h: vpt_scene_attach_subdiv; vpt_subdiv_update.hip): the settings, and ONE allocation that
// holds the uploaded tables, the cage's floats as the device keeps them, and the scratch of an edit - so an edit allocates nothing.
// Every pointer below points into `block`.  shape < 0: a free slot (the plan was detached, or its shape was replaced or removed).
struct subdiv_plan_dev {
  int   shape = -1, subdivisions = 0, smooth = 0, displacement_tex = -1;
  float displacement = 0;
  int   num_cage = 0, num_cage_normals = 0, num_refined = 0, num_quads = 0, num_vertices = 0;   // num_refined: positions after the last level
  std::vector<subdiv_level_dev> levels;
  device_buffer block;
  size_t        block_bytes = 0;
  float*      cage         = nullptr;   // float3 x num_cage
  const float* cage_normals = nullptr;  // float3 x num_cage_normals
  const int4* quads        = nullptr;   // the final quadspos, with quads_normals' face lists (smooth and subdivisions > 0)
  const int * quad_offsets = nullptr, *quad_items = nullptr;
  const int * verts        = nullptr;   // int3 x num_vertices
  const int * tri_offsets  = nullptr, *tri_items = nullptr;   // triangles_normals' face lists (displacement_tex >= 0)
  float *buf0 = nullptr, *buf1 = nullptr, *tverts = nullptr;  // float3 x the widest level each
  float *refined_normals = nullptr;     // float3 x num_refined
  float *stage_pos = nullptr, *stage_nrm = nullptr, *stage_tmp = nullptr;   // float3 x num_vertices each
};

inline int most_of(const std::vector<int>& v) { return v.empty() ? 0 : std::max(0, *std::max_element(v.begin(), v.end())); }

struct resident {
  int                        device = 0;
  DScene                     d      = {};
  std::vector<device_buffer> tables;   // one allocation per table of d
  host_mirrors h;                      // range checks of vpt_intersect, vpt_kat; sizes of a vertex edit
  edit_mirrors m;                      // as vpt_scene_create made them, as the last edit left them
  long long    num_shape_nodes = 0;    // nodes of d.shape_nodes
  long long    num_shape_wnodes = 0;   // float4s of d.shape_wnodes; with the vectors below, what prep_quad_nodes_and_stacks found of the
  // shapes' trees, per shape: binary depth, quad-stack need, quad nodes.  An edit that builds the scene BVH alone decides the traversal
  // limits from their maxima (vpt_instance_update.hip); one that changes the shape list keeps the untouched shapes' (vpt_shape_update.hip)
  std::vector<int> shape_depth, shape_need4, shape_quads;
  int          scene_depth = 0, scene_need4 = 0;   // the same of the scene BVH, for an edit that keeps it
  long long    num_positions = 0, num_normals = 0, num_texcoords = 0, num_colors = 0;   // entries of the four vertex pools
  int          light_features  = 0;      // VPT_FEAT_* bits this scene's lights need from the mesh kernels
  bool         varying_media   = false;  // prep_media_vary of m.materials: K1's general instance, which carries a path's medium in registers
  refit_tables refit;
  std::vector<subdiv_plan_dev> subdivs;   // the attached tesselation plans by subdiv id (vpt_subdiv_update.hip)
  // buffers of an edit on its way to the tables, kept from call to call
  device_buffer d_stage;   // vpt_scene_update: moved vertices and frames
  size_t        stage_bytes = 0;
  device_buffer d_jobs, d_result, d_tags;   // a light rebuild: the recomputed lights' descriptors, {sorted, last entry} per job, record tags per light
  device_buffer d_sin;     // sin((j + 0.5f) * pif / height) per row of the recomputed environments, made on the host
  // what the last edit did (vpt_scene_update_stats): begin_update (vpt_update_helpers.h) starts them, launches and sends count themselves
  int        last_launches = 0;
  long long  last_bytes    = 0;
  float      last_ms       = 0;   // device time between the two events (stream 0)
  hipEvent_t upd_ev0 = nullptr, upd_ev1 = nullptr;   // made by the first edit, destroyed by vpt_scene_destroy
};

// What an edit did that the render side of the handle must follow (vpt_capi.hip: edit_scene, which hands it to the unit's *_apply).
// The stacks and `curves` start as the handle's own values: a unit that leaves them alone leaves them as they are.
struct edit_outcome {
  bool changed        = false;   // false: nothing was launched or sent, the counters of vpt_scene_update_stats are the last edit's
  bool lights_rebuilt = false;   // the light tables were made anew: light_prims and the medium records sit in fresh allocations
  bool topology       = false;   // trees or lists were replaced, not refitted: the four values below are the new scene's
  int  stack_cap, stack_lds4, stack_spill4;   // the traversal stacks (vpt_scene_prep.h: prep_quad_nodes_and_stacks)
  bool curves;                   // some instanced shape holds points or lines (VPT_FEAT_CURVES)
};

// the resident part of a handle (not null), for a unit that sees no more of it: vpt_capi.hip defines it
const resident& resident_of(const vpt_scene* s);
