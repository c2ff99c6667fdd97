// vpt_scene_prep.h — host half of vpt_scene_create: a vpt_scene_desc checked and turned into the tables of the device
// layout (vpt_device.h), in host memory.  No device call: vpt_capi.hip uploads the tables, one allocation each.
#pragma once
#include <vector>

#include "vpt_device.h"

// host copies of a few index tables: range checks of the batch entry points (vpt_intersect, vpt_kat)
struct host_mirrors {
  std::vector<int> slot_of;   // instance -> scene-BVH primitive slot (-1: not in the scene BVH); also a device table
  std::vector<int> inst_shape, shape_elems, shape_elem_offset;
  std::vector<int> shape_vertices;   // vertices per shape (vpt_scene_update: the size of a vertex edit)
  std::vector<int> prim_slot;   // [shape elem_offset + element] -> slot in leaf_prims / leaf_attrs
};

// Host copies of the small tables an edit of the resident scene is checked against and its light list is decided from
// (vpt_resident.h), and the entry counts of the pooled tables.  Made here, from the descriptor and the tables, moved into the
// handle with host_mirrors and kept current by every edit: never read back from the device.
struct edit_mirrors {
  std::vector<vpt_material>    materials;
  std::vector<vpt_environment> environments;
  std::vector<vpt_texture>     textures;     // a texture is an emitter's when the emission_tex of an environment with non-zero emission names it
  std::vector<char>            textured;     // material bound to a mesh instance: its texture ids are range-checked
  std::vector<DShape>          shapes;       // offsets, counts and root_ref (root_box: creation's, the device refits its own)
  std::vector<int>             inst_material, inst_flags;   // DInstance::material / shape_flags
  std::vector<int>             shape_flags;   // VPT_SHP_* of every shape: the shape_flags of an instance that is bound to it later
  std::vector<vpt_light>       lights;
  std::vector<int>             light_kind;   // VPT_LIGHT_* of every light record (the tag of its last word)
  std::vector<char>            shape_lit;    // some light's instance uses the shape
  std::vector<DCdfIndex>       light_index;
  std::vector<vpt_sdf>         sdfs;
  std::vector<vpt_volume>          volumes;
  std::vector<vpt_volume_instance> vol_instances;
  // entries of the pooled tables the device holds now: a texture, a volume or a light that needs more room gets it in a pool made anew
  long long num_cdf = 0, num_pool = 0, num_guide = 0, num_texels_f = 0, num_texels_b = 0, num_voxels = 0;
};

struct scene_tables {
  // the scalar fields of DScene: counts, scene_root_*, group_forms, sdf_bound_*, sdf_num_planes; the table pointers stay null
  DScene d = {};
  // geometry: vertex pools, shapes and their elements, leaf records and their vertex attributes in BVH leaf order
  std::vector<float4> positions, normals, colors;
  std::vector<float2> texcoords;
  std::vector<DShape> shapes;
  std::vector<int4>   elems;
  std::vector<float4> leaf_prims, leaf_attrs;
  std::vector<float4> tri_prims, tri_attrs;   // the compact records: empty unless every shape holds triangles
  // quad nodes of all BVHs in one table: the scene's first (scene_wnodes float4s), then the shapes'
  std::vector<float4> wnodes;
  size_t              scene_wnodes = 0, shape_wnodes = 0;   // float4s of the two parts
  int                 shape_depth = 0, shape_need4 = 0;    // the deepest shape BVH, the largest quad-stack need of a shape
  std::vector<int>    shape_depths, shape_need4s, shape_quads;   // the same per shape, and its quad nodes: the maxima are over these
  int                 scene_depth = 0, scene_need4 = 0;    // of the scene BVH
  std::vector<float4> enter;
  std::vector<DInstance> instances;
  std::vector<float4> env_inv, sdf_inv;
  std::vector<float>  srgb_lut;
  std::vector<DCdfIndex> light_index;   // + its pool and guide table
  std::vector<float>     light_index_pool;
  std::vector<int2>      light_guide;
  std::vector<float4>    light_rec, sdf_fn_rec, sdf_grid_rec;
  // traversal stacks: binary-BVH walk of the implicit kernels (refs only); quad-node traversal entries in LDS / in HBM
  int stack_cap = 16, stack_lds4 = 8, stack_spill4 = 0;
  int light_features = 0;   // VPT_FEAT_* bits this scene's lights need from the mesh kernels
  bool curves = false;      // some instanced shape holds points or lines: the mesh kernels' VPT_FEAT_CURVES instances
  bool varying_media = false;   // prep_media_vary() of the scene
  host_mirrors h;
  edit_mirrors m;
};

// validate(desc, curves), then every table (curves may be null: no shape has points or lines); VPT_ERR_INVALID_ARG for a bad descriptor, VPT_ERR_UNSUPPORTED for a scene past a traversal
// limit or with a shape that mixes points, lines and faces
int prepare_scene(const vpt_scene_desc& desc, const vpt_scene_curves* curves, scene_tables& out);

// Pieces of the layout that vpt_scene_update (vpt_scene_update.hip) needs for a resident scene, so that the tables keep one description:
// the packed inverse (adjoint over determinant) and forward frame of an instance with its translation_only flag; of an environment
// (rigid inverse); the rule of validate() for one material; and, per quad node of a BVH in the order build_quad_nodes emits them,
// the four binary nodes its slots hold (appended to `slots`, -1: empty slot).
void prep_instance_frames(const vpt_frame& frame, float4 inv[3], float4 fwd[3], int* translation_only);
void prep_environment_frames(const vpt_frame& frame, float4 inv[3], float4 fwd[3]);
int  prep_check_material(const vpt_material& m, int index, int num_textures, bool textured);
void prep_quad_slots(const vpt_bvh_node* nodes, int count, std::vector<int>& slots);
// What hangs on the TOPOLOGY of the BVHs, for vpt_scene_create and for vpt_scene_rebuild_bvh (vpt_bvh_rebuild.hip), which calls it with a
// descriptor that carries nothing but the node arrays it built: the quad nodes of every BVH (out.wnodes: the scene's, out.scene_wnodes
// float4s, then the shapes' in shape order), wnode_offset / root_ref / root_box / stack_need of every out.shapes[i], out.d.scene_root_*,
// and the stack sizes out.stack_cap / stack_lds4 / stack_spill4 (VPT_STACK_LDS and VPT_DEBUG are read here).  Reads of `desc`:
// num_shapes, shapes[i].bvh_node_offset / num_bvh_nodes, shape_bvh_nodes, scene_bvh_nodes, num_scene_bvh_nodes; of `out`: shapes[i].num_nodes.
// VPT_ERR_UNSUPPORTED for trees past a traversal limit: the 256-entry LDS stack, the packed pop floor, 2^27 quad nodes.
// shapes_kept (vpt_scene_update_instances, vpt_instance_update.hip: only the scene BVH is new): the shapes' part is not made -
// out.wnodes holds the scene's quad nodes alone, out.shapes is not written - and what the limits need to know of the shapes is read
// from out.shape_depth / shape_need4 / shape_wnodes, which every call without the flag leaves there.
// shape_made (vpt_scene_update_shapes, vpt_shape_update.hip: some shapes are new, the others keep their trees), one flag per shape:
// quad nodes, root_ref, root_box and stack_need are made for the flagged shapes alone - out.wnodes holds theirs, in shape order, behind
// the scene's - while a kept shape's depth, need and number of quad nodes are read from out.shape_depths / shape_need4s / shape_quads,
// which every call without shapes_kept leaves there per shape; wnode_offset is numbered for all, out.shape_wnodes counts all.
// scene_kept (the same unit, when the scene BVH stays): nothing of the scene BVH is made or read from `desc`; out.scene_depth,
// scene_need4 and scene_wnodes, which every other call leaves there, are read instead, and out.d.scene_root_* is not written.
int prep_quad_nodes_and_stacks(const vpt_scene_desc& desc, scene_tables& out, bool shapes_kept = false, const char* shape_made = nullptr, bool scene_kept = false);
// validate()'s rules for the elements of one shape, for vpt_scene_create and for the shapes of a vpt_shape_edit: not both triangles and
// quads; points, lines and faces not mixed (VPT_ERR_UNSUPPORTED); every vertex index in range.  The lists are the shape's own; i names it.
int prep_check_shape_elements(int i, int num_vertices, const int32_t* triangles, int num_triangles, const int32_t* quads, int num_quads, const int32_t* points,
    int num_points, const int32_t* lines, int num_lines);
// the integer words of the enter record `e` (6 float4) of the scene-BVH slot that holds `instance`: e4.zw = root_ref, first quad node of
// the shape in the one quad-node array (scene_quads = the scene BVH's own); e5 = leaf_offset, instance, translation_only, num_nodes
void prep_enter_tail(float4* e, const DShape& shape, int scene_quads, int instance, int translation_only);
// Whether the medium behind some instance is more than a function of its material (vpt_device.h: medium records): a material of a
// volumetric type with a colour, emission or scattering texture or on a shape with vertex colours - or more materials than the
// path state's 16-bit id holds.  Such scenes render with K1's general instance, which carries the medium in registers.
bool prep_media_vary(const vpt_material* materials, int num_materials, const int* inst_material, const int* inst_flags, int num_instances);
// The SDF side of the layout, for vpt_scene_create and for vpt_scene_update_volumes (vpt_volume_update.hip): the inverse frames of
// the SDFs (3 float4 each), the evaluation records of the SDFs (6 float4 each) and of the grid instances (7 float4 each, the
// volume's offset in two words), and in D the scene's bounding ball (sdf_bound_*) and sdf_num_planes.  Always every record of a scene.
void prep_sdf_records(const vpt_sdf* sdfs, int num_sdfs, const vpt_volume* volumes, const vpt_volume_instance* vol_instances, int num_vol_instances,
    std::vector<float4>& sdf_inv, std::vector<float4>& sdf_fn_rec, std::vector<float4>& sdf_grid_rec, DScene& D);
