/* include/vpt.h — C-ABI of the MI355X volumetric path-tracing integrator (libvpt_hip.so).
 *
 * This is the drop-in boundary for ONE function of the reference:
 *
 *   void pathtrace_samples(pathtrace_state&, const scene_data&, const bvh_scene&,
 *                          const pathtrace_lights&, const pathtrace_params&)
 *                                      libs/yocto_pathtrace/yocto_pathtrace.h:133-135
 *                                      libs/yocto_pathtrace/yocto_pathtrace.cpp:1052-1092
 *
 * The reference has no FFI of its own: its seam is that C++ free
 * function, whose arguments are STL containers.  The C-ABI below is what a maintainer binds
 * behind it: plain pointers + counts to the *flattened* forms of the same four inputs
 * (INTEGRATION.md shows the ~80-line flattening stub for the reference tree).
 *
 * Conventions
 *  - every struct is little-endian POD with the reference's field order where one exists;
 *  - indices are int32, -1 (VPT_INVALID) == reference `invalidid`;
 *  - frames are 12 floats, column layout x,y,z,o (yocto_math.h:1099-1107);
 *  - nothing here owns caller memory: vpt_scene_create() copies everything to the device;
 *  - all entry points return 0 on success, a negative vpt_status otherwise, and never throw;
 *    the message for the last failure on the calling thread is vpt_last_error().
 */
#ifndef VPT_H_
#define VPT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VPT_INVALID (-1)

typedef enum vpt_status {
  VPT_OK                = 0,
  VPT_ERR_INVALID_ARG   = -1, /* null pointer, bad size, index out of range                */
  VPT_ERR_NO_DEVICE     = -2, /* no gfx950 device / HIP runtime unavailable                */
  VPT_ERR_HIP           = -3, /* a HIP call failed (message has hipGetErrorString)         */
  VPT_ERR_UNKNOWN_SHADER = -4, /* reference: get_shader throws "sampler unknown" (cpp:947) */
  VPT_ERR_UNSUPPORTED   = -5  /* scene outside the hot-path scope: a traversal limit, or a
                                  shape that mixes points / lines with faces or with each other */
} vpt_status;

/* pathtrace_shader_type, yocto_pathtrace.h:74-84 (same order, same names) */
typedef enum vpt_shader {
  VPT_SHADER_VOLPATHTRACE    = 0,
  VPT_SHADER_PATHTRACE       = 1,
  VPT_SHADER_NAIVE           = 2,
  VPT_SHADER_EYELIGHT        = 3,
  VPT_SHADER_NORMAL          = 4,
  VPT_SHADER_TEXCOORD        = 5,
  VPT_SHADER_COLOR           = 6,
  VPT_SHADER_IMPLICIT        = 7,
  VPT_SHADER_IMPLICIT_NORMAL = 8,
  /* ids 9 .. 15 name nothing and stay refused (VPT_ERR_UNKNOWN_SHADER, "sampler unknown"); the extension shaders start at 16 */
  VPT_SHADER_VOLGRID         = 16  /* not the reference's: the voxel-grid instances as heterogeneous media ("the volgrid shader" below) */
} vpt_shader;
/* 1 for a shader id some kernel renders (0 .. 8 and 16), 0 for every other: what each entry point that takes vpt_params asks */
int vpt_shader_known(int shader_id);

/* material_type, yocto_scene.h:105-110 */
typedef enum vpt_material_type {
  VPT_MAT_MATTE = 0, VPT_MAT_GLOSSY = 1, VPT_MAT_REFLECTIVE = 2, VPT_MAT_TRANSPARENT = 3,
  VPT_MAT_REFRACTIVE = 4, VPT_MAT_SUBSURFACE = 5, VPT_MAT_VOLUMETRIC = 6, VPT_MAT_GLTFPBR = 7
} vpt_material_type;

/* sdf_type, yocto_sdfs.h:23 */
typedef enum vpt_sdf_type {
  VPT_SDF_BBOX = 0, VPT_SDF_BOX = 1, VPT_SDF_CAPPED_CONE = 2, VPT_SDF_PLANE = 3,
  VPT_SDF_SPHERE = 4, VPT_SDF_TORUS = 5
} vpt_sdf_type;

/* frame3f, yocto_math.h:1099-1107 */
typedef struct vpt_frame { float x[3], y[3], z[3], o[3]; } vpt_frame;

/* camera_data, yocto_scene.h:84-92 */
typedef struct vpt_camera {
  vpt_frame frame;
  int32_t   orthographic;
  float     lens, film, aspect, focus, aperture;
} vpt_camera;

/* bvh_node, yocto_bvh.h:73-79 — identical 32-byte layout */
typedef struct vpt_bvh_node {
  float   bbox_min[3], bbox_max[3];
  int32_t start;    /* first child (internal) or first slot in the primitive array (leaf) */
  int16_t num;      /* 2 (internal) or #primitives (leaf, <= 4)                            */
  int8_t  axis;     /* split axis                                                          */
  uint8_t internal; /* bool                                                                */
} vpt_bvh_node;

/* shape_data, yocto_shape.h:74-87 — offsets into the pooled vertex / element arrays.
 * Element indices stay shape-local (add *_offset when fetching).  At most one of
 * num_triangles / num_quads is non-zero; a shape of points or lines has neither and is
 * described by its entry in vpt_scene_curves::shape_curves. */
typedef struct vpt_shape {
  int32_t num_vertices;
  int32_t position_offset;  /* into positions[] (float3 units)                */
  int32_t normal_offset;    /* into normals[]   (float3 units), -1 if absent  */
  int32_t texcoord_offset;  /* into texcoords[] (float2 units), -1 if absent  */
  int32_t color_offset;     /* into colors[]    (float4 units), -1 if absent  */
  int32_t num_triangles, triangle_offset; /* into triangles[] (int3 units)    */
  int32_t num_quads, quad_offset;         /* into quads[]     (int4 units)    */
  int32_t num_bvh_nodes, bvh_node_offset; /* into shape_bvh_nodes[]           */
  int32_t bvh_prim_offset;                /* into shape_bvh_prims[]           */
} vpt_shape;

/* instance_data, yocto_scene.h:143-149 */
typedef struct vpt_instance {
  vpt_frame frame;
  int32_t   shape;
  int32_t   material;
} vpt_instance;

/* material_data, yocto_scene.h:121-140 */
typedef struct vpt_material {
  int32_t type;
  float   emission[3];
  float   color[3];
  float   roughness, metallic, ior;
  float   scattering[3];
  float   scanisotropy, trdepth, opacity;
  int32_t emission_tex, color_tex, roughness_tex, scattering_tex, normal_tex;
} vpt_material;

/* texture_data, yocto_scene.h:96-102 — pixels live in one of two pools */
typedef struct vpt_texture {
  int32_t width, height;
  int32_t linear;   /* texture_data::linear                                     */
  int32_t is_float; /* 1: pixelsf (float4 pool), 0: pixelsb (uchar4 pool)       */
  int64_t offset;   /* first texel, in texels, inside its pool                  */
} vpt_texture;

/* environment_data, yocto_scene.h:152-157 */
typedef struct vpt_environment {
  vpt_frame frame;
  float     emission[3];
  int32_t   emission_tex;
} vpt_environment;

/* volume<float>, yocto_scene.h:203-212 */
typedef struct vpt_volume {
  int32_t whd[3];
  float   res;
  int64_t offset; /* first voxel inside voxels[]; index x + y*W + z*W*H */
} vpt_volume;

/* volume_instance, yocto_scene.h:214-219 */
typedef struct vpt_volume_instance {
  vpt_frame frame;
  int32_t   volume;
  int32_t   material;
  float     scalef;
} vpt_volume_instance;

/* sdf_data, yocto_scene.h:194-200.  The reference stores a std::function built in
 * yocto_sceneio.cpp:3684-3730; here it is a tagged union:
 *   BBOX        p = {thickness, w, h, d}   sd_bbox(p, {w,h,d}, thickness)
 *   BOX         uses whd                   sd_box(p - whd/2, whd/2)
 *   CAPPED_CONE p = {height, r1, r2}
 *   PLANE       —
 *   SPHERE      p = {radius}
 *   TORUS       p = {r1, r2}
 * `whd` is sdf_data::whd (only set for BOX; used by the SDF light sampling). */
typedef struct vpt_sdf {
  vpt_frame frame;
  int32_t   type;
  int32_t   material;
  float     whd[3];
  float     p[4];
} vpt_sdf;

/* pathtrace_light, yocto_pathtrace.h:106-111 */
typedef struct vpt_light {
  int32_t instance, environment, sdf;
  int32_t cdf_len;
  int64_t cdf_offset; /* into light_cdf[] */
} vpt_light;

/* The points / lines of a shape (shape_data::points, lines, radius; yocto_shape.h:74-87), in the side array
 * vpt_scene_curves::shape_curves (below).  A shape holds points OR lines OR faces: a shape that mixes them has no single
 * behaviour in the reference (its BVH tests points first, its eval_* functions triangles first) and is refused
 * with VPT_ERR_UNSUPPORTED.  Indices stay shape-local, as for faces.  Shapes of points or lines are never lights
 * (make_lights, yocto_pathtrace.cpp:992): an emissive one emits when hit and is never sampled. */
typedef struct vpt_shape_curves {
  int32_t num_points, point_offset;  /* into points[] (int units)                                  */
  int32_t num_lines, line_offset;    /* into lines[]  (int2 units)                                 */
  int32_t radius_offset;             /* into radius[] (num_vertices floats), -1 if absent: only a
                                        shape without points and lines may omit it                 */
} vpt_shape_curves;

/* The flattened (scene_data, bvh_scene, pathtrace_lights) triple. */
typedef struct vpt_scene_desc {
  int32_t num_cameras;       const vpt_camera*          cameras;
  int32_t num_instances;     const vpt_instance*        instances;
  int32_t num_shapes;        const vpt_shape*           shapes;
  int32_t num_materials;     const vpt_material*        materials;
  int32_t num_textures;      const vpt_texture*         textures;
  int32_t num_environments;  const vpt_environment*     environments;
  int32_t num_volumes;       const vpt_volume*          volumes;
  int32_t num_vol_instances; const vpt_volume_instance* vol_instances;
  int32_t num_sdfs;          const vpt_sdf*             sdfs;
  int32_t num_lights;        const vpt_light*           lights;

  /* pooled vertex / element data (counts in elements of the stated unit) */
  int64_t num_positions;  const float*   positions;  /* float3 */
  int64_t num_normals;    const float*   normals;    /* float3 */
  int64_t num_texcoords;  const float*   texcoords;  /* float2 */
  int64_t num_colors;     const float*   colors;     /* float4 */
  int64_t num_triangles;  const int32_t* triangles;  /* int3   */
  int64_t num_quads;      const int32_t* quads;      /* int4   */

  /* texture / voxel / cdf pools */
  int64_t num_texels_f;   const float*   texels_f;   /* float4 */
  int64_t num_texels_b;   const uint8_t* texels_b;   /* uchar4 */
  int64_t num_voxels;     const float*   voxels;
  int64_t num_light_cdf;  const float*   light_cdf;

  /* two-level BVH, bvh_data yocto_bvh.h:87-92 */
  int32_t num_scene_bvh_nodes;  const vpt_bvh_node* scene_bvh_nodes;
  int32_t num_scene_bvh_prims;  const int32_t*      scene_bvh_prims; /* instance ids */
  int64_t num_shape_bvh_nodes;  const vpt_bvh_node* shape_bvh_nodes; /* pooled */
  int64_t num_shape_bvh_prims;  const int32_t*      shape_bvh_prims; /* pooled, element ids */
} vpt_scene_desc;

/* The points and lines of a scene, BESIDE its descriptor: vpt_scene_desc keeps the layout that binaries built against earlier
 * versions of this header fill in, and vpt_scene_create / vpt_multi_create keep meaning "no shape has points or lines".
 * shape_curves: one entry per shape of the descriptor (desc->num_shapes); the pools are shared by all shapes.  The shape BVH of a
 * points / lines shape is built over point_bounds(p, r) / line_bounds(p0, p1, r0, r1) (yocto_bvh.cpp:537-549). */
typedef struct vpt_scene_curves {
  const vpt_shape_curves* shape_curves;
  int64_t num_points;     const int32_t* points;     /* int    */
  int64_t num_lines;      const int32_t* lines;      /* int2   */
  int64_t num_radius;     const float*   radius;     /* float  */
} vpt_scene_curves;

/* pathtrace_params, yocto_pathtrace.h:87-99 (fields the path reads) */
typedef struct vpt_params {
  int32_t camera;
  int32_t resolution;
  int32_t shader;   /* vpt_shader */
  int32_t samples;  /* total samples requested: the call is a no-op once reached (cpp:1055);
                       ==1 selects the pixel-centre preview branch (cpp:1059-1068)          */
  int32_t bounces;
  int32_t noparallel;          /* accepted, ignored (one lane per pixel)                    */
  int32_t noimplicit_mis;
  int32_t spheretrace_maxiter;
} vpt_params;

/* Opaque device-side scene.  NOT thread-safe: a handle carries the launch schedule and staging buffers of its last
 * call, so calls on ONE handle must not overlap (the reference serialises its own calls the same way);
 * different handles may be used from different threads.  Launches on one handle may move between streams: the schedule
 * tables written on the previous launch's stream are waited for. */
typedef struct vpt_scene vpt_scene;

/* How pixels are laid out in device-resident state and shared between GPUs.
 * The image is cut into tile_w x tile_h pixel tiles (row-major tile order); tile t belongs
 * to rank (t % nranks) and is that rank's local tile (t / nranks).  A rank's state arrays are
 * TILE-MAJOR and compact: local index l = local_tile * (tile_w*tile_h) + (py*tile_w + px).
 * Slots whose pixel falls outside the image are padding and never touched. */
typedef struct vpt_layout {
  int32_t width, height;
  int32_t tile_w, tile_h; /* tile_w*tile_h must be a multiple of 64 (one wave64 per 8x8) */
  int32_t rank, nranks;
} vpt_layout;

/* ---- queries ----------------------------------------------------------------------- */
int         vpt_device_count(void);
const char* vpt_last_error(void);
const char* vpt_version(void);

/* ---- scene ------------------------------------------------------------------------- */
/* Validates every index/offset in `desc` against its pool, precomputes
 * inverse(frame, non_rigid=true) per instance with the reference's adjoint/determinant
 * formula (yocto_math.h:2802-2808, 2948-2956), uploads to `device`.                      */
int  vpt_scene_create(const vpt_scene_desc* desc, int device, vpt_scene** out);
/* the same for a scene whose shapes may hold points or lines (curves == NULL: vpt_scene_create) */
int  vpt_scene_create_curves(const vpt_scene_desc* desc, const vpt_scene_curves* curves, int device, vpt_scene** out);
void vpt_scene_destroy(vpt_scene* scene);

/* ---- editing a resident scene: cameras, frames, materials, vertices; BVHs refitted on the device -----------
 * The counterpart of the reference's update_bvh(bvh, scene, updated_instances, updated_shapes) (yocto_bvh.h:100-103,
 * yocto_bvh.cpp:509-524, 613-689) for a scene that lives on a GPU.  Topology, node ids, primitive order, leaf slots and every
 * count stay as they were at creation; boxes, records and frames are recomputed.  After vpt_scene_update(s, edit) every table on
 * the device holds the bytes vpt_scene_create would upload for the edited descriptor carrying the refitted BVH arrays, so every
 * render, vpt_intersect and vpt_kat call gives the bits of a fresh handle made from that descriptor.
 *  - Order of a refit = the reference's: edited shapes first, then the scene BVH from ALL instances (yocto_bvh.cpp:680-689:
 *    `updated_instances` is ignored by its non-Embree path and the scene BVH is refitted on every call); done here whenever the
 *    edit names an instance or a shape.
 *  - Boxes: leaf node = invalidb3f merged with its primitives' bounds in slot order; internal node = invalidb3f merged with
 *    child `start`, then `start + 1` (yocto_bvh.cpp:510-524).  Primitive bounds are triangle_bounds / quad_bounds /
 *    point_bounds(p, r) / line_bounds(p0, p1, r0, r1) (yocto_geometry.h:461-479), instance bounds transform_bbox(frame, shape
 *    root box) over the eight corners in the reference's order (yocto_geometry.h:441-451; transform_point with its own operation
 *    order, no contraction).  min / max are the reference's select forms ((a < b) ? a : b), applied in that order: with signed
 *    zeros the order decides the bits, so fminf / fmaxf or a reduction in another order are not equivalent.  An instance of a shape
 *    without BVH nodes gets invalidb3f, as in make_bvh (yocto_bvh.cpp:601-603; the reference's refit reads nodes[0] of an empty
 *    vector there).
 *  - Validation before anything is written: ids in range and not repeated within one list, every float of the edit finite,
 *    material types and texture ids under the rules of vpt_scene_create.  A refused edit leaves the scene exactly as it was
 *    (VPT_ERR_INVALID_ARG; the message names the entry).  A failure of the device after validation (VPT_ERR_HIP) is another matter:
 *    the tables may be half written and the handle is good for vpt_scene_destroy only.
 *  - What an edit may not do (VPT_ERR_UNSUPPORTED, scene unchanged): turn a material's emission from zero to non-zero or back
 *    (the light list and the kernel instances are fixed at creation); move the vertices of a shape that a light's instance uses
 *    (its element CDF is the caller's light_cdf, made from areas); change counts, indices or radii (the edit has no field for them;
 *    textures are vpt_scene_update_textures', volumes and SDFs vpt_scene_update_volumes').  Moving an emissive INSTANCE is allowed (the CDF is over shape-local areas).
 *  - Synchronisation: the call waits for the device's outstanding work (it rewrites tables launches read) and has completed when
 *    it returns.  It touches no pathtrace_state: restarting accumulation is the caller's business, as in the reference's
 *    reset_display.  It forgets the handle's launch-schedule record and tile-splitting decision (the camera index may be the
 *    same, the picture is not); results never depended on that record.
 *  - The traversal limits decided at creation (stack sizes) depend on topology only and stay valid. */
typedef struct vpt_scene_edit {
  int32_t num_cameras;      const int32_t* camera_ids;      const vpt_camera*   cameras;
  int32_t num_instances;    const int32_t* instance_ids;    const vpt_frame*    instance_frames;
  int32_t num_environments; const int32_t* environment_ids; const vpt_frame*    environment_frames;
  int32_t num_materials;    const int32_t* material_ids;    const vpt_material* materials;
  int32_t num_shapes;       const int32_t* shape_ids;       /* shapes whose vertices move                                  */
  const float* const* shape_positions;   /* per entry: that shape's num_vertices float3                                    */
  const float* const* shape_normals;     /* per entry: num_vertices float3 or NULL (keep); the array itself may be NULL    */
} vpt_scene_edit;
int vpt_scene_update(vpt_scene* scene, const vpt_scene_edit* edit);
/* The BVHs as the device holds them now, in the reference's layout (the descriptor's scene_bvh_nodes / shape_bvh_nodes): for
 * callers that keep a host copy, and for the tests.  *_capacity in nodes, at least the current counts (vpt_scene_get_bvh_counts; the
 * descriptor's for a handle that vpt_scene_rebuild_bvh never touched); a null array is skipped. */
int vpt_scene_get_bvh(vpt_scene* scene, vpt_bvh_node* scene_nodes, int scene_capacity, vpt_bvh_node* shape_nodes, int64_t shape_capacity);
/* What the last vpt_scene_update on this handle cost (measurements, tests): kernel launches, bytes of payload sent to the device, and
 * the time between two events on the device's null stream, one recorded before the first and one after the last launch of the refit -
 * the payload is on the device before the first, so the span holds launches only (0 for an edit of cameras, materials and environments:
 * it launches nothing).  VPT_UPDATE_NO_FUSE=1 in the environment, read per call, runs the refit with one launch per level throughout
 * instead of finishing the narrow top levels of a tree in one launch: same bits (the tests' and the measurements' A/B switch). */
int vpt_scene_update_stats(const vpt_scene* scene, int* launches, int64_t* bytes, float* device_ms);

/* ---- edits that change the lights: the light tables rebuilt on the device ------------------------------------------
 * vpt_scene_update_lights takes the edit of vpt_scene_update under the same validation with its two refusals about lights lifted:
 * a material's emission may switch between zero and non-zero, and the vertices of a shape that a light's instance uses may move.
 * vpt_scene_update itself is unchanged and keeps refusing both.
 *  - The refit runs exactly as in vpt_scene_update (edited shapes first, then the scene BVH).  Afterwards every light table on the
 *    device - lights, light_cdf, the light records, light_prims, the search index with its pool, the guide table, num_lights -
 *    holds the bytes vpt_scene_create would upload for the edited descriptor carrying make_lights of the edited scene, so every
 *    render, vpt_intersect and vpt_kat call gives the bits of a fresh handle.
 *  - The list = make_lights (yocto_pathtrace.cpp:983-1049): instances in id order whose material has emission != 0 and whose shape
 *    holds triangles or quads (shapes of points or lines never become lights); then the environments in id order (the edit has no
 *    field for their emission or texture: their entries and CDFs are kept byte for byte); then SDFs in id order whose material is
 *    emissive, cdf = {whd.x * whd.y}.  An empty list is valid.  cdf_offset = the sum of the earlier lengths.
 *  - The element CDF: cdf[0] = area_0, cdf[i] = area_i + cdf[i - 1], float32, in element order; triangle_area = length(cross(p1 - p0,
 *    p2 - p0)) / 2, quad_area = triangle_area(p0, p1, p3) + triangle_area(p2, p3, p1) (yocto_geometry.h:506-518); no operation fused,
 *    the square root correctly rounded.  Float addition is not associative: the additions run in the reference's order, a serial
 *    chain per light (lights side by side), never a tree or a block scan.  A mesh light's CDF is recomputed only when the light is
 *    new or its shape is in the edit; every other CDF, the environment's included, moves device to device.  Nothing proportional to
 *    an element or texel count crosses PCIe: vpt_scene_update_stats counts the edit's payload plus a few words per light.
 *  - The search structures of the recomputed lights are those of creation: an index only for more than 64 non-decreasing entries
 *    (NaN: none), 16-ary levels padded with +inf, the guide table with the same double-precision bounds, nextafter widening and
 *    upper_bound brackets.  A light whose CDF moved keeps its index, offsets rebased.
 *  - The kernel instances follow the new list (the features the lights need are recomputed): an all-triangle scene that gains an
 *    emissive mesh with a BVH leaves the compact-record instance, K2's lean instance follows the same rule.  Stack sizes depend on
 *    topology and stay.
 *  - An edit without consequence for the lights - the list stays as it is and no moved shape belongs to one of its lights - does
 *    exactly what vpt_scene_update does: the same launches, the same bytes.
 *  - Synchronisation, failure semantics and the forgetting of the launch-schedule record: those of vpt_scene_update.
 *  - VPT_LIGHTS_PLAIN=1 in the environment, read per call, runs the running sum as one lane per light straight from global memory
 *    instead of the wave form (64 areas per load, the chain through a cross-lane move): same bits (the tests' and the measurements'
 *    A/B switch). */
int vpt_scene_update_lights(vpt_scene* scene, const vpt_scene_edit* edit);
/* The light list and the CDF pool as the device holds them now, for callers that keep a host copy, and for the tests.  Capacities
 * in entries; a null array is skipped; *num_lights / *num_cdf (either may be null) are set even when a capacity is too small. */
int vpt_scene_get_lights(vpt_scene* scene, vpt_light* lights, int light_capacity, int* num_lights, float* cdf, int64_t cdf_capacity, int64_t* num_cdf);
/* The medium records as the device holds them now, for the tests: 12 floats per material = density.xyz, scattering.xyz, emission.xyz,
 * scanisotropy, 0, 0 - what a volumetric path carries of a material once it is inside (made on the device at creation, remade by
 * vpt_scene_update / vpt_scene_update_lights when materials change).  capacity in materials; a null array is skipped; *num_materials
 * (may be null) is set even when the capacity is too small.  *varying (may be null): 1 for a scene where a material of a volumetric
 * type has a colour, emission or scattering texture or sits on a shape with vertex colours - its media vary over the surface, and it
 * renders with the kernel instance that carries a path's medium along instead of reading these records.  VPT_MEDIUM_REGS=1 in the
 * environment, read per launch, renders any scene that way: same bits (the tests' A/B switch). */
int vpt_scene_get_media(vpt_scene* scene, float* records, int capacity, int* num_materials, int* varying);
/* FNV-1a (64 bit) over six things read back from the device: the light list, the CDF pool, the light records, light_prims, the
 * search index followed by its pool, the guide table.  For the tests: an updated handle against a fresh one. */
int vpt_scene_light_tables_hash(vpt_scene* scene, uint64_t out[6]);

/* ---- edits of environments and textures; the environment CDF rebuilt on the device -----------------------------------
 * vpt_scene_edit keeps its layout (older binaries fill it in); what it has no field for comes in a struct of its own.  An
 * environment entry replaces that environment's frame, emission and emission_tex; a texture entry replaces ALL texels of one
 * texture: width, height, linear and is_float describe the NEW contents, offset is the first texel inside THIS EDIT's pools
 * (texels_f: float4, texels_b: uchar4).  Counts stay fixed: no texture or environment is added.
 * After vpt_scene_update_textures(s, edit) every table on the device that a render, vpt_intersect or vpt_kat call reads holds what
 * vpt_scene_create would hold for the edited descriptor carrying the host's make_lights of the edited scene:
 * vpt_scene_light_tables_hash equals a fresh handle's on all six tables, vpt_scene_get_lights the host mirror's byte for byte, and
 * every render is bit-identical.  The layout of the texel pools is not part of the contract: nothing observable depends on a
 * texture's offset.  vpt_scene_update and vpt_scene_update_lights are unchanged and keep leaving environment entries alone.
 *  - The list = make_lights (yocto_pathtrace.cpp:1015-1032): an environment is a light iff its emission is not {0, 0, 0}; the
 *    environments come after the instance lights, in id order, before the SDF lights; an environment with a texture has cdf_len =
 *    width * height, otherwise 0.  Emission zero <-> non-zero therefore adds or removes a light and rebases every later cdf_offset;
 *    a scale between two non-zero values leaves every light table as it is and changes the environment's entry only.  Records
 *    follow vpt_scene_create: VPT_LIGHT_ENV_CONST / VPT_LIGHT_ENV_TEX, both frames, {width, height} and the CDF's total.
 *  - Textures: the same width, height and is_float overwrite the texture's range of its pool in place.  New dimensions or a new
 *    format give the texture fresh room at the end of a pool allocated anew, the old pool moved device to device; the range the
 *    texture leaves stays unused until vpt_scene_destroy (pools are never compacted).  A texture that a material names may be
 *    edited: the kernels read a texture's entry at use.  Only a light's CDF depends on texels: an edit of a texture that no
 *    emissive environment's emission_tex names launches nothing beyond the copies.
 *  - The environment CDF is recomputed when the environment's light is new, its emission_tex changed, or that texture is in the
 *    edit.  For idx in row-major order, i = idx % width, j = idx / width:
 *        w[idx] = max4(texel) * sin_row[j],   cdf[0] = w[0],   cdf[idx] = w[idx] + cdf[idx - 1]
 *    all in float32 with nothing fused.  max4 = max(max(max(x, y), z), w) with max(a, b) = (a > b) ? a : b (yocto_math.h:1356, 1824;
 *    alpha takes part; with NaN the select form decides, so fmaxf is not equivalent).  The texel is lookup_texture WITHOUT as_linear:
 *    a float4 as it is, a uchar4 as b / 255.0f per channel (a correctly rounded division, not the sRGB table).  sin_row[j] =
 *    sin((j + 0.5f) * pif / height) is computed ON THE HOST, where make_lights computes it, and sent as `height` floats: the device's
 *    sine is not the host's, and a 1-ulp difference moves the CDF.  One float per row is the only thing beyond the edit's own payload
 *    and a few words per light that crosses PCIe.  The running sum is the serial chain of vpt_scene_update_lights (VPT_LIGHTS_PLAIN=1:
 *    its plain form), never a tree or a block scan; the index, the guide table and the {sorted, last entry} read-back are that
 *    call's too: a CDF that is not non-decreasing (a negative or NaN texel) gets no index, exactly as at creation.  Every other
 *    light's CDF, index and guide table move device to device.
 *  - vpt_scene_update_stats afterwards: launches of the weight, running-sum, index, guide and record kernels; bytes = the edit's
 *    texels (16 or 4 each) + 24 per texture entry + 112 per environment entry (the entry and its inverse frame) + 4 * height per
 *    recomputed environment + 96 per environment light whose frame alone changed, and, when the light tables are rebuilt, per light
 *    84 (list entry 24, index header 56, record tag 4) + 128 per environment light (its record) + 4 per SDF light + 32 per
 *    recomputed CDF (job 24, result 8).  Nothing else is sent.  Device time: from before the first to after the last launch.
 *  - Validation before anything is written (VPT_ERR_INVALID_ARG, the message names the entry, the scene is untouched): ids in
 *    range and not repeated within a list; every float of an environment entry finite; emission_tex -1 or a texture id; width and
 *    height >= 0 with width * height < 2^31; offset >= 0 and offset + width * height inside the edit's pool; an emissive
 *    environment's texture must hold at least one texel, as at creation.
 *  - Synchronisation, the VPT_ERR_HIP semantics and the forgetting of the launch-schedule record: those of vpt_scene_update. */
typedef struct vpt_texture_edit {
  int32_t num_environments; const int32_t* environment_ids; const vpt_environment* environments; /* frame, emission, emission_tex */
  int32_t num_textures;     const int32_t* texture_ids;     const vpt_texture* textures;
      /* width, height, linear, is_float of the NEW contents; offset = first texel inside this edit's pools */
  int64_t num_texels_f; const float*   texels_f;   /* float4 */
  int64_t num_texels_b; const uint8_t* texels_b;   /* uchar4 */
} vpt_texture_edit;
int vpt_scene_update_textures(vpt_scene* scene, const vpt_texture_edit* edit);

/* ---- edits of volumes, grid instances and SDFs; baking into the resident voxel pool -----------------------------------
 * The `implicit` side of a resident scene: the voxel grids, the instances that place them and the analytic SDFs.  A struct of its own,
 * as for textures: vpt_scene_edit keeps its layout.  Counts stay fixed: no volume, instance or SDF is added or removed by this call
 * (that is vpt_scene_update_volume_set's, below), so the LDS budget of the implicit kernels' record copy stays as it was.
 * After vpt_scene_update_volumes(s, edit) every table on the device that a render, vpt_intersect or vpt_kat call reads holds what
 * vpt_scene_create would hold for the edited descriptor carrying the host's make_lights of the edited scene: every render is
 * bit-identical to a fresh handle's and vpt_scene_light_tables_hash equals a fresh handle's on all six tables.  The layout of the voxel
 * pool is not part of the contract: nothing observable depends on a volume's offset (vpt_scene_get_volumes reports the resident one).
 *  - Instances and SDFs.  An instance entry replaces frame, volume, material and scalef; an SDF entry replaces the whole vpt_sdf, type
 *    included.  The evaluation records (frame, sizes, the identity tag, dimensions, res and the two-word voxel offset of a grid
 *    instance), the inverse frames, the per-record bounding balls, the scene's bounding ball and the count of planes are remade by
 *    the function vpt_scene_create calls (vpt_scene_prep.h: prep_sdf_records), for ALL records, from host mirrors of the three small
 *    tables made when the handle is created and kept current by every edit: a res, dimension or offset change of a volume therefore reaches the record of every
 *    instance that names it.
 *  - Voxels from the host (offset >= 0).  whd and res describe the volume AFTER the edit; the entry writes the box region_lo ..
 *    region_lo + region_whd of it from edit->voxels + offset, region order, x fastest.  The same whd overwrites in place and any region
 *    box inside the grid is allowed (an empty one changes res alone).  A new whd requires the region to be the whole grid and mode
 *    REPLACE: the volume gets fresh room at the end of a pool allocated anew, the old pool moved device to device; the room the volume
 *    leaves stays unused until vpt_scene_destroy (the pool is never compacted).  The payload crosses PCIe once, into a staging buffer; a
 *    kernel writes the region from there.
 *  - VPT_VOXELS_UNION is the reference's op_union (yocto_sdfs.h:82) with a the resident and b the incoming value: (a < b) ? a : b - a
 *    select, never fminf: with a NaN on either side the select decides (a NaN resident value is replaced, a NaN incoming value stays).
 *  - Voxels baked (offset == -1).  bake is a vpt_bake_desc under the rules of vpt_bake_sdf with bake->whd equal to the entry's whd;
 *    origin and step are the caller's (fit_volume).  The values have the bits of vpt_bake_sdf for that descriptor - the same kernel
 *    body, instantiated with the pool as its destination: it runs only the bricks that touch the region, writes only the lanes inside
 *    it, and in UNION mode selects against the resident value.  No voxel crosses PCIe in either direction.  The host preparation
 *    (validation, feature normals, the tree through vpt_build_bvh, the depth check, the records) is vpt_bake_sdf's; a tree deeper than
 *    the kernel's stack gives VPT_ERR_UNSUPPORTED before anything is written.  VPT_BAKE_BRUTE=1 works as there.
 *  - Lights.  An SDF is a light iff its material is emissive (the materials as the handle holds them); its CDF is {whd.x * whd.y}.  When
 *    the edit changes which SDFs are lights (an entry's material) or the whd of an SDF that is a light, the light tables are rebuilt
 *    by the code of vpt_scene_update_lights, every other light's CDF, index and guide table moving device to device.  Otherwise
 *    nothing of the lights is touched.
 *  - Validation before anything is written (VPT_ERR_INVALID_ARG, the message names the entry, the scene is untouched): ids in range
 *    and not repeated within a list; every float finite (frames, scalef, whd, p, res; voxels are data and may hold anything); type in
 *    0..5; material and volume ids in range; whd >= 0 with a product below 2^31; the region inside whd; mode REPLACE or UNION; a new
 *    whd only with the whole grid and REPLACE; offset + region size inside the edit's pool; a bake descriptor valid and of the entry's
 *    whd.  (A volume id cannot be named by a host entry and a bake entry at once: ids are not repeated.)
 *  - vpt_scene_update_stats afterwards: launches = region kernels + bake kernels + those of a light rebuild; bytes = 4 per host voxel
 *    + 24 per volume entry + 60 per instance entry + 84 per SDF entry + the remade record tables (144 per SDF: 96 record, 48 inverse
 *    frame; 112 per grid instance) + per bake entry 32 per tree node and the size of its triangle records - not one voxel - + what a
 *    light rebuild sends (vpt_scene_update_textures).  Device time: from before the first to after the last launch.
 *  - Synchronisation, the VPT_ERR_HIP semantics and the forgetting of the launch-schedule record: those of vpt_scene_update. */
enum { VPT_VOXELS_REPLACE = 0, VPT_VOXELS_UNION = 1 };
struct vpt_bake_desc;   /* below: baking a mesh into a signed-distance voxel grid */
typedef struct vpt_volume_source {
  int32_t whd[3]; float res;            /* the volume AFTER the edit */
  int32_t region_lo[3], region_whd[3];  /* the box of voxels this entry writes */
  int32_t mode;                         /* VPT_VOXELS_REPLACE / VPT_VOXELS_UNION */
  int64_t offset;                       /* first voxel inside edit->voxels (region order, x fastest); -1: baked */
  const struct vpt_bake_desc* bake;     /* offset == -1: bake->whd must equal whd; origin / step are the caller's (fit_volume) */
} vpt_volume_source;
typedef struct vpt_volume_edit {
  int32_t num_vol_instances; const int32_t* vol_instance_ids; const vpt_volume_instance* vol_instances;
  int32_t num_sdfs;          const int32_t* sdf_ids;          const vpt_sdf* sdfs;
  int32_t num_volumes;       const int32_t* volume_ids;       const vpt_volume_source* volumes;
  int64_t num_voxels;        const float* voxels;
} vpt_volume_edit;
int vpt_scene_update_volumes(vpt_scene* scene, const vpt_volume_edit* edit);
/* The three small tables as the device holds them now, for callers that keep a host copy, and for the tests.  Capacities in
 * entries, at least the scene's counts; a null array is skipped.  A volume's offset is the resident pool's. */
int vpt_scene_get_volumes(vpt_scene* scene, vpt_volume* volumes, int volume_capacity, vpt_volume_instance* vol_instances, int instance_capacity,
                          vpt_sdf* sdfs, int sdf_capacity);
/* how many volumes, grid instances and SDFs the handle holds now: counts[0..2].  vpt_scene_update_volume_set changes them, so a caller
 * sizes the arrays of vpt_scene_get_volumes by this and not by the descriptor the handle was made from.  No device call. */
int vpt_scene_count_implicit(vpt_scene* scene, int32_t counts[3]);
/* the voxels of one volume as the device holds them (x + y*W + z*W*H); capacity in voxels, at least the volume's W*H*D */
int vpt_scene_get_voxels(vpt_scene* scene, int volume, float* voxels, int64_t capacity);

/* ---- sculpting the voxel grids of a resident scene with analytic SDF brushes ------------------------------------------
 * An edit of its own: vpt_volume_source keeps its layout and its two modes.  A stamp is an analytic brush (a vpt_sdf; its material is
 * ignored), an op and a blend width; an entry names a volume, a box of its voxels, the grid those voxels are sampled on and a run of the
 * edit's stamps - a stroke.  The kernel evaluates the brushes where the voxels live: no voxel crosses PCIe in either direction, a stroke
 * of any length reads and writes each voxel of its region once.  whd and res never change, so no record, no light table and no pool
 * layout is touched: only the voxels inside each entry's region change, every other voxel keeps its bits.
 * The rule, written once in csrc/vpt_sculpt_rule.h (compiled by the kernel and by the host mirror, host/vpt_sculpt.cpp, both with
 * -ffp-contract=off: float32, nothing fused, every sum in the order that header writes, division and square root the IEEE operations):
 *  - Sample point.  Voxel (i, j, k) is sampled at origin + (float)i * step per axis: vpt_bake_sdf's rule and the same voxel space as a
 *    bake.  Stored values are distances in that space, as a bake's are.
 *  - Brush distance.  f(transform_point(brush.frame, sample)), the reference's sdf.f(transform_point(sdf.frame, p)) (yocto_sdfs.cpp:21),
 *    f one of the six sd_* as yocto_sceneio.cpp:3684-3730 binds them (the table at vpt_sdf), with the reference's ternary abs / min / max
 *    (yocto_math.h:1354-1356) in the reference's term order.
 *  - Combination, a the resident value, b the brush distance, k = blend.  REPLACE: b.  With k == 0: UNION (a < b) ? a : b; SUBTRACT
 *    (-b > a) ? -b : a, the reference's op_subtraction(brush, resident) (yocto_sdfs.h:87); INTERSECT (a > b) ? a : b - selects, never
 *    fminf / fmaxf: a NaN resident value is replaced by UNION and INTERSECT and kept with its bits by SUBTRACT.  With k > 0 the polynomial
 *    smooth minimum  m = (x < y) ? x : y; d = x - y; ad = d < 0 ? -d : d; t = k - ad; h = (t > 0 ? t : 0) / k;
 *    smin = m - ((h * h) * k) * 0.25f:  UNION smin(a, b), SUBTRACT -smin(b, -a), INTERSECT -smin(-a, -b).  REPLACE ignores blend.
 *  - A stroke.  The stamps first_stamp .. first_stamp + num_stamps of an entry are applied to each voxel in list order,
 *    v = op_s(v, brush_s(sample)): a stroke of N stamps equals N one-stamp edits bit for bit.  Every voxel of the region evaluates every
 *    stamp.  Entries run in order, and a volume id may repeat: the launches are ordered on one stream.
 *  - Validation before anything is written (VPT_ERR_INVALID_ARG, the message names the entry or the stamp, the scene is untouched): the
 *    volume id in range; the region inside the resident whd; the stamp range inside the edit's list; type 0..5 and op 0..3; every float
 *    finite (frame, whd, p, origin, step, blend) and blend >= 0.  An entry whose region voxels x num_stamps exceeds 2^36 is refused with
 *    VPT_ERR_UNSUPPORTED (split the stroke): one launch on a shared GPU stays short.
 *  - An entry with an empty region or no stamps launches nothing.  vpt_scene_update_stats afterwards: launches = one per entry that is
 *    neither; bytes = VPT_SCULPT_RECORD_BYTES per stamp of the edit's list, uploaded in one copy when anything is launched (0 otherwise) -
 *    not one voxel.  An edit without entries starts the counters again at (0, 0).
 *  - Synchronisation, the VPT_ERR_HIP semantics and the forgetting of the launch-schedule record: those of vpt_scene_update. */
enum { VPT_SCULPT_REPLACE = 0, VPT_SCULPT_UNION = 1, VPT_SCULPT_SUBTRACT = 2, VPT_SCULPT_INTERSECT = 3 };
#define VPT_SCULPT_RECORD_BYTES 80   /* one stamp as the device reads it: frame, four parameters, type | op << 8, blend */
typedef struct vpt_sculpt_stamp { vpt_sdf brush; int32_t op; float blend; } vpt_sculpt_stamp;
typedef struct vpt_sculpt_entry {
  int32_t volume;
  int32_t region_lo[3], region_whd[3];  /* the box of voxels this entry changes */
  float   origin[3], step[3];           /* voxel (i, j, k) is sampled at origin + (i, j, k) * step */
  int32_t first_stamp, num_stamps;      /* its stroke inside edit->stamps */
} vpt_sculpt_entry;
typedef struct vpt_sculpt_edit {
  int32_t num_entries; const vpt_sculpt_entry* entries;
  int32_t num_stamps;  const vpt_sculpt_stamp* stamps;
} vpt_sculpt_edit;
int vpt_scene_sculpt_volumes(vpt_scene* scene, const vpt_sculpt_edit* edit);

/* ---- adding and removing volumes, grid instances and SDFs -------------------------------------------------------------
 * The one thing vpt_scene_update_volumes leaves fixed: how many there are.  An edit of its own, because vpt_volume_edit keeps its layout;
 * the contract is that of vpt_scene_update_instances and vpt_scene_update_shapes.  After vpt_scene_update_volume_set(s, edit) every table
 * on the device holds the bytes vpt_scene_create would hold for the descriptor built as follows (renders are bit-identical to a fresh
 * handle's, vpt_scene_light_tables_hash equals a fresh handle's on all six tables).
 *  - Lists.  The three old lists with the removed entries erased and the added ones appended in the order given: survivors keep their
 *    order and the ids close up (erase + push_back).  Removals are applied first, on current ids, then the adds.  There is no `set` list:
 *    vpt_scene_update_volumes edits entries, before or after this call, on the ids that hold then.
 *  - Renumbering.  A surviving grid instance's `volume` follows the new volume numbering.  An added instance names a volume of the NEW
 *    list, so it may name a volume added by the same edit.
 *  - Voxels.  A survivor keeps its voxels bit for bit.  A FROM_HOST volume holds voxels[offset .. offset + W*H*D) (whole grid, x fastest).
 *    A FROM_BAKE volume holds the bits of vpt_bake_sdf for its descriptor, written by the bake kernel straight into its new place (also
 *    under VPT_BAKE_BRUTE=1).  A FILL volume holds the bits of `fill` in every voxel (any float, a NaN's payload included).  A COPY volume
 *    holds what volume copy_of (a CURRENT id) held before the call; the source may be removed by the same edit.
 *  - Pool layout.  After an edit that adds or removes at least one volume the pool is exactly the volumes in id order with no gap between
 *    them: vpt_scene_get_volumes reports offsets equal to the running sum of W*H*D, and the room earlier regrowths of
 *    vpt_scene_update_volumes left unused is reclaimed.  The new pool is a fresh allocation filled by ONE launch, whatever the number of
 *    volumes (then one bake launch per FROM_BAKE entry).  An edit that touches no volume leaves the pool alone.
 *  - Records.  The evaluation records, inverse frames, bounding balls, the scene's ball and the plane count are prep_sdf_records' for all
 *    records, as after vpt_scene_update_volumes; the device tables are allocated at their new lengths.  No grid instance and no SDF at all
 *    is a valid scene (every `implicit` sample is a miss), and a scene created with none may gain its first.
 *  - Lights.  make_lights of the new scene under the rule of vpt_scene_update_lights: vpt_light::sdf follows the new SDF numbering, mesh
 *    and environment lights keep their CDFs, indices and guide tables (moved device to device).  With no change among the SDF lights
 *    (none added, none removed, none renumbered) nothing of the lights is touched.
 *  - The LDS budget of the implicit kernels' record copy is decided per launch: a scene that grew past it is refused at render time
 *    (VPT_ERR_UNSUPPORTED), exactly as a fresh handle of the same descriptor is.
 *  - volgrid.  The brick tables are indexed by volume: the next volgrid launch or query rebuilds them.
 *  - Validation before anything is written (VPT_ERR_INVALID_ARG, the message names the entry, the scene is untouched): null lists with
 *    non-zero counts, negative counts; ids out of range or repeated within a list; a removed volume that a surviving or added grid
 *    instance still names; `volume` or `material` out of range in the new numbering; floats that are not finite and `type` outside 0..5
 *    (the checks of vpt_scene_update_volumes); whd >= 0 with a product below 2^31, factor by factor; the pool's new total below 2^43
 *    voxels, the reach of the one gather launch (and below 2^62 before that, so that no sum overflows);
 *    offset + grid size inside `voxels`; an unknown source; copy_of out of range or a COPY whose whd differs from its source's; a bake
 *    descriptor vpt_bake_sdf would refuse or whose whd is not the entry's.  A bake tree deeper than the kernel's stack gives
 *    VPT_ERR_UNSUPPORTED, also before anything is written.
 *  - Everything is built into buffers of the call; pointers, counts and mirrors are swapped after the last check.  A device failure after
 *    validation (VPT_ERR_HIP) leaves the handle good for vpt_scene_destroy only.  An edit with all counts zero does nothing.
 *  - vpt_scene_update_stats afterwards: launches = 1 gather (when a volume is added or removed and the new pool is not empty) + 1 per
 *    non-empty bake + those of a light rebuild; bytes = 4 per voxel of the edit's payload (sent whole and once when a FROM_HOST entry names it: pack the grids tightly, as
 *    VolumeSetEdit does) + 32 per segment of the gather's table + the three small
 *    tables and the record tables at their new lengths (24 per volume, 60 + 112 per grid instance, 84 + 144 per SDF) + per bake its tree
 *    and triangle records + what a light rebuild sends.  Nothing is proportional to the voxels of a surviving, baked, filled or copied
 *    volume.
 *  - Synchronisation, the VPT_ERR_HIP semantics and the forgetting of the launch-schedule record: those of vpt_scene_update. */
enum { VPT_VOLUME_FROM_HOST = 0, VPT_VOLUME_FROM_BAKE = 1, VPT_VOLUME_FILL = 2, VPT_VOLUME_COPY = 3 };
typedef struct vpt_volume_new {
  int32_t whd[3]; float res;
  int32_t source;                     /* one of the four above */
  int64_t offset;                     /* FROM_HOST: first voxel inside edit->voxels (whole grid, x fastest) */
  const struct vpt_bake_desc* bake;   /* FROM_BAKE: bake->whd == whd, the rules of vpt_bake_sdf */
  float   fill;                       /* FILL: every voxel gets these bits */
  int32_t copy_of;                    /* COPY: a CURRENT volume id; whd must equal that volume's */
} vpt_volume_new;
typedef struct vpt_volume_set_edit {
  int32_t num_remove_vol_instances; const int32_t* remove_vol_instance_ids;       /* current ids */
  int32_t num_remove_sdfs;          const int32_t* remove_sdf_ids;                /* current ids */
  int32_t num_remove_volumes;       const int32_t* remove_volume_ids;             /* current ids */
  int32_t num_add_volumes;          const vpt_volume_new* add_volumes;            /* appended after the survivors */
  int32_t num_add_vol_instances;    const vpt_volume_instance* add_vol_instances; /* `volume` in the NEW numbering */
  int32_t num_add_sdfs;             const vpt_sdf* add_sdfs;
  int64_t num_voxels;               const float* voxels;                          /* the payload of the FROM_HOST entries */
} vpt_volume_set_edit;
int vpt_scene_update_volume_set(vpt_scene* scene, const vpt_volume_set_edit* edit);

/* ---- the volgrid shader: voxel grids as heterogeneous media (VPT_SHADER_VOLGRID) ------------------------------------
 * The reference has no such shader: the rule is this project's and is written here.  The parts that more than one side computes - clean,
 * the brick majorants, a grid instance's record, its density at a point - are csrc/vpt_volgrid_rule.h, compiled by the kernel (K3,
 * csrc/vpt_volgrid_kernel.hip.h) and by the host mirror (host/vpt_volgrid.cpp), both with -ffp-contract=off.
 *  - What it sees.  vol_instances as media, environments as background and light.  Mesh instances and analytic SDFs are ignored, as
 *    `implicit` ignores meshes: there are no surfaces inside the media.
 *  - Density of grid instance g at world point p.  pl = transform_point(instance.frame, p); bbox_size = volume.res * whd * scalef, as
 *    eval_sdf (yocto_sdfs.cpp:30-49) maps a point into a grid.  Outside [0, bbox_size] the density is 0.  Inside, v = eval_volume(volume,
 *    pl * 2 / bbox_size - 1), the reference's trilerp in its term order, and sigma = clean(v) / trdepth with clean(x) = x for a finite
 *    positive x, 0 otherwise (NaN, +-Inf, negative values, zero) and trdepth that of the instance's material: a voxel value of 1 is a
 *    mean free path of trdepth.  scalef scales the box, never the density.  A volgrid render (any entry point) of a scene where some grid
 *    instance's material has trdepth <= 0 or not finite is refused with VPT_ERR_INVALID_ARG, the message names the instance, scene and
 *    state stay untouched.
 *  - The medium, from the same material.  Single-scattering albedo = scattering clamped to [0, 1] per channel; phase function
 *    Henyey-Greenstein with g = scanisotropy (sample_phasefunction, eval_phasefunction: yocto_shading.h:1077-1102); emission is added at
 *    every real collision; the extinction is grey, colour comes from the albedo.
 *  - Majorants.  Per volume a table of brick maxima: brick (bx, by, bz) covers the cells [8 b, 8 b + 8) per axis of the W - 1 cells
 *    between the nodes, and its value is the maximum of clean(node) over the nodes [8 b, min(8 b + 8, W - 1)] per axis.  A trilerp inside
 *    the brick is a convex combination of those nodes up to rounding, so a tentative collision is real with probability
 *    min(sigma / majorant, 1).  The tables are built on the device, by the first volgrid launch or query of a handle, and again before a
 *    volgrid launch whenever the scene was edited since: a handle counts its edits, and those that write voxels (vpt_scene_update_volumes
 *    with its bakes and pool growth, vpt_scene_sculpt_volumes) apart.  No other shader pays for them.
 *  - Free flight of a ray (o, d): track.  The grid instances in index order; tmax = the nearest real collision so far, at first none.
 *    Instance g: the ray is clipped against its box in local space (slab test; the parameter t stays the world's) and against tmax; the
 *    bricks along it are walked in node coordinates.  A brick of majorant 0 is crossed without a draw.  In a brick of majorant m (as
 *    extinction: m / trdepth) repeat: t += -log(1 - rand1f(rng)) / m; past the brick's exit: on to the next brick from the exit point (the
 *    overshoot is discarded: the process has no memory); else rand1f(rng) < min(sigma(p) / m, 1) makes the collision real - tmax = t,
 *    instance g, on to instance g + 1 - else it is null and the walk goes on.  The nearest real collision over all instances wins:
 *    independent free flights per medium with the minimum taken are exact for a superposition of media, so instances may overlap and every
 *    collision has one material.  A free flight that has taken VPT_VOLGRID_MAX_STEPS (2^20) tracking steps ends its path with nothing more
 *    added and counts in the word vpt_check_watchdog reads.
 *  - The path (the volume branch of shade_volpathtrace, yocto_pathtrace.cpp:653-683):
 *      radiance = 0, weight = 1, hit = false
 *      for bounce in [0, bounces):
 *        ev = track(ray, rng);  escape: radiance += weight * eval_environment(ray.d), done
 *        if bounce == 0: hit = true
 *        radiance += weight * emission
 *        E = the light-list entries with environment >= 0, in list order
 *        if E is empty or noimplicit_mis:  incoming = sample_phasefunction(g, outgoing, rn), drawn as sample_scattering draws (rn.x,
 *            rn.y, then the rnl nobody reads); weight *= albedo - no division: f / pdf is 1 by construction
 *        else: rand1f < 0.5 ? the same draw : the environment branch of sample_lights for a uniformly chosen entry of E (ruv.x, ruv.y,
 *            rel, rl as sample_lights draws them); weight *= albedo * (f / (0.5 f + 0.5 pdf_E)), f = eval_phasefunction(g, outgoing,
 *            incoming), pdf_E = the environment branch of sample_lights_pdf summed over E, times 1 / |E|
 *        weight zero or not finite: done
 *        if bounce > 3: rr = min(1, max(weight)); if rr < 1 { rand1f >= rr: done; weight /= rr }
 *        ray = (position, incoming)
 *      return (radiance, hit ? 1 : 0)
 *    The roulette is NOT the reference's min(0.99, .): with 0.99 a white furnace is never exact; with min(1, .) a medium of albedo 1 keeps
 *    weight 1 for ever and `bounces` ends its paths.  The camera ray, the draws of a sample's jitter and lens, the preview branch of
 *    samples == 1, the NaN guard and the accumulation into the state are pathtrace_samples', as in every shader here: the alpha channel
 *    sums `hit`, hits[] counts the samples.
 * VPT_VOLGRID_NO_BRICKS=1 (read per launch) walks every box with one majorant, the maximum of its volume's bricks: the A/B switch of the
 * tests and the measurements - same distribution, other draws.
 *
 * vpt_scene_get_volgrid_majorants: the brick table of `volume` as the device holds it (built or rebuilt first if it is stale), x fastest;
 * dims (nullable) receives the bricks per axis, out (nullable with capacity 0: the dims alone) their product of floats.
 * vpt_scene_volgrid_density: at n world points (3 floats each) sigma[i] = the sum over the grid instances, in index order, of their
 * densities, and instance[i] (nullable) = the first instance whose box holds the point, -1 if none does.  Refused like a render when a
 * grid instance's material has no usable trdepth.
 * vpt_scene_volgrid_track: track(ray, rng) above on n given world rays (6 floats each: origin, unit direction) with n given PCG32 streams
 * (state, inc), one lane per record, through the device functions K3 itself calls, compiled in K3's unit: event[i] = 0 escape, 1
 * collision, 2 the flight ran into VPT_VOLGRID_MAX_STEPS; instance[i] and t[i] = the collision's grid instance and world parameter (-1 and
 * FLT_MAX unless event[i] == 1); steps[i] = the tracking steps taken; rng_out (nullable) = the streams after the flight.  Tables are
 * brought up to date as before a launch, VPT_VOLGRID_NO_BRICKS is honoured, the refusal of a medium without usable trdepth is a render's;
 * the steps word of vpt_scene_volgrid_stats does not count these flights.  VPT_ERR_INVALID_ARG before anything is launched: n < 0, a null
 * pointer other than rng_out when n > 0, a ray component that is not finite, a direction whose length is not within 1e-3 of 1.
 * vpt_scene_volgrid_stats: tracking steps taken by the handle's volgrid launches so far and the builds of its brick tables so far (either
 * nullable); synchronous. */
#define VPT_VOLGRID_MAX_STEPS (1 << 20)
int vpt_scene_get_volgrid_majorants(vpt_scene* scene, int volume, float* out, int64_t capacity, int32_t dims[3]);
int vpt_scene_volgrid_density(vpt_scene* scene, int n, const float* points, int32_t* instance, float* sigma);
int vpt_scene_volgrid_track(vpt_scene* scene, int n, const float* rays /* n x {o[3], d[3]} */, const uint64_t* rng_in /* n x {state, inc} */,
                            int32_t* event /* 0 escape, 1 collision, 2 step bound reached */, int32_t* instance /* -1 unless event == 1 */,
                            float* t /* flt_max unless event == 1 */, int32_t* steps, uint64_t* rng_out /* n x {state, inc}, nullable */);
int vpt_scene_volgrid_stats(vpt_scene* scene, uint64_t* steps, int32_t* table_builds);

/* ---- the BVHs of a resident scene built anew on the device ------------------------------------------------------------
 * The four edits above keep a tree's topology as creation left it: vpt_scene_update is the reference's update_bvh, a refit.  After a
 * real deformation, or after instances have been rearranged, boxes and renders stay correct but the tree no longer fits the geometry.
 * vpt_scene_rebuild_bvh is the reference's make_bvh (yocto_bvh.cpp:526-611) for a scene that lives on a GPU.
 * After the call every table on the device holds the bytes vpt_scene_create would upload for a descriptor that satisfies three
 * conditions:
 *  - The named shapes' shape_bvh_nodes / shape_bvh_prims are what the reference's make_bvh builds from the shape's current vertices
 *    on the device.  The element boxes are those of yocto_bvh.cpp:537-549 (point_bounds, line_bounds, triangle_bounds, quad_bounds,
 *    with the select-form min / max of vpt_scene_update).  The build is build_bvh(..., highquality = false): split_middle, at most
 *    four primitives per leaf, node ids in the reference's creation order, libstdc++'s std::partition - the rule of vpt_build_bvh.
 *  - The scene BVH is what make_bvh builds over transform_bbox(frame, shape root box) of the current instances, ALL of them, in
 *    instance order.  An instance of a shape without nodes gets invalidb3f, as in yocto_bvh.cpp:601-603.
 *  - The shape node pool and the quad-node pool are laid out contiguously in shape order, as the host's flatten lays them out.  The
 *    node counts change, so node_offset, num_nodes, the quad-node offset and the root reference of every later shape follow.
 * So renders, vpt_intersect, vpt_kat, vpt_scene_get_bvh and vpt_scene_light_tables_hash give the bits of a fresh handle made from
 * that descriptor.  Element counts stay: a shape has exactly as many leaf slots before and after; its records move to their new slots.
 *  - what->scene non-zero builds the scene BVH anew; it is forced when num_shapes > 0, as make_bvh would.  num_shapes == 0 and
 *    scene == 0 is valid and does nothing.
 *  - Refusals.  Validation comes first: a null argument, an id out of range or an id repeated gives VPT_ERR_INVALID_ARG.  The
 *    traversal limits vpt_scene_create decides are decided anew from the new trees, by the same function: the 256-entry LDS stack of
 *    the binary walk, the packed pop floor of the quad traversal, 2^27 quad nodes; a tree past them gives VPT_ERR_UNSUPPORTED.  A
 *    refused call leaves the scene exactly as it was: everything is built into new buffers, and pointers, counts and mirrors are
 *    swapped only after the last check.  A device failure after validation (VPT_ERR_HIP) leaves the handle good for
 *    vpt_scene_destroy only, as in vpt_scene_update.
 *  - The stack sizes of the handle follow the new trees: the HBM part of the traversal stacks may appear, grow or go.
 *    VPT_STACK_LDS and VPT_DEBUG are read as at creation.  The next vpt_scene_update makes its refit tables anew.
 *  - What crosses PCIe: down, the new node arrays (32 B per node of the shape pool and of the scene BVH) and primitive orders (4 B
 *    per element of a named shape and per instance); up, the tables that depend on topology alone, made on the host from that one
 *    read-back by the functions of vpt_scene_create (quad nodes, 128 B each; the integer words of the enter records, 96 B per
 *    instance; the slot of every instance; the shape records, 80 B each).  No vertex, leaf record or element box crosses.
 *    vpt_scene_update_stats reports the launches, the bytes of both directions in one sum, and the device time of the call.
 *  - Synchronisation and the forgetting of the launch-schedule record: those of vpt_scene_update. */
typedef struct vpt_bvh_rebuild {
  int32_t num_shapes; const int32_t* shape_ids;  /* shape BVHs to build anew; ids in range, none repeated */
  int32_t scene;                                 /* non-zero: build the scene BVH anew; forced when num_shapes > 0, as make_bvh would */
} vpt_bvh_rebuild;
int vpt_scene_rebuild_bvh(vpt_scene* scene, const vpt_bvh_rebuild* what);
/* vpt_scene_rebuild_bvh with the trees of the reference's high-quality build: `quality` is VPT_BVH_MIDDLE (vpt_scene_rebuild_bvh itself)
 * or VPT_BVH_SAH (the rule at vpt_build_bvh_quality, below).  The contract is the one above with highquality = quality: after the call
 * every table holds the bytes vpt_scene_create would upload for a descriptor whose named shapes' trees, and whose scene tree when it is
 * built, are build_bvh(..., highquality = quality).  Refusals, limits (creation's own function, on the new trees), the swap after the last
 * check and the PCIe accounting are those above; another quality gives VPT_ERR_INVALID_ARG before anything is built.
 * What follows from the other contracts: a refit (vpt_scene_update) keeps the topology, so SAH trees survive it; vpt_scene_update_instances
 * and a `set` in vpt_scene_update_shapes build with the middle split, as their rules say - the handle remembers no quality. */
int vpt_scene_rebuild_bvh_quality(vpt_scene* scene, const vpt_bvh_rebuild* what, int quality);
/* The node counts as the device holds them now: what vpt_scene_get_bvh's capacities must reach (for a handle that was never rebuilt,
 * the descriptor's counts).  shape_node_offsets: per shape, the first node of its BVH in the pool; may be NULL. */
int vpt_scene_get_bvh_counts(vpt_scene* scene, int32_t* scene_nodes, int64_t* shape_nodes, int64_t* shape_node_offsets /* per shape, may be NULL */);
/* The primitive orders as the device holds them now: the scene's (one entry per scene-BVH slot: num_instances after a rebuild) and the
 * shapes', pooled at each shape's element offset (the element id in every leaf slot).  Capacities in entries; a null array is skipped. */
int vpt_scene_get_bvh_prims(vpt_scene* scene, int32_t* scene_prims, int capacity, int32_t* shape_prims, int64_t shape_capacity);

/* ---- instances of a resident scene added, removed and re-pointed on the device ------------------------------------------
 * The edits above keep the set of instances as creation left it.  vpt_scene_update_instances changes it: the instance table changes
 * length and numbering, and everything keyed by an instance id follows.  Shapes, elements, materials, textures, volumes and SDFs stay.
 * After the call every table on the device holds the bytes vpt_scene_create would upload for a descriptor that satisfies three
 * conditions:
 *  - Instances.  The old list with the `set` entries replaced (frame, shape and material), the removed entries erased and the added
 *    ones appended in the order given.  Survivors keep their relative order and the ids close up, exactly as
 *    scene.instances.erase + push_back would leave the reference's scene_data.
 *  - Scene BVH.  What make_bvh (build_bvh, highquality = false; the rule of vpt_build_bvh) builds over transform_bbox(frame, shape root
 *    box) of ALL instances of the new list, in the new id order.  The shape root boxes are the ones the device holds now - they may
 *    have been refitted or rebuilt - and the shape BVHs are not touched.  An instance of a shape without nodes gets invalidb3f.
 *  - Lights.  make_lights of the new scene under the rule of vpt_scene_update_lights: emissive instances of faces in the new id order,
 *    then the environments' and the SDFs' lights, which keep their entries, CDFs and records byte for byte.
 * So renders, vpt_intersect (scene and single-instance query), vpt_kat, vpt_scene_get_bvh*, vpt_scene_light_tables_hash and
 * vpt_scene_instance_tables_hash give the bits of a fresh handle made from that descriptor.
 *  - Order of application.  `set` first (on current ids), then `remove` (current ids), then `add`.  An edit with all three counts zero
 *    is valid and does nothing: no launch, no bytes.
 *  - Validation before anything is written (VPT_ERR_INVALID_ARG, scene untouched): a null list with a non-zero count or a negative
 *    count; an id out of range or repeated within its list; an id both set and removed; a shape or material out of range; a frame
 *    value that is not finite; the material rule of vpt_scene_create - a material that becomes bound to a mesh instance for the first
 *    time has its texture ids range-checked, as creation checks the materials of instances.  Zero instances after the edit is valid,
 *    as it is for vpt_scene_create: the scene BVH has no nodes and no primitives.
 *  - Refusals after building (VPT_ERR_UNSUPPORTED, scene untouched).  The traversal limits vpt_scene_create decides are decided anew
 *    for the new scene BVH together with the shapes' trees, by the same function: the 256-entry LDS stack of the binary walk, the
 *    packed pop floor of the quad traversal, 2^27 quad nodes.  Everything is built into buffers of the call; pointers, counts and
 *    mirrors are swapped only after the last check.  A device failure after validation (VPT_ERR_HIP) leaves the handle good for
 *    vpt_scene_destroy only.
 *  - Lights under renumbering.  A surviving emissive instance keeps its CDF, its search index (offsets rebased) and its guide table,
 *    all moved device to device; a CDF is computed only for an instance that is new, newly emissive, or whose shape changed through
 *    `set`.  vpt_light::instance, the light records and light_prims are made anew for the new numbering.
 *  - The kernel instances follow the new scene: whether an instanced shape holds points or lines, whether media vary over a surface,
 *    the light features.  The stack sizes follow the new scene BVH as after vpt_scene_rebuild_bvh.  The next vpt_scene_update makes
 *    its refit tables anew.
 *  - What crosses PCIe.  Down, in one copy: 4 B per removed id and per set id (each of the two lists padded to 16 B) and 128 B per set
 *    or added instance (the record creation would upload, its inverse made on the host); then the tables that depend on the scene BVH's topology, made on the host by the functions of
 *    vpt_scene_create: the scene's quad nodes (128 B each), the integer words of the enter records (96 B per instance), the slot of
 *    every instance (4 B); when the lights change, a few words per light (32 B list entry, 56 B index header, 4 B tag, 24 B job
 *    descriptor of a recomputed one).  Up: the scene BVH's nodes (32 B each) and primitive order (4 B per instance), and 8 B per
 *    recomputed light.  Nothing proportional to vertices, elements, leaf records, texels, voxels or CDF entries crosses, and no node
 *    or quad node of a shape does: the shapes' part of the quad-node table moves device to device.
 *    vpt_scene_update_stats reports the launches, the bytes of both directions in one sum, and the device time of the call.
 *  - Synchronisation and the forgetting of the launch-schedule record: those of vpt_scene_update. */
typedef struct vpt_instance_edit {
  int32_t num_remove; const int32_t* remove_ids;                     /* current ids, none repeated */
  int32_t num_set;    const int32_t* set_ids; const vpt_instance* set; /* current ids, none repeated, none also removed: frame, shape and material replaced */
  int32_t num_add;    const vpt_instance* add;                       /* appended after the survivors, in this order */
} vpt_instance_edit;
int vpt_scene_update_instances(vpt_scene* scene, const vpt_instance_edit* edit);
/* forward frame, shape, material of every instance as the device holds them; capacity in entries; `out` may be NULL (the count only) */
int vpt_scene_get_instances(vpt_scene* scene, vpt_instance* out, int capacity, int* num_instances);
/* FNV-1a over four tables read back from the device: the instance records (128 B each), scene_enter, slot_of_instance, scene_prims */
int vpt_scene_instance_tables_hash(vpt_scene* scene, uint64_t out[4]);

/* ---- shapes of a resident scene added, removed and replaced on the device -----------------------------------------------
 * The edits above keep the meshes as creation left them: how many vertices and elements a shape has, and of what kind.
 * vpt_scene_update_shapes changes the shape list: the per-shape pools change length and layout, and what is keyed by a shape id or by an
 * offset into a pool follows.  Materials, textures, volumes and SDFs stay, and so does the number of instances.
 * After the call every table on the device holds the bytes vpt_scene_create would upload for a descriptor built as follows:
 *  - Shape list.  The old list with the `set` entries replaced, the removed entries erased and the added ones appended.  Survivors keep
 *    their order and the ids close up.  `set` is applied first, on current ids, then `remove` (current ids), then `add`, as for
 *    vpt_scene_update_instances.
 *  - Renumbered instances.  Every instance's `shape` follows the renumbering; its shape_flags are those of the shape it names now.
 *  - Pools.  Vertex, element, node, quad-node and leaf pools are contiguous in shape order, as the host mirror's flatten lays them out.
 *    A scene whose pools are not (a descriptor made by other means) is refused with VPT_ERR_UNSUPPORTED before anything is built.
 *  - BVHs of `set` and added shapes.  What make_bvh builds from their elements: the boxes of yocto_bvh.cpp:537-549 (point_bounds,
 *    line_bounds, triangle_bounds, quad_bounds), build_bvh with highquality = false.
 *  - BVHs of untouched shapes.  The trees the device holds now, refitted or rebuilt ones included.
 *  - Scene BVH.  Built anew over all instances when, and only when, num_set > 0: a replaced shape has another root box.  Otherwise
 *    the nodes and the primitive order stay, and only the integer words of the enter records follow the new offsets.
 *  - Lights.  make_lights of the new scene under the rule of vpt_scene_update_lights.  A mesh light on a `set` shape gets a CDF of the
 *    new length and the kind (single leaf of at most four elements, or tree) of its new BVH; every other light keeps its CDF.
 * So renders, both forms of vpt_intersect, vpt_kat, vpt_scene_get_bvh*, vpt_scene_light_tables_hash, vpt_scene_instance_tables_hash
 * and vpt_scene_shape_tables_hash give the bits of a fresh handle made from that descriptor.
 *  - An edit with all three counts zero is valid and does nothing: no launch, no bytes.
 *  - One shape (vpt_shape_data).  Indices are local to the shape, as in the descriptor.  Exactly one kind of element, or none: triangles,
 *    quads, points or lines.  normals, texcoords and colors are NULL or hold num_vertices entries; radius is required with points or lines
 *    and ignored otherwise.
 *  - Validation before anything is written (VPT_ERR_INVALID_ARG, scene untouched): a null list with a non-zero count or a negative
 *    count; an id out of range or repeated within its list; an id both set and removed; a vertex index out of range; both triangles and
 *    quads; points or lines without radius; a float that is not finite; a removed shape that an instance still names (the caller removes
 *    or re-points its instances through vpt_scene_update_instances first); a pool whose new entry count does not fit the 32-bit offsets
 *    of the shape records.  A shape that mixes points, lines and faces is refused with VPT_ERR_UNSUPPORTED, as by vpt_scene_create.
 *  - Refusals after building (VPT_ERR_UNSUPPORTED, scene untouched).  The traversal limits of vpt_scene_create are decided anew by the
 *    same function from the new shapes' trees, what the handle keeps of the untouched ones (depth and quad-stack need per shape) and
 *    the scene BVH: removing the deepest shape lowers the stack sizes as a fresh creation would.  Everything is built into buffers of the
 *    call; pointers, counts and mirrors are swapped only after the last check.  A device failure after validation (VPT_ERR_HIP)
 *    leaves the handle good for vpt_scene_destroy only.
 *  - Compact triangle records (vpt_scene_record_bytes) exist while every shape holds triangles and VPT_NO_COMPACT_TRIANGLES is unset:
 *    they are dropped when a shape of another kind (or an empty one) enters and made on the device from the general records when the
 *    last such shape leaves or becomes triangles.  The kernel instances follow the new scene: points or lines among the instanced
 *    shapes, media that vary over a surface (a replaced shape may gain or lose vertex colours), the light features.  The next
 *    vpt_scene_update makes its refit tables anew.
 *  - What crosses PCIe.  Down: the payload of the `set` and added shapes in one copy, every array padded to 16 B - 12 B per position
 *    and per normal, 8 B per texcoord, 16 B per colour, 4 B per radius, 12 / 16 / 4 / 8 B per triangle / quad / point / line; 128 B per
 *    quad node of a `set` or added shape; 80 B per shape of the new list, a second time when the scene BVH is built (the instance boxes
 *    need the root boxes before the quad nodes are numbered); 8 B per shape of the old list (new id and flags); 96 + 4 B per
 *    instance (the integer words of the enter records, the slots); 128 B per quad node of the scene BVH when it is built; the lights'
 *    words of vpt_scene_update_instances.  Up: 32 B per node and 4 B per element of `set` and added shapes; 32 B per scene node and 4 B
 *    per instance when the scene BVH is built; 8 B per recomputed light.  Nothing is proportional to vertices, elements, nodes, quad
 *    nodes or leaf records of an untouched shape - they move device to device, one copy per pool and run of adjacent survivors - nor
 *    to texels, voxels or CDF entries of an untouched light.  vpt_scene_update_stats reports launches, bytes and device time.
 *  - Synchronisation and the forgetting of the launch-schedule record: those of vpt_scene_update. */
typedef struct vpt_shape_data {          /* one shape, indices shape-local, as in the descriptor */
  int32_t num_vertices;
  const float* positions;                /* float3, required when num_vertices > 0 */
  const float* normals;                  /* float3 or NULL */
  const float* texcoords;                /* float2 or NULL */
  const float* colors;                   /* float4 or NULL */
  const float* radius;                   /* float or NULL; required with points or lines */
  int32_t num_triangles; const int32_t* triangles;   /* int3 */
  int32_t num_quads;     const int32_t* quads;       /* int4 */
  int32_t num_points;    const int32_t* points;      /* int  */
  int32_t num_lines;     const int32_t* lines;       /* int2 */
} vpt_shape_data;
typedef struct vpt_shape_edit {
  int32_t num_remove; const int32_t* remove_ids;                          /* current ids, none repeated, none named by an instance */
  int32_t num_set;    const int32_t* set_ids; const vpt_shape_data* set;  /* current ids, none repeated, none also removed: the whole mesh replaced */
  int32_t num_add;    const vpt_shape_data* add;                          /* appended after the survivors, in this order */
} vpt_shape_edit;
int vpt_scene_update_shapes(vpt_scene* scene, const vpt_shape_edit* edit);
/* FNV-1a over eight groups of tables read back from the device: the shape records (80 B each); positions, normals, texcoords and
 * colors in one chain; elems; leaf_prims (with its 8 trailing float4); leaf_attrs; tri_prims then tri_attrs in one chain (0 where the
 * scene has none); shape_nodes; the shapes' quad nodes */
int vpt_scene_shape_tables_hash(vpt_scene* scene, uint64_t out[8]);
/* the number of shapes and the entries of the pooled element and vertex tables as the device holds them; any pointer may be NULL */
int vpt_scene_get_shape_counts(vpt_scene* scene, int32_t* num_shapes, int64_t* num_elements, int64_t* num_vertices);

/* ---- subdivision surfaces of a resident scene: re-tesselated on the device ---------------------------------------
 * The last member of the reference's scene_data that was frozen at load time: `subdivs`.  A subdivision surface is edited through a
 * cage of tens of vertices and a displacement amount; tesselate_surface (yocto_pathtrace.cpp:1230-1273) turns them into the vertices
 * of its shape.  The integer half of that work (catmullclark topology, split_facevarying, the per-vertex face lists) is done once on the
 * host and attached to the scene as a PLAN; afterwards only the cage's floats move, and the float half runs on the device into the
 * resident vertex pools, followed by the refit of vpt_scene_update and, for a shape a light uses, the rebuild of vpt_scene_update_lights.
 *
 * The plan (vpt_subdiv_plan; libvpt_host.so makes it: vpth_scene_subdiv_plan_item).  Every index in it is checked on the host at attach:
 *  - settings: the shape id, subdivisions, smooth, displacement, displacement_tex (-1: none);
 *  - cage floats: positions (float3) and - read only when subdivisions == 0 - the cage's own normals (float3, or none).  The cage's
 *    texcoords are not part of it: the shape's texcoords do not depend on positions or displacement, they stay as they are resident;
 *  - levels: one vpt_subdiv_level (dim 3) per subdivision, level k + 1 taking the refined vertices of level k;
 *  - quads: the cage's quadspos after the last level (int4; the cage's own for subdivisions == 0), read by quads_normals when the
 *    subdiv is smooth and subdivisions > 0;
 *  - verts: split_facevarying's table, int3 per shape vertex {position, normal or -1, texcoord or -1} - indices into the refined
 *    positions, and into the normals: quads_normals' (one per refined position) for a smooth subdiv with subdivisions > 0, the cage's
 *    for subdivisions == 0;
 *  - triangles_normals reads the shape's triangles where they are resident (the element table); its per-vertex face lists are built by
 *    the library at attach, from one read-back of the shape's elements, whenever displacement_tex >= 0.
 * vpt_scene_attach_subdiv validates the plan (VPT_ERR_INVALID_ARG, scene untouched: a null array with a count, a negative count, a
 * level whose num_vertices is not the refined count of the one before, any index out of range, a float that is not finite) and checks
 * it against the resident shape: it holds triangles, num_vertices is its vertex count, the number of triangles quads_to_triangles makes
 * of `quads` (two per quad, one where z == w) is its element count, normals are present exactly when the plan's settings produce them
 * (below), texcoords exactly when verts[].z >= 0, displacement_tex names a texture of the scene, and no other plan names the shape.
 * Then it uploads the tables in ONE allocation with the plan's scratch (vpt_scene_update_stats: the bytes sent, no launch; the
 * allocation's size is what the plan holds in HBM - DESIGN.md §25 has the formula).  It renders nothing and changes no table of the
 * scene.  *subdiv_id_out names the plan from then on.  vpt_scene_detach_subdiv frees it; ids of other plans stay.
 * vpt_scene_subdiv_count: the plans attached.  vpt_scene_subdiv_shape: the shape a plan edits now, -1 for an id that is not attached.
 *
 * The edit (vpt_subdiv_edit): per named plan a new cage (num_cage_positions float3) or NULL to keep the one the device holds, and a
 * displacement amount or NaN to keep it (displacement NULL keeps all).  An entry that keeps both is valid: it tesselates again from
 * what the device holds NOW, the displacement texture's texels included - how a vpt_scene_update_textures reaches the mesh.
 * Contract: after the call every table on the device holds the bytes it would hold after the host mirror's tesselate_surface on the
 * edited subdiv, vpt_scene_update with that shape's shape_positions / shape_normals, and vpt_scene_update_lights when a light's
 * instance uses the shape.  The topology stays; renders, vpt_intersect, vpt_kat, vpt_scene_get_bvh, vpt_scene_shape_tables_hash and
 * vpt_scene_light_tables_hash give that path's bits.  (The one difference: the parent's path refuses a tesselated vertex that is not
 * finite - 0 / 0 for a cage vertex no face names; here only the cage's floats are checked, and such a vertex is written as it is.)
 * On the device, per named plan, stream 0:
 *  1. the levels through the points and averaging kernels of vpt_subdivide_vertices; consecutive levels that refine to at most 256
 *     vertices run in one launch of one workgroup (same device functions, __syncthreads() between passes and levels); VPT_UPDATE_NO_FUSE
 *     in the environment, read per call, gives every level its two launches - same bits;
 *  2. quads_normals when smooth and subdivisions > 0;
 *  3. the gather through `verts`, one thread per shape vertex: positions and normals as float3 into the plan's staging buffers;
 *  4. when displacement != 0 and displacement_tex >= 0: triangles_normals if the shape has no normals so far, the displacement through
 *     the scene's OWN tables (the shape's resident texcoords, the resident texture record and texels), triangles_normals again when smooth;
 *  5. vpt_scene_update's scatter, leaf records, refit and everything behind it, reading the staging buffers where it reads the
 *     uploaded payload otherwise; then vpt_scene_update_lights' rebuild when a light's instance uses one of the shapes.
 * Which pools a shape has follows the settings: normals are present when smooth, for subdivisions > 0; for subdivisions == 0 they are
 * the cage's own (present when it has some) while not displaced, and present when smooth while displaced.
 * Refusals, scene untouched.  VPT_ERR_INVALID_ARG (the message names the entry): a null list with a count, a negative count, an id out
 * of range, repeated or not attached, a float that is not finite (NaN in `displacement` means keep).  VPT_ERR_UNSUPPORTED: a
 * displacement switched between zero and non-zero on a plan with subdivisions == 0 whose cage has normals while it is not smooth (or
 * has none while it is smooth): the shape would gain or lose its normals - that edit is vpt_scene_update_shapes'; and a displaced plan
 * whose shape has no texcoords.  There is no field for subdivisions, smooth, the cage's topology or texcoords: they change counts or
 * pools.  Device failures, synchronisation and the launch-schedule record: as vpt_scene_update.
 * Living with the other edits.  A plan stores the shape id only and reads pool offsets, the texture record and the shape's elements'
 * place at edit time.  vpt_scene_update_shapes: a `set` or removed shape drops its plan (its id then answers "not attached"); the
 * plans of the survivors follow the renumbering.  vpt_scene_rebuild_bvh leaves plans alone (the element table keeps its order; the
 * refit tables are made anew).  vpt_scene_update: a plain vertex edit of a subdiv's shape is allowed; the next subdiv edit overwrites
 * it.  vpt_scene_update_textures: a later subdiv edit reads the new texels, also after the pool has grown and moved.
 * What crosses PCIe per edit: 12 B per cage vertex of an entry with a new cage, and what vpt_scene_update itself sends for an edit
 * without vertices - nothing else; the constant per named plan is 0 B (settings and table addresses travel as kernel arguments).
 * vpt_scene_update_stats reports launches, bytes and device time of the whole call, refit and light rebuild included. */
typedef struct vpt_subdiv_level vpt_subdiv_level;   /* below, with vpt_subdivide_vertices */
typedef struct vpt_subdiv_plan {
  int32_t shape, subdivisions, smooth;
  float   displacement;
  int32_t displacement_tex;                                       /* -1: none */
  int32_t num_cage_positions; const float* cage_positions;        /* float3 */
  int32_t num_cage_normals;   const float* cage_normals;          /* float3; 0 / NULL: the cage has none */
  int32_t num_levels;         const vpt_subdiv_level* levels;     /* == subdivisions */
  int32_t num_quads;          const int32_t* quads;               /* int4: quadspos after the last level */
  int32_t num_vertices;       const int32_t* verts;               /* int3 per shape vertex: position, normal or -1, texcoord or -1 */
} vpt_subdiv_plan;
int vpt_scene_attach_subdiv(vpt_scene* scene, const vpt_subdiv_plan* plan, int* subdiv_id_out);
int vpt_scene_detach_subdiv(vpt_scene* scene, int subdiv_id);
int vpt_scene_subdiv_count(const vpt_scene* scene);
int vpt_scene_subdiv_shape(const vpt_scene* scene, int subdiv_id);
typedef struct vpt_subdiv_edit {
  int32_t num; const int32_t* subdiv_ids;
  const float* const* cage_positions;   /* per entry: the cage's float3 array, or NULL (keep); the list itself may be NULL (keep all) */
  const float* displacement;            /* per entry; the array may be NULL (keep all); NaN = keep one    */
} vpt_subdiv_edit;
int vpt_scene_update_subdivs(vpt_scene* scene, const vpt_subdiv_edit* edit);

/* ---- the drop-in for pathtrace_samples() --------------------------------------------
 * Host, row-major (idx = j*width + i) caller-owned state, exactly pathtrace_state
 * (yocto_pathtrace.h:57-64): image float4[w*h], hits int32[w*h], rng {u64 state, u64 inc}[w*h].
 * Renders min(nsamples, params->samples - *samples_io) passes; the result equals that many
 * consecutive reference calls.  *samples_io is state.samples (in/out).                    */
int vpt_render(vpt_scene* scene, const vpt_params* params, int nsamples, int width, int height,
               float* image_rgba, int32_t* hits, uint64_t* rng, int* samples_io);

/* ---- the same over several GPUs of this process ("multi-GPU fan-out is internal", §8(e)) ----------
 * One host thread per GPU; the frame's 8x8-pixel tiles are dealt round-robin (tile t -> devices[t % ndev]); every
 * device holds the whole scene and the state of its own tiles, so rendering needs no communication and the result is
 * bit-identical to vpt_render's (pixels own their RNG streams).
 *
 * Residency: the tile state (radiance sums, hit counts, PCG32 streams) STAYS ON THE DEVICES between calls
 * (the reference's pathtrace_state is the same progressive accumulator, yocto_pathtrace.h:57-64).
 *   vpt_multi_set_state   host pathtrace_state -> devices (pinned staging, one thread per GPU)
 *   vpt_multi_render      with null image/hits/rng: `nsamples` passes on the resident state, nothing is transferred;
 *                         with host pointers: the contract of vpt_render - the arrays ARE the state: they are read on
 *                         every call and current after it (yocto_pathtrace.cpp:1081-1090).  RULE: a device's part of
 *                         the upload is skipped only if the device provably holds it - the three arrays are the very
 *                         ones (same addresses, size, *samples_io > 0) the previous call on this handle downloaded
 *                         into, and a 64-bit checksum over every word of that part (taken after the download, re-taken
 *                         from the arrays now) is unchanged.  An in-place edit of any pixel, another state object, a
 *                         fresh make_state: uploaded, nothing to announce.  vpt_multi_uploaded_parts() tells what
 *                         the last call did.
 *   vpt_multi_get_state   devices -> host arrays, on demand
 *   vpt_multi_get_render  get_render of the resident state, assembled on devices[0]: the float4 tile buffers travel there
 *                         over xGMI by grouped RCCL send / receive (RCCL is bound on first use, a copy the process already
 *                         carries is reused; one device never touches it unless VPT_MULTI_FORCE_RCCL=1, which sends the
 *                         buffer to itself through a one-rank communicator) or, where RCCL cannot be had, by
 *                         hipMemcpyPeerAsync; then the kernel of vpt_resolve_device.
 * Like vpt_render, a render fails with VPT_ERR_HIP if a wave of the implicit kernel gave up on its watchdog. */
typedef struct vpt_multi vpt_multi;
int  vpt_multi_create(const vpt_scene_desc* desc, const int* devices, int ndev, vpt_multi** out);
int  vpt_multi_create_curves(const vpt_scene_desc* desc, const vpt_scene_curves* curves, const int* devices, int ndev, vpt_multi** out);
void vpt_multi_destroy(vpt_multi* m);
/* vpt_scene_update with the same edit on every device of `m`, one after the other; an edit the first device refuses has changed
 * none.  The resident tile state is left as it is. */
int  vpt_multi_update(vpt_multi* m, const vpt_scene_edit* edit);
/* vpt_scene_update_lights in the same way */
int  vpt_multi_update_lights(vpt_multi* m, const vpt_scene_edit* edit);
/* vpt_scene_update_textures in the same way */
int  vpt_multi_update_textures(vpt_multi* m, const vpt_texture_edit* edit);
/* vpt_scene_update_volumes in the same way (a bake entry is prepared and baked once per device) */
int  vpt_multi_update_volumes(vpt_multi* m, const vpt_volume_edit* edit);
/* vpt_scene_sculpt_volumes in the same way: the same stamps run on every device */
int  vpt_multi_sculpt_volumes(vpt_multi* m, const vpt_sculpt_edit* edit);
/* vpt_scene_update_volume_set in the same way (a FROM_BAKE entry is prepared and baked once per device) */
int  vpt_multi_update_volume_set(vpt_multi* m, const vpt_volume_set_edit* edit);
/* vpt_scene_rebuild_bvh in the same way: every device builds its own trees; the arrays are equal by construction */
int  vpt_multi_rebuild_bvh(vpt_multi* m, const vpt_bvh_rebuild* what);
int  vpt_multi_rebuild_bvh_quality(vpt_multi* m, const vpt_bvh_rebuild* what, int quality);   /* vpt_scene_rebuild_bvh_quality on every device */
/* vpt_scene_update_instances in the same way: every device renumbers and builds its own tables; they are equal by construction */
int  vpt_multi_update_instances(vpt_multi* m, const vpt_instance_edit* edit);
/* vpt_scene_update_shapes in the same way: every device lays out its own pools and builds its own trees; they are equal by construction */
int  vpt_multi_update_shapes(vpt_multi* m, const vpt_shape_edit* edit);
/* vpt_scene_attach_subdiv / _detach_subdiv / _update_subdivs in the same way: every device holds its own copy of a plan under the same
 * id (the devices take the same calls in the same order, so their ids agree; VPT_ERR_HIP if they ever do not) */
int  vpt_multi_attach_subdiv(vpt_multi* m, const vpt_subdiv_plan* plan, int* subdiv_id_out);
int  vpt_multi_detach_subdiv(vpt_multi* m, int subdiv_id);
int  vpt_multi_subdiv_shape(const vpt_multi* m, int subdiv_id);   /* of devices[0] */
int  vpt_multi_update_subdivs(vpt_multi* m, const vpt_subdiv_edit* edit);
int  vpt_multi_device_count(const vpt_multi* m);
/* how vpt_multi_get_render moves the parts: "rccl", "peer-copy" (several devices, no RCCL) or "local" (one device) */
const char* vpt_multi_transport(const vpt_multi* m);
int  vpt_multi_set_state(vpt_multi* m, int width, int height, const float* image_rgba, const int32_t* hits,
                         const uint64_t* rng, int samples);
int  vpt_multi_get_state(vpt_multi* m, float* image_rgba, int32_t* hits, uint64_t* rng, int* samples);
/* pathtrace_samples over all GPUs of `m` (see above for null host pointers) */
int  vpt_multi_render(vpt_multi* m, const vpt_params* params, int nsamples, int width, int height,
                      float* image_rgba, int32_t* hits, uint64_t* rng, int* samples_io);
/* get_render (yocto_pathtrace.cpp:1105-1116) of the resident state: row-major float4 image * (1 / samples) into the
 * caller's host buffer, gathered and resolved on devices[0] */
int  vpt_multi_get_render(vpt_multi* m, float* image_rgba);
/* how many devices' parts the last vpt_multi_render call with host pointers uploaded (0 ... device count) */
int  vpt_multi_uploaded_parts(const vpt_multi* m);

/* ---- device-resident state (bench / multi-GPU; buffers owned by the caller, e.g. torch) */
/* number of state slots a rank needs for `layout` (multiple of tile_w*tile_h) */
int64_t vpt_layout_slots(const vpt_layout* layout);
/* host row-major <-> device tile-major (only this rank's pixels are touched) */
int vpt_state_upload(const vpt_layout* layout, const float* image_rgba, const int32_t* hits,
                     const uint64_t* rng, void* d_image, void* d_hits, void* d_rng, void* stream);
int vpt_state_download(const vpt_layout* layout, const void* d_image, const void* d_hits,
                       const void* d_rng, float* image_rgba, int32_t* hits, uint64_t* rng,
                       void* stream);
/* nsamples passes over this rank's pixels; asynchronous on `stream` (hipStream_t) - with one exception per layout: the call
 * that takes the tile-splitting decision (below: the second full call on a layout that is short of waves) waits for the previous
 * launch and reads its per-tile costs back (a few tens of ms at 3840x1600) before it enqueues.  params->samples == 1
 * selects the pixel-centre preview branch (yocto_pathtrace.cpp:1059-1068).
 * Scheduling: a wave renders all samples of its 64 pixels, so the scene handle remembers how long every
 * wave of the last launch took and starts the next launch on the same layout / camera / shader longest wave
 * first.  Without such a record and with nsamples >= 16, the first nsamples/64 (1..16) samples are rendered by a separate pilot
 * launch that takes the measurement.  Neither changes the result  (pixels are independent, batching is exact). */
int vpt_render_device(vpt_scene* scene, const vpt_params* params, const vpt_layout* layout,
                      int nsamples, void* d_image, void* d_hits, void* d_rng, void* stream);
/* get_render (yocto_pathtrace.cpp:1105-1116) on device: gathered tile-major float4 sums of ALL
 * ranks ([nranks][slots]) -> row-major float4 image * (1/samples).                          */
int vpt_resolve_device(const vpt_layout* layout, const void* d_tiles_all_ranks, int samples,
                       void* d_image_rowmajor, void* stream);

/* the same followed by the 8-bit output stage of save_image (rgb_to_srgb + float_to_byte, yocto_color.h:207-231;
 * yocto_sceneio.cpp:509-571 then hands the bytes to the encoder): row-major RGBA8 on the device, 4 B per pixel
 * to download for a preview instead of 16.  Uses the device's powf: a byte may differ by one from the host
 * routine where the curve lands within an ulp of a quantisation step (parity checks use the host routine). */
int vpt_resolve_srgb8_device(const vpt_layout* layout, const void* d_tiles_all_ranks, int samples,
                             void* d_rgba8_rowmajor, void* stream);

/* ---- first-hit AOVs in one pass: denoising guides, depth, ids ------------------------------------------
 * The three debug shaders draw no random number after the camera ray (yocto_pathtrace.cpp:893-930), so from equal hits / rng they
 * trace the same rays.  vpt_render_aov_device traces each of them once: per sample and slot -> pixel (px, py) it draws u, v and the
 * lens sample exactly as vpt_render_device does (the pixel-centre branch of params->samples == 1 draws no jitter), evaluates
 * eval_camera, runs ONE intersect_bvh(bvh, scene, ray) and gives every plane that is not null this sample's value:
 *   normal, albedo, texcoord  float4 per slot, sums: what `normal`, `color`, `texcoord` add to `image` (alpha 1); {0,0,0,0} on a miss
 *   depth                     float4 per slot, sums: {distance, 0, 0, 1} on a hit, {0,0,0,0} on a miss
 *   ids, uvt                  int32 x2 and float x3 per slot, vpt_intersect's format: {instance, element} and {u, v, distance},
 *                             {-1, -1} and zeros on a miss.  Written only by the sample that finds hits[slot] == 0 - the state's
 *                             first sample; later samples leave them alone, so they do not depend on how a render is batched.
 * A sample's value that is not finite counts as zeros, decided per plane as for `image` (cpp:1087-1089).  Shapes of points or lines
 * give the values the debug shaders give on them.  hits and rng advance exactly as under a debug shader.  The planes are tile-major in
 * the layout's slots like `image` (the float planes resolve through vpt_resolve_device, ids / uvt through vpt_resolve_ids_device);
 * padding slots and other ranks' slots are never touched.
 * Contract: from equal hits / rng a plane has the bits of `image` after vpt_render_device with the matching debug shader, hits and rng
 * are equal afterwards, and any batching of nsamples gives the same bits in every plane.  With params->samples == 1, ids / uvt are
 * those of vpt_intersect on the pixel-centre rays.  The pass reports what intersect_bvh sees: no SDF, no voxel grid
 * (those: vpt_render_sdf_aov_device, below).
 * vpt_render_aov_device: asynchronous on `stream`, one plain launch (no schedule, no pilot, no tile splitting); it allocates nothing
 * beyond what vpt_render_device would; nsamples == 0 is a no-op; params->shader is ignored.  VPT_ERR_INVALID_ARG when every plane is
 * null or uvt is given without ids.  The planes must be distinct buffers that do not overlap each other, hits or rng: each is updated
 * on its own (two planes at one address are refused; a partial overlap is the caller's to avoid).
 * vpt_resolve_ids_device: the gathered ids / uvt of ALL ranks ([nranks][slots]) -> row-major; d_uvt and d_uvt_rowmajor null together.
 * vpt_render_aov: the same on host arrays - `planes` holds HOST pointers to row-major planes (in and out: the float planes are sums),
 * hits / rng are those of a row-major pathtrace_state (in and out); min(nsamples, params->samples - *samples_io) samples, a no-op at
 * the cap.  Synchronous; buffers owned by the call.  Arguments are checked before a device is looked for, the scene last
 * (VPT_ERR_INVALID_ARG, the message names the argument). */
typedef struct vpt_aov_planes {
  void* normal;     /* float4 per slot (pixel), or NULL */
  void* albedo;
  void* texcoord;
  void* depth;
  void* ids;        /* int32 x2 */
  void* uvt;        /* float x3; needs ids */
} vpt_aov_planes;
int vpt_render_aov_device(vpt_scene* scene, const vpt_params* params, const vpt_layout* layout, int nsamples,
                          const vpt_aov_planes* planes, void* d_hits, void* d_rng, void* stream);
int vpt_resolve_ids_device(const vpt_layout* layout, const void* d_ids, const void* d_uvt, void* d_ids_rowmajor,
                           void* d_uvt_rowmajor, void* stream);
int vpt_render_aov(vpt_scene* scene, const vpt_params* params, int nsamples, int width, int height,
                   const vpt_aov_planes* planes, int32_t* hits, uint64_t* rng, int* samples_io);

/* ---- first-hit AOVs of the implicit shaders: one sphere-traced pass -------------------------------------------
 * The implicit counterpart of the pass above: what the SDF side of a scene - voxel-grid instances and analytic SDFs - shows under a
 * pixel.  shade_implicit_normal draws no random number after the camera ray (yocto_pathtrace.cpp:538-562), so per sample and slot ->
 * pixel (px, py) vpt_render_sdf_aov_device draws u, v and the lens sample exactly as vpt_render_device does (the pixel-centre branch
 * of params->samples == 1 draws no jitter), evaluates eval_camera, runs ONE spheretrace(scene, ray, params->spheretrace_maxiter)
 * (cpp:289-307, the march of the implicit kernels step for step) and gives every plane that is not null this sample's value:
 *   normal   float4 per slot, sums: {normal * 0.5 + 0.5, 1} on a hit - what `implicit_normal` adds to `image` -, {0,0,0,0} on a miss;
 *            the normal is eval_sdf_normal of the hit's grid instance or analytic SDF at (position, t), position = o + d * t
 *   albedo   float4 per slot, sums: {color of the hit's material (vol_instances[i].material / sdfs[j].material, no texture), 1} on a
 *            hit, {0,0,0,0} on a miss
 *   depth    float4 per slot, sums: {t, 0, 0, 1} on a hit, {0,0,0,0} on a miss
 *   ids      int32 x2 per slot: {vol_instance, sdf}, spheretrace_result's pair - exactly one of them >= 0 on a hit, {-1, -1} on a miss
 *   hit      float4 per slot: {position.xyz, t} of the same hit, zeros on a miss.  ids / hit are written only by the sample that
 *            finds hits[slot] == 0 - the state's first sample; later samples leave them alone, so they do not depend on batching.
 * A FIRST hit is reported whatever the opacity of its material: `implicit` may step through a surface of opacity < 1 with a random
 * draw, this pass draws nothing after the camera ray and reports the surface it meets first.  A sample's value that is not finite
 * counts as zeros, decided per plane as for `image` (cpp:1087-1089).  hits and rng advance exactly as under `implicit_normal`.  The
 * planes are tile-major in the layout's slots like `image` (the float planes resolve through vpt_resolve_device, ids / hit through
 * vpt_resolve_sdf_ids_device); padding slots and other ranks' slots are never touched.  A scene with no grid instance and no SDF is
 * not an error: every sample is a miss.
 * Contract: from equal hits / rng, `normal` has the bits of `image` after vpt_render_device with `implicit_normal`, hits and rng are
 * equal afterwards, and any batching of nsamples gives the same bits in every plane.  With params->samples == 1, ids and hit.w are
 * vpt_spheretrace's {instance, sdf} and t on the pixel-centre rays.
 * vpt_render_sdf_aov_device: asynchronous on `stream`, one plain launch (no schedule, no pilot, no tile splitting, no watchdog: a
 * launch ends after at most nsamples x (spheretrace_maxiter + 1) rounds of the march); it allocates nothing; nsamples == 0 is a
 * no-op; params->shader is ignored.  VPT_ERR_INVALID_ARG (the message names the argument) when every plane is null, hit is given
 * without ids, two planes share a buffer, hits / rng / params / layout is null, or params->spheretrace_maxiter is outside
 * [0, 1 << 20] (the range vpt_kat accepts); VPT_ERR_UNSUPPORTED when the scene's SDF records exceed the 64 KiB the implicit kernels
 * copy to LDS.  The planes must not overlap each other, hits or rng (a partial overlap is the caller's to avoid).
 * vpt_resolve_sdf_ids_device: the gathered ids / hit of ALL ranks ([nranks][slots]) -> row-major; d_hit and d_hit_rowmajor null together.
 * vpt_render_sdf_aov: the same on host arrays, with vpt_render_aov's contract - `planes` holds HOST pointers to row-major planes (in
 * and out: the float planes are sums), hits / rng are those of a row-major pathtrace_state; min(nsamples, params->samples -
 * *samples_io) samples, a no-op at the cap.  Synchronous; buffers owned by the call.  Arguments are checked before a device is
 * looked for, the scene last. */
typedef struct vpt_sdf_aov_planes {
  void* normal;     /* float4 per slot (pixel), or NULL */
  void* albedo;
  void* depth;
  void* ids;        /* int32 x2 */
  void* hit;        /* float4; needs ids */
} vpt_sdf_aov_planes;
int vpt_render_sdf_aov_device(vpt_scene* scene, const vpt_params* params, const vpt_layout* layout, int nsamples,
                              const vpt_sdf_aov_planes* planes, void* d_hits, void* d_rng, void* stream);
int vpt_resolve_sdf_ids_device(const vpt_layout* layout, const void* d_ids, const void* d_hit, void* d_ids_rowmajor,
                               void* d_hit_rowmajor, void* stream);
int vpt_render_sdf_aov(vpt_scene* scene, const vpt_params* params, int nsamples, int width, int height,
                       const vpt_sdf_aov_planes* planes, int32_t* hits, uint64_t* rng, int* samples_io);

/* ---- adaptive sampling: every pixel renders until its noise meets a target ---------------------------
 * A pixel that stops after k samples holds exactly the state k consecutive reference calls leave (image, rng, hits == k):
 * pixels are independent and batching is exact, so the numerical contract holds per pixel.  Rendering goes in rounds; each
 * round renders min(step, params->samples - hits) samples for every pixel still rendering (the same count for all of them:
 * hits[] is uniform on entry and they have rendered every round).  The pixels left are packed 64 to a wave, in tile-major order.
 * The rule, after round n (n = 1, 2, ...) of m samples, for each pixel p still rendering:
 *   L = (image.x + image.y + image.z) / 3               (the pixel's radiance sum, float32, in that order)
 *   b = (L - lum_prev) / m, then lum_prev = L          (lum_prev starts as L of the entry state)
 *   Welford over the rounds' means:  delta = b - mean;  mean += delta / n;  m2 += delta * (b - mean)   (mean, m2 start at 0)
 *   p stops when hits[p] >= params->samples (the per-pixel cap), or when
 *     threshold > 0  and  n >= 2  and  hits[p] >= min_samples  and  m2 / (n * (n - 1)) <= (threshold * max(mean, 1/256))^2
 *   i.e. the standard error of the pixel's mean luminance is within `threshold` of that mean, with a floor for dark pixels.
 * Every value is float32 (n and n - 1 converted to float before their product); threshold == 0 never stops a pixel early. */
typedef struct vpt_adaptive {
  float   threshold;    /* relative standard error at which a pixel stops (rule above); 0: never stops early */
  int32_t min_samples;  /* no pixel stops early with fewer hits; 1 <= min_samples <= params->samples        */
  int32_t step;         /* samples per round for every pixel still rendering (>= 1)                         */
} vpt_adaptive;
/* Host pathtrace_state, like vpt_render; params->samples is the per-pixel cap; all hits[] must be equal on entry
 * (VPT_ERR_INVALID_ARG otherwise); *samples_io becomes max(hits); *rendered (nullable) the samples actually taken.
 * Like vpt_render it fails with VPT_ERR_HIP if a wave of the implicit kernel gave up on its watchdog. */
int vpt_render_adaptive(vpt_scene* scene, const vpt_params* params, const vpt_adaptive* adaptive, int width, int height,
                        float* image_rgba, int32_t* hits, uint64_t* rng, int* samples_io, int64_t* rendered);
/* The same on device-resident tile-major state of one rank (vpt_layout), asynchronous on `stream` apart from one small
 * read-back per round (the count of pixels still rendering, which sizes the next launch and ends the loop at 0) and the
 * watchdog check after each round of the implicit kernels.  hits[] must be equal over the rank's pixels on entry (checked on
 * the device before anything renders: VPT_ERR_INVALID_ARG).  *rounds, *rendered (both nullable): rounds run, samples taken.
 * The rounds bypass the launch schedule of vpt_render_device (no pilot, no longest-first order, no tile splitting, no wave
 * costs recorded): the handle's record for the layout is left as it was.  vpt_last_kernel_ms covers the whole call. */
int vpt_render_device_adaptive(vpt_scene* scene, const vpt_params* params, const vpt_adaptive* adaptive, const vpt_layout* layout,
                               void* d_image, void* d_hits, void* d_rng, void* stream, int* rounds, int64_t* rendered);
/* The same loop as an object, so that it can stop after any round and go on in a later call.
 * vpt_render_device_adaptive is create + rounds(INT_MAX) + destroy.
 *  create   the checks of vpt_render_device_adaptive and its round 0: statistics initialised, min / max of hits[] read back,
 *           unequal hits refused (VPT_ERR_INVALID_ARG, no run is made).  The run keeps the pointers, the stream, copies of params
 *           and adaptive, and its own scratch, sized for the full layout.
 *  rounds   up to max_rounds more rounds of min(step, params->samples - hits) samples, each followed by the 16-byte read-back (and
 *           the watchdog check for the implicit kernels), exactly the rounds the one-call form runs.  *rounds_done, *rendered: of this
 *           call; *active: pixels still rendering afterwards (all three nullable).  It returns at once, with 0 rounds and nothing
 *           enqueued, when no pixel is active or the cap is reached.  The schedule record is left alone.  vpt_last_kernel_ms covers
 *           create and the rounds of the first call that runs any; after a later call, that call's rounds.
 *  progress rounds, samples and active pixels so far, and the hit count of the pixels that rendered every round (each nullable).
 *  noise_device / stats_device   the run's tile-major statistics as row-major width x height planes of this rank's pixels (others
 *           are left as they are), asynchronous on `stream`, which must be ordered after the run's own.  The rule, for the pixel p
 *           of every slot that owns one, with step = adaptive->step and m2, mean the Welford values of the rule above:
 *             n_p     = (hits[p] + step - 1) / step        (integer: the rounds p rendered; it presumes the run began at hits 0)
 *             se2[p]  = m2 / ((float)n_p * (float)(n_p - 1))   if n_p >= 2, else 0      (float32; the left side of the stop rule)
 *             hits_out[p] = hits[p]                       (d_hits_rowmajor, nullable)
 *           stats_device writes mean and m2 themselves.  A pixel that stopped keeps the statistics of its last round.
 *  destroy  waits for the run's stream and frees the scratch; the state buffers are the caller's.
 * A run is tied to its scene handle as the handle was when the run was created: ANY edit or rebuild of the scene
 * (vpt_scene_update*, vpt_scene_rebuild_bvh*) ends the run's validity - destroy it before the edit and create another after. */
typedef struct vpt_adaptive_run vpt_adaptive_run;
int  vpt_adaptive_run_create(vpt_scene* scene, const vpt_params* params, const vpt_adaptive* adaptive, const vpt_layout* layout,
                             void* d_image, void* d_hits, void* d_rng, void* stream, vpt_adaptive_run** out);
int  vpt_adaptive_run_rounds(vpt_adaptive_run* run, int max_rounds, int* rounds_done, int64_t* rendered, int* active);
int  vpt_adaptive_run_progress(const vpt_adaptive_run* run, int* rounds, int64_t* rendered, int* active, int* max_hits);
int  vpt_adaptive_run_noise_device(vpt_adaptive_run* run, void* d_se2_rowmajor, void* d_hits_rowmajor, void* stream);
int  vpt_adaptive_run_stats_device(vpt_adaptive_run* run, void* d_mean_rowmajor, void* d_m2_rowmajor, void* stream);
void vpt_adaptive_run_destroy(vpt_adaptive_run* run);
/* box3 of a row-major float plane, the rule stated with the denoiser below: out[p] = (sum of in over the 3x3 taps of p inside the
 * image, dy outer -1..1, dx inner -1..1, starting at 0) / (their count, summed as float 1s).  Asynchronous on `stream`; out may
 * not alias in.  The variance a session hands to its filter in adaptive mode is vpt_box3_device(se2). */
int  vpt_box3_device(int width, int height, const void* d_in, void* d_out, void* stream);
/* get_render with each pixel's own sample count: gathered tile-major float4 sums and int32 hit counts of ALL ranks
 * ([nranks][slots] each) -> row-major image[p] * (1.0f / hits[p]), 0 where hits[p] == 0.  With uniform hits it gives the
 * bits of vpt_resolve_device (the same multiplication by the same reciprocal). */
int vpt_resolve_hits_device(const vpt_layout* layout, const void* d_tiles_all_ranks, const void* d_hits_all_ranks,
                            void* d_image_rowmajor, void* stream);

/* ---- denoising: an edge-avoiding à-trous wavelet filter guided by first-hit renders ----------------------
 * The body of the reference's denoise_render(denoised, render, albedo, normal) (yocto_trace.h:176-190), which without
 * OpenImageDenoise copies its input: here the spatial filter of SVGF (Dammertz et al. 2010, Schied et al. 2017).  It reads
 * resolved row-major images and writes another; no pathtrace_state is touched.  All images are row-major width x height:
 *   color     float4, a resolved render (get_render, get_render_hits, vpt_resolve_device, vpt_resolve_hits_device, ...)
 *   normal    float4, nullable: a resolved render of the `normal` (`implicit_normal`) shader; w is the coverage
 *   albedo    float4, nullable: a resolved render of the `color` shader
 *   variance  float,  nullable: an estimate of the variance of each pixel's mean luminance
 * The rule.  Every value is float32, every operation one of + - * / sqrt abs max, taken in the order written, none fused, and no
 * libm function: the host mirror (host/vpt_denoise.cpp), a numpy replay (tests/test_denoise_host.py) and the kernels give the
 * same bits.
 *   lum(c)   = ((c.x + c.y) + c.z) / 3
 *   d2(a, b) = (((a.x-b.x)^2 + (a.y-b.y)^2) + (a.z-b.z)^2) + (a.w-b.w)^2
 *   h[-2..2] = 1/16, 1/4, 3/8, 1/4, 1/16
 *   box3(f)[p] = (sum of f over the 3x3 taps of p inside the image, dy outer -1..1, dx inner -1..1, starting at 0) / (their
 *                count, summed as float 1s)
 *   v_0 = variance if given, else max(0, box3(lum * lum) - box3(lum) * box3(lum)) of color   (the spatial seed)
 *   c_0 = color
 *   rn = 1 / (sigma_normal * sigma_normal);  ra = 1 / (sigma_albedo * sigma_albedo)
 *   pass k = 0 .. iterations-1, stride s = 2^k, for every pixel p:
 *     r = 1 / (sigma_luminance * sqrt(v_k[p]) + 1e-4)
 *     taps q = p + s * (dx, dy), dy outer -2..2, dx inner -2..2; a tap outside the image is skipped
 *       x = abs(lum(c_k[p]) - lum(c_k[q])) * r
 *       x = x + d2(normal[p], normal[q]) * rn     if normal is given
 *       x = x + d2(albedo[p], albedo[q]) * ra     if albedo is given
 *       u = max(1 - x / 4, 0);  w = (h[dy] * h[dx]) * ((u * u) * (u * u))
 *       W = W + w;  C = C + w * c_k[q] (x, y, z each);  V = V + (w * w) * v_k[q]       (W, C, V start at 0)
 *     c_{k+1}[p].xyz = C / W;  c_{k+1}[p].w = c_k[p].w;  v_{k+1}[p] = V / (W * W)     (W >= 9/64: the centre tap has x = 0)
 *   out = c_iterations                                                                 (so out.w == color.w)
 * (The three quotients of a tap are products with reciprocals taken once per pixel or per call: a pass is bound by arithmetic, not by
 * memory, and a correctly rounded float32 division costs about ten instructions - DESIGN.md §11 has the times of both.)
 * ((u*u)*(u*u) stands where a Gaussian filter has exp(-x): it is 0 from x = 4 on, so a tap across an edge of the guides adds
 * exactly nothing.)  The half variance, from two points of one sample chain - S_a the radiance sums after the first a samples, S_n
 * after all n, 0 < a < n; samples a+1..n are independent of 1..a, so it costs no extra sample:
 *   A = S_a / a;  B = (S_n - S_a) / (n - a)   (x, y, z each; a, n - a as float);  g = (lum(A) - lum(B)) / 2;  variance = box3(g * g)
 * Defaults: iterations 5, sigma_luminance 4, sigma_normal 0.35, sigma_albedo 0.1. */
typedef struct vpt_denoise_params {
  int32_t iterations;        /* passes, 1..8; pass k has stride 2^k                         */
  float   sigma_luminance;   /* each finite and > 0                                         */
  float   sigma_normal;
  float   sigma_albedo;
} vpt_denoise_params;
#define VPT_DENOISE_DEFAULT_ITERATIONS 5
#define VPT_DENOISE_DEFAULT_SIGMA_LUMINANCE 4.0f
#define VPT_DENOISE_DEFAULT_SIGMA_NORMAL 0.35f
#define VPT_DENOISE_DEFAULT_SIGMA_ALBEDO 0.1f
/* bytes of the scratch buffer one vpt_denoise_device call needs (two colour and two variance images); -1 for a bad size */
int64_t vpt_denoise_scratch_bytes(int width, int height);
/* Device pointers, asynchronous on `stream`: no allocation, read-back or synchronisation inside.  d_out (float4 image) and
 * d_scratch may alias neither an input nor each other (VPT_ERR_INVALID_ARG); the inputs are left unchanged.  Passes of stride 1
 * and 2 take their taps from a tile staged in LDS, larger strides from global memory (csrc/vpt_denoise.hip): same bits;
 * VPT_DENOISE_PLAIN=1 in the environment, read per call, keeps every pass on the global-memory form. */
int vpt_denoise_device(const vpt_denoise_params* params, int width, int height, const void* d_color, const void* d_normal,
                       const void* d_albedo, const void* d_variance, void* d_out, void* d_scratch, void* stream);
/* the half variance above on two row-major float4 sum images, asynchronous on `stream` */
int vpt_half_variance_device(int width, int height, const void* d_sum_a, int a, const void* d_sum_n, int n, void* d_variance,
                             void* stream);
/* The same two on host arrays: synchronous, on GPU `device`, buffers owned by the call.  Arguments are checked before a
 * device is looked for (VPT_ERR_INVALID_ARG, the message names the argument); then VPT_ERR_NO_DEVICE without a GPU or for a
 * negative `device`. */
int vpt_denoise(const vpt_denoise_params* params, int device, int width, int height, const float* color, const float* normal,
                const float* albedo, const float* variance, float* out);
int vpt_half_variance(int device, int width, int height, const float* sum_a, int a, const float* sum_n, int n, float* variance);

/* ---- progressive rendering: a session whose state, image and display stay on one GPU -----------------------
 * The headless body of the reference's run_interactive (apps/ypathtrace/ypathtrace.cpp:90-304): reset_display (:144-194), the
 * worker's frame loop (:180-193) and the edits (:253-266, :292-296), without a window.  Three device stages, then the session.
 *
 * vpt_state_init_device: make_state (yocto_pathtrace.cpp:960-980) into this rank's tile-major slots.  The rule, for the pixel with
 * row-major index idx = j * width + i:
 *   g   = make_rng(1301081) advanced by idx steps            (the master stream in front of the pixel's draw)
 *   r   = the PCG32 output of g's state                      (what the (idx + 1)-th _advance_rng returns)
 *   rng = make_rng(961748941, (r % 2^31) / 2 + 1);  image = 0;  hits = 0
 * PCG32's state update is an LCG, so "advanced by idx steps" is the jump state' = A^idx state + inc (A^idx - 1) / (A - 1) mod 2^64
 * (csrc/vpt_rng_jump.h: square-and-multiply, at most 64 rounds): a wave takes one jump to the first pixel of its 8x8 block and every
 * lane one step of the LCG (A^k, c_k), k = row * width + column inside the block, from a 64-entry table the host makes per call.
 * Integers only: the bits of the host's make_state followed by vpt_state_upload.  Padding slots and the slots of other ranks are
 * left as they are, as vpt_state_upload leaves them.  Asynchronous on `stream`; no allocation.
 *
 * vpt_tonemap_device: tonemap(vec4f, exposure, filmic, srgb) of yocto_color.h:306-316 over a row-major float4 image, into a float4
 * display image, an RGBA8 image (float_to_byte, :207-211, of all four channels) or both (either pointer may be null, not both).
 * The rule, per pixel c, every value float32, every operation in the order written, none fused:
 *   e = exp2f(exposure), taken once per call on the host     (the reference takes the same value per pixel)
 *   if exposure != 0:  c.xyz = c.xyz * e
 *   if filmic:         h = c * 0.6f;  ldr = ((h * h) * 2.51f + h * 0.03f) / (((h * h) * 2.43f + h * 0.59f) + 0.14f);
 *                      c = (0 < ldr) ? ldr : 0              (x, y, z each; the reference's max in select form: a NaN becomes 0)
 *   if srgb:           c = (c <= 0.0031308f) ? 12.92f * c : (1 + 0.055f) * powf(c, 1 / 2.4f) - 0.055f     (rgb_to_srgb, :228-231)
 *   c.w passes through;  byte = clamp(int(c * 256), 0, 255)
 * Without srgb the stage holds no libm call and gives the bits of the host mirror (tonemap_image of host/vpt_host.h) and of the
 * reference; with srgb the device's powf stands where they have glibc's, as in vpt_resolve_srgb8_device, whose routine this is:
 * a byte may differ by one count (DESIGN.md §13 has the measured distances).  Values whose int(a * 256) is undefined in the
 * reference (not finite, outside int) give what that routine gives.  The accurate-fit branch of tonemap_filmic, which no caller of
 * the reference reaches, is not restated.
 *
 * vpt_upscale_device: the preview replicated to full size (ypathtrace.cpp:164-169):
 *   out[j * width + i] = preview[min(j / pratio, ph - 1) * pw + min(i / pratio, pw - 1)] */
typedef struct vpt_display_params {
  float   exposure;   /* finite                                       */
  int32_t filmic;     /* 0 / 1                                        */
  int32_t srgb;       /* 0 / 1; the reference's displays use 1        */
} vpt_display_params;
int vpt_state_init_device(const vpt_layout* layout, void* d_image, void* d_hits, void* d_rng, void* stream);
int vpt_tonemap_device(const vpt_display_params* display, int width, int height, const void* d_linear, void* d_display_f,
                       void* d_rgba8, void* stream);
int vpt_upscale_device(int pratio, int pw, int ph, const void* d_preview, int width, int height, void* d_out, void* stream);
/* vpt_tonemap_device on host arrays: synchronous, on GPU `device`, buffers owned by the call.  Arguments are checked before a device
 * is looked for (VPT_ERR_INVALID_ARG, the message names the argument); then VPT_ERR_NO_DEVICE without a GPU or for a negative `device`. */
int vpt_tonemap(const vpt_display_params* display, int device, int width, int height, const float* linear, float* display_f,
                uint8_t* rgba8);
/* the resident camera `camera` of a scene (after the edits it has taken) and the device it lives on */
int vpt_scene_get_camera(vpt_scene* scene, int camera, vpt_camera* out);
int vpt_scene_get_device(const vpt_scene* scene);

/* A session belongs to one vpt_scene and so to one device.  It owns the tile-major pathtrace_state of a one-rank 8x8 layout, the
 * preview's state, the row-major linear `image`, the float4 and RGBA8 `display`, a stream, and - with denoise = 1 - the guides,
 * the variance, the filtered image and the filter's scratch.  Nothing of these crosses PCIe unless a read-out call asks for it.
 * NOT thread-safe; while a session lives, calls on its scene handle must not overlap with calls on the session.
 *  vpt_session_create   width / height by make_state's rule from the resident camera (yocto_pathtrace.cpp:964-970); refuses pratio
 *                       outside 1..64 (the reference's slider) and resolution / pratio < 1 (VPT_ERR_INVALID_ARG), a bad shader
 *                       (VPT_ERR_UNKNOWN_SHADER).  The session starts as after vpt_session_reset.
 *  vpt_session_reset    reset_display: the state initialised on the device; the preview - a fresh state of resolution / pratio,
 *                       samples = 1 (the pixel-centre branch), through vpt_render_device, resolved and replicated into `image`;
 *                       `display` = tone map of `image`; samples = 0.  With non-null params it adopts them first, and allocates
 *                       again if the size changes.  With denoise = 1 it also renders the guides: guide_samples passes of `normal`
 *                       and `color` (`implicit_normal` and no albedo for the implicit shaders, as pathtrace_guides chooses) over
 *                       states initialised on the device, resolved with vpt_resolve_device (the mesh shaders' two guides come from
 *                       one first-hit pass with those bits: below).
 *  vpt_session_advance  min(nsamples, render.samples - samples) passes on the resident state, get_render into `image`, the filter
 *                       if denoise = 1, the tone map into `display`; a no-op at the cap.  For the implicit shaders it waits for
 *                       the passes and returns VPT_ERR_HIP when the watchdog fired, as vpt_render does; else it is asynchronous on
 *                       the session's stream and the read-out calls wait.
 *  vpt_session_set_display  tone-maps the image held (the filtered one where the display shows it) with the new parameters
 *                       (ypathtrace.cpp:259-266): nothing renders, state and samples stay.
 *  vpt_session_edit     vpt_scene_update, then a reset (:292-296); an edit that vpt_scene_update refuses leaves the session as it was.
 *  read-out             get_display (either pointer nullable: 4 or 16 B per pixel), get_image (the unfiltered linear image),
 *                       get_denoised (the filtered one; VPT_ERR_INVALID_ARG unless denoise = 1 and an advance has run since the last
 *                       reset), get_state (the pathtrace_state, row-major), size, samples.
 *  vpt_session_stats    what the last call on the session cost: kernel launches it enqueued itself (the render and filter entry points
 *                       it calls count one each), bytes it sent to the device (kernel arguments apart) and bytes it fetched.
 * Contract: after a reset and advances of k samples in total, get_state returns the bits of make_state + vpt_render(k), in any
 * batching; after a reset alone, `image` has the bits of the upscale of get_render of a vpt_render preview; `display` is the tone
 * map of `image`, or with denoise = 1 after an advance of the filtered image: display = tonemap(denoise(image, normal, albedo,
 * variance)).  The preview frame is never filtered.
 * Variance rule (denoise = 1): a starts at 0 at a reset.  At the start of an advance that begins at s > 0 samples, if s >= 2 a, the
 * radiance sums are copied (S_a) and a = s.  After the advance, at n > a samples: variance = vpt_half_variance_device(S_a, a, S_n, n)
 * if a > 0, else the filter's spatial seed.  The filter, the half variance and the guides are bit-exact, so the filtered image has
 * the bits of the host pipeline on the same inputs (pathtrace_guides, half_variance, denoise_render). */
typedef struct vpt_session_params {
  vpt_params         render;
  int32_t            pratio;          /* preview ratio, 1..64 (pathtrace_params::pratio, default 8)   */
  vpt_display_params display;
  int32_t            denoise;         /* 0 / 1: the display shows the filtered image                  */
  vpt_denoise_params filter;          /* read when denoise = 1                                        */
  int32_t            guide_samples;   /* >= 1 when denoise = 1                                        */
} vpt_session_params;
typedef struct vpt_session vpt_session;
int  vpt_session_create(vpt_scene* scene, const vpt_session_params* params, vpt_session** out);
void vpt_session_destroy(vpt_session* session);
int  vpt_session_reset(vpt_session* session, const vpt_session_params* params_or_null);
int  vpt_session_advance(vpt_session* session, int nsamples);
int  vpt_session_set_display(vpt_session* session, const vpt_display_params* display);
int  vpt_session_edit(vpt_session* session, const vpt_scene_edit* edit);
/* the same through vpt_scene_update_lights: an edit that switches a light on or off, or moves an emitter's vertices */
int  vpt_session_edit_lights(vpt_session* session, const vpt_scene_edit* edit);
/* vpt_scene_update_textures, then a reset; a refused edit leaves the session as it was */
int  vpt_session_edit_textures(vpt_session* session, const vpt_texture_edit* edit);
/* vpt_scene_update_volumes, then a reset; a refused edit leaves the session as it was */
int  vpt_session_edit_volumes(vpt_session* session, const vpt_volume_edit* edit);
/* vpt_scene_sculpt_volumes, then a reset; a refused edit leaves the session as it was */
int  vpt_session_sculpt_volumes(vpt_session* session, const vpt_sculpt_edit* edit);
/* vpt_scene_update_volume_set, then a reset (which drops both id frames: pick_sdf never names an entry that is gone); a refused edit
 * leaves the session as it was */
int  vpt_session_edit_volume_set(vpt_session* session, const vpt_volume_set_edit* edit);
/* vpt_scene_rebuild_bvh, then a reset (the picture is the same, its accumulation restarts as after the session's other edits); a refused call leaves the session as it was */
int  vpt_session_rebuild_bvh(vpt_session* session, const vpt_bvh_rebuild* what);
int  vpt_session_rebuild_bvh_quality(vpt_session* session, const vpt_bvh_rebuild* what, int quality);   /* vpt_scene_rebuild_bvh_quality, then a reset */
/* vpt_scene_update_instances, then a reset; a refused edit leaves the session as it was */
int  vpt_session_edit_instances(vpt_session* session, const vpt_instance_edit* edit);
/* vpt_scene_update_shapes, then a reset; a refused edit leaves the session as it was */
int  vpt_session_edit_shapes(vpt_session* session, const vpt_shape_edit* edit);
/* vpt_scene_update_subdivs, then a reset; a refused edit leaves the session as it was (plans are attached on the session's scene handle) */
int  vpt_session_edit_subdivs(vpt_session* session, const vpt_subdiv_edit* edit);
int  vpt_session_get_display(vpt_session* session, uint8_t* rgba8, float* display_f);
int  vpt_session_get_image(vpt_session* session, float* linear);
int  vpt_session_get_denoised(vpt_session* session, float* linear);
int  vpt_session_get_state(vpt_session* session, float* image_rgba, int32_t* hits, uint64_t* rng, int* samples);
int  vpt_session_size(const vpt_session* session, int* width, int* height);
int  vpt_session_samples(const vpt_session* session);
int  vpt_session_stats(const vpt_session* session, int* launches, int64_t* bytes_to_device, int64_t* bytes_to_host);
/* ---- what is under a pixel, and the guides -----------------------------------------------------------------
 * With denoise = 1 and a mesh shader, a reset renders both guides in ONE first-hit pass (vpt_render_aov_device: normal + albedo over a
 * state initialised on the device) and resolves each: the bits of the two separate renders, half their traversals.
 *   get_guides   the row-major guides, float4 per pixel, either pointer nullable, not both; VPT_ERR_INVALID_ARG unless denoise = 1
 *                (and for `albedo` under an implicit shader, which has none).
 * The id frame: {instance, element} and {u, v, distance} of every pixel, vpt_intersect's format and bits on the rays through the pixel
 * centres at full resolution - one sample of vpt_render_aov_device with samples = 1 over hits / rng of its own, initialised on the
 * device.  It is made by the first pick or get_ids after a reset (3 launches, buffers allocated then; the scene's instance table is
 * read with it, vpt_scene_get_instances, and counted in that call's bytes_to_host) and kept until the next reset.  Every edit resets,
 * so it never names what the scene no longer holds.
 *   pick         the hit under pixel (x, y): one launch that packs {hit, instance, element, u, v, distance} and one copy of those 24
 *                bytes; shape and material are those of vpt_scene_get_instances()[instance] (-1 on a miss, like instance and
 *                element).  x / y outside the frame: VPT_ERR_INVALID_ARG.
 *   get_ids      the whole frame, row-major: ids int32 x2 and uvt float x3 per pixel, either pointer nullable, not both.
 * pick and get_ids return VPT_ERR_UNSUPPORTED when the session's shader is implicit or implicit_normal: what the user sees there
 * is not what the mesh BVH holds (vpt_session_pick_sdf / vpt_session_get_sdf_ids, below, serve those sessions). */
typedef struct vpt_pick {
  int32_t hit;                  /* 0 / 1 */
  int32_t instance, element;
  int32_t shape, material;
  float   u, v, distance;
} vpt_pick;
int  vpt_session_get_guides(vpt_session* session, float* normal, float* albedo);
int  vpt_session_pick(vpt_session* session, int x, int y, vpt_pick* out);
int  vpt_session_get_ids(vpt_session* session, int32_t* ids, float* uvt);
/* ---- what is under a pixel of an implicit session ---------------------------------------------------------------
 * The counterpart of pick / get_ids for a session whose shader is implicit or implicit_normal.  The id frame: {vol_instance, sdf}
 * and {position, t} of every pixel, vpt_spheretrace's ids and t on the rays through the pixel centres at full resolution - one
 * sample of vpt_render_sdf_aov_device with samples = 1 over hits / rng of its own, initialised on the device, then
 * vpt_resolve_sdf_ids_device.  It is made by the first pick_sdf or get_sdf_ids after a reset (3 launches, buffers sized by the
 * layout's slots and allocated then) and kept until the next reset.  Every edit resets, so it never names a grid instance or an SDF
 * the scene no longer holds.
 *   pick_sdf     the hit under pixel (x, y): one launch that packs the 48 bytes below and one copy of them.  volume and material
 *                are those of the resident vol_instances[vol_instance] or sdfs[sdf] (volume -1 for an analytic SDF); normal is
 *                eval_sdf_normal of that record at (position, distance): the bits VPT_KAT_SDF_NORMAL gives.  On a miss hit = 0,
 *                the four ids are -1 and the floats 0.  x / y outside the frame: VPT_ERR_INVALID_ARG.
 *   get_sdf_ids  the whole frame, row-major: ids int32 x2 and hit float x4 per pixel, either pointer nullable, not both.
 * Both return VPT_ERR_UNSUPPORTED under a mesh shader (use vpt_session_pick / vpt_session_get_ids there). */
typedef struct vpt_sdf_pick {
  int32_t hit;                  /* 0 / 1 */
  int32_t vol_instance, sdf;    /* exactly one >= 0 on a hit */
  int32_t volume, material;
  float   distance;
  float   position[3];
  float   normal[3];
} vpt_sdf_pick;
int  vpt_session_pick_sdf(vpt_session* session, int x, int y, vpt_sdf_pick* out);
int  vpt_session_get_sdf_ids(vpt_session* session, int32_t* ids, float* hit);
/* ---- adaptive sampling in a session ------------------------------------------------------------------------
 * vpt_session_set_adaptive adopts the settings and resets; NULL switches the mode off (and resets).  Checked like
 * vpt_render_adaptive: threshold finite and >= 0, step >= 1, 1 <= min_samples <= render.samples (VPT_ERR_INVALID_ARG; a refused
 * call leaves the session exactly as it was).  While the mode is on, a vpt_session_reset whose params have samples < min_samples
 * is refused in the same way.  The mode survives resets and edits; render.samples is the per-pixel cap.
 * A reset (and so every vpt_session_edit* and rebuild, before the scene changes) drops the vpt_adaptive_run; the first advance
 * afterwards creates it, so a reset costs what it costs without the mode.
 * vpt_session_advance(s, nsamples) in adaptive mode runs ceil(nsamples / step) whole rounds (vpt_adaptive_run_rounds), fewer when
 * every pixel has stopped or the cap is reached - never a partial round, so the rounds do not depend on how advances are batched -
 * then image = vpt_resolve_hits_device(state), the filter if denoise = 1, the tone map.  It waits once per round for the 16-byte
 * read-back (counted in bytes_to_host).  When no pixel is active it is a no-op: 0 launches, state, image and displays untouched.
 * vpt_session_samples returns the largest hit count.
 * Variance rule with denoise = 1 in adaptive mode: S_a and S_n are not used.  After an advance, with R rounds run since the reset:
 * variance = vpt_box3_device(se2) of vpt_adaptive_run_noise_device if R >= 2, else the filter's spatial seed (no variance given).
 * Read-out, each VPT_ERR_INVALID_ARG while the mode is off:
 *   progress            rounds run since the reset, samples taken, pixels still rendering (each nullable)
 *   get_hits            the hit counts, row-major int32 (zeros before the first advance)
 *   get_noise           se2 and variance = box3(se2) as above, row-major float, either nullable, not both; refused before the first
 *                       advance after a reset that ran a round
 *   get_adaptive_stats  the Welford mean and m2 of every pixel, row-major float: the inputs of the se2 rule; refused likewise
 * Contract: after a reset and advances that ran R rounds in total, in any split into calls, get_state returns the bits of
 * make_state + vpt_render_adaptive with the same vpt_adaptive and params.samples = min(render.samples, R * step) - or, where that
 * is below min_samples, of make_state + vpt_render(R * step); `image` has the bits of get_render_hits of that state; `display` is
 * the tone map of `image`, or of the filtered image.  With threshold 0 the session is bit-identical in state, image and display
 * to one without the mode advanced by the same sample count, the variance handed to the filter excepted. */
int  vpt_session_set_adaptive(vpt_session* session, const vpt_adaptive* adaptive_or_null);
int  vpt_session_progress(const vpt_session* session, int* rounds, int64_t* rendered, int* active);
int  vpt_session_get_hits(vpt_session* session, int32_t* hits_rowmajor);
int  vpt_session_get_noise(vpt_session* session, float* se2, float* variance);
int  vpt_session_get_adaptive_stats(vpt_session* session, float* mean, float* m2);

/* per-launch profile of the last vpt_render_device on this scene (HIP events on `stream`); synchronises with that
 * launch.  Like vpt_render it returns VPT_ERR_HIP if a wave of the implicit kernel gave up on its watchdog (a wave
 * that has not finished after 300 s leaves the kernel instead of holding the GPU: a defect, never a workload). */
int vpt_last_kernel_ms(vpt_scene* scene, float* ms);
/* the watchdog check alone (synchronous; the caller has waited for its launches): VPT_ERR_HIP if any wave of the
 * implicit kernel on this scene handle has given up since the handle was created */
int vpt_check_watchdog(vpt_scene* scene);

/* How long every wave of the last vpt_render_device launch on this scene ran, in ticks of the 100 MHz wall clock:
 * what the next launch's longest-first order is made from, exposed for load-balance analysis (critical path = the
 * largest entry, slot time = their sum).  Wave w renders state slots 64 w .. 64 w + 63 - unless the launch split
 * costly tiles into several partly filled waves (below), in which case the entries follow the split launch's waves.
 * Synchronises with the launch.  *count = waves of the launch; at most `capacity` entries are written.
 *
 * Tile splitting.  A wave runs all samples of its pixels one after the other, so a launch is at least as long as its
 * costliest tile.  When a layout shares the frame among ranks (nranks > 1) the work per GPU falls with N and that
 * chain does not, and a small frame (fewer than three tiles per wave slot of the chip) is in the same position: from the
 * second full call on such a layout the mesh kernels run the costliest tiles as 2^k waves
 * that hold every 2^k-th pixel (fewer live lanes diverge less: a wave with 8 lanes takes ~0.45 of the time), chosen
 * once from the measured per-tile costs by simulating the launch's schedule.  Results do not depend on it (pixels own
 * their RNG streams).  VPT_SPLIT=0 disables it, VPT_SPLIT=1 considers it for every layout (it never pays on a full-size frame on one GPU). */
int vpt_last_wave_costs(vpt_scene* scene, unsigned* ticks, int capacity, int* count);

/* Bytes per primitive of the records the path tracers' BVH leaf tests / shading fetch on this scene: 64 / 96 in general (four corner
 * positions; four normals + four texcoords), 48 / 64 when every shape of the scene holds triangles (three corners; three normals with the
 * texcoords in their spare words).  Such a scene keeps both forms on the device: pathtrace and volpathtrace read the short ones on scenes
 * without emissive meshes that need a BVH walk and without SDF lights, everything else reads the general ones.  Same results either way
 * (VPT_NO_COMPACT_TRIANGLES=1 at scene creation keeps the general records only: the tests' A/B switch). */
int vpt_scene_record_bytes(const vpt_scene* scene, int* leaf_bytes, int* attribute_bytes);

/* intersect_bvh(bvh, scene, ray) (instance < 0) / intersect_bvh(bvh, scene, instance, ray) of yocto_bvh.h, for a
 * batch of `n` host rays {o.xyz, d.xyz} with the reference's default tmin = 1e-4, tmax = flt_max, through the
 * kernels' own traversal.  ids[2i..] = {instance, element} (-1, -1 on a miss), uvt[3i..] = {u, v, distance}.
 * Synchronous.  The parity tests use it to compare the traversal with the reference's bit for bit on rays path
 * tracing rarely produces (axis-aligned, grazing a box plane, denormal direction components). */
int vpt_intersect(vpt_scene* scene, int n, const float* rays, int instance, int32_t* ids, float* uvt);

/* build_bvh(bvh, bboxes, highquality = false) of the reference (libs/yocto/yocto_bvh.cpp:447-507, split_middle
 * :411-441) on the device: `n` boxes {min.xyz, max.xyz} in, the reference's node array and primitive order out - the
 * same nodes under the same ids, the same primitive permutation, the same float bits (the reference's build is depth
 * first over a stack with std::partition; csrc/vpt_bvh_build.hip says how a level-parallel build arrives at the same
 * arrays).  nodes: room for `capacity` >= max(1, 2 n - 1) entries; *num_nodes = entries written; primitives: n ints.
 * Synchronous.  SURVEY §8(f) row 4 (load-time callers of the hot path). */
int vpt_build_bvh(int device, const float* bboxes, int n, vpt_bvh_node* nodes, int capacity, int* num_nodes, int32_t* primitives);

/* The same build with the reference's other branch: build_bvh(bvh, bboxes, highquality = quality).  VPT_BVH_MIDDLE is vpt_build_bvh
 * (split_middle); VPT_BVH_SAH is split_sah (yocto_bvh.cpp:317-373), which no caller of the reference switches on because 45 passes
 * over every node's primitives are too slow on a CPU.  Another quality gives VPT_ERR_INVALID_ARG before anything is built.
 * The SAH rule is that of vpt_build_bvh except for how an internal node (more than 4 primitives) chooses `axis` and `split`:
 *  - cbbox is the box of the node's primitive centres, csize = cbbox.max - cbbox.min.  All three sizes zero: the node is cut in halves
 *    on axis 0, as in vpt_build_bvh.
 *  - Otherwise the search starts with min_cost = flt_max, split = 0.0f, axis = 0, and runs saxis = 0, 1, 2 outside and b = 1 .. 15
 *    inside: bsplit = cbbox.min[saxis] + ((float)b * csize[saxis]) / 16.0f.  Left is every primitive of the node whose centre on saxis
 *    is < bsplit, right is the rest; left_bbox and right_bbox are the merges of their boxes, starting from the invalid box
 *    (min = flt_max, max = -flt_max).
 *  - area(x) = ((1e-12f + (2 * sx) * sy) + (2 * sx) * sz) + (2 * sy) * sz with s = x.max - x.min.
 *    cost = (1 + ((float)left_n * area(left_bbox)) / area(cbbox)) + ((float)right_n * area(right_bbox)) / area(cbbox), where
 *    area(cbbox) is the area of the CENTRE box, as the reference has it.
 *  - A candidate wins only when cost < min_cost (strict): the first of equal costs wins, and a NaN or infinite cost never wins.  An
 *    empty side gives 0 * inf = NaN.  When no candidate wins the node is partitioned at 0.0f on axis 0.
 *  - Then the same std::partition by centre[axis] < split and the same halves fallback when one side is empty; node ids and primitive
 *    order follow as in vpt_build_bvh.
 *  - Every value is float32, nothing is fused, divisions are IEEE.
 * The device evaluates the 45 candidates of a node from 16 bins per axis (a primitive's bin is the number of borders its centre is not
 * below; candidate b is the sum and merge of bins 0 .. b-1, and of the rest) - the same counts and boxes whenever a node's 15 borders
 * do not decrease with b; a node where they do (a NaN or overflowing csize) is evaluated candidate by candidate.  DESIGN.md §22. */
#define VPT_BVH_MIDDLE 0
#define VPT_BVH_SAH 1
int vpt_build_bvh_quality(int device, const float* bboxes, int n, int quality, vpt_bvh_node* nodes, int capacity, int* num_nodes, int32_t* primitives);

/* The float32 half of one level of the reference's Catmull-Clark subdivision (tesselate_catmullclark,
 * libs/yocto_pathtrace/yocto_pathtrace.cpp:1119-1226) on the device.  The caller supplies the level's
 * topology (integers: host/vpt_tesselate.cpp builds it as the reference does): the cage's edges in the reference's numbering,
 * its faces (a quad with z == w is a triangle), the refined faces, and per refined vertex - old vertices first, then one per
 * edge, then one per face - its kind (`valence`: 0 locked boundary, 1 creased boundary, 2 smooth) and the items whose centroids
 * the reference's averaging pass adds to it, IN THE ORDER ITS LOOPS REACH THEM (items[offsets[v] .. offsets[v + 1]): valence 0:
 * the vertex id, once per contribution; valence 1: vertex pairs (a, b) of crease edges; valence 2: refined face ids).  The
 * device computes the refined points, the averages in that order and the correction: `new_vertices` (num_vertices + num_edges
 * + num_faces entries of `dim` floats) holds the same bits as the reference's `vert` after the level.  Synchronous; every
 * index is validated on the host before a kernel runs. */
typedef struct vpt_subdiv_level {
  int32_t        dim;                                   /* floats per vertex: 3 (positions) or 2 (texcoords) */
  int32_t        num_vertices, num_edges, num_faces;    /* of the cage                                        */
  int32_t        num_new_faces;
  const int32_t* edges;                                 /* int2 [num_edges]                                   */
  const int32_t* faces;                                 /* int4 [num_faces]                                   */
  const int32_t* new_faces;                             /* int4 [num_new_faces]                               */
  const int32_t* valence;                               /* [num_vertices + num_edges + num_faces]             */
  const int32_t* offsets;                               /* [that + 1]                                         */
  const int32_t* items;
  int64_t        num_items;
} vpt_subdiv_level;
int vpt_subdivide_vertices(int device, const vpt_subdiv_level* level, const float* vertices, float* new_vertices);
/* The rest of tesselate_surface's float work on the device (yocto_pathtrace.cpp:1239, 1256-1271), same ordered-list scheme, same bits:
 * vpt_vertex_normals   quads_normals (corners = 4; a quad with z == w is a triangle and adds to three vertices) / triangles_normals
 *                      (corners = 3) of yocto_shape.cpp:1478-1512: area-weighted face normals added per vertex IN FACE ORDER, normalised;
 *                      positions / normals are float3 arrays, faces int4 / int3.  The per-vertex face lists are built on the host here.
 * vpt_displace_vertices  new_positions = positions + normals * displacement * (mean(xyz(eval_texture(texture, uv, as_linear = true)))
 *                      [- 0.5 for an 8-bit texture]) (cpp:1259-1265) through the render kernels' own eval_texture; `texels` is the
 *                      texture's first texel (uchar4 or float4 by texture->is_float; texture->offset is ignored).
 * Synchronous; indices are validated on the host before a kernel runs. */
int vpt_vertex_normals(int device, int32_t num_vertices, const float* positions, int32_t num_faces, int32_t corners, const int32_t* faces, float* normals);
int vpt_displace_vertices(int device, const vpt_texture* texture, const void* texels, float displacement, int32_t num_vertices,
                          const float* positions, const float* normals, const float* texcoords, float* new_positions);

/* ---- baking a mesh into a signed-distance voxel grid -----------------------------------------------------------
 * The load-time producer of the `volume<float>` grids the implicit shaders render (the reference only loads them: load_volume,
 * yocto_sceneio.cpp:885-967).  The rule, which csrc/vpt_bake_rule.h states operation by operation for the kernel and for the host
 * mirror (host/vpt_bake.cpp: the same bits):
 *  - Sample point.  Voxel (i, j, k) is sampled at origin + (float)i * step per axis: float32, unfused.  voxels[x + y*W + z*W*H].
 *  - Value.  voxel = s * sqrt(d2): d2 the smallest squared distance from the sample point p to any kept triangle, s = -1 if
 *    dot(p - c, n) < 0 and +1 otherwise, c the closest point of the winning triangle, n the pseudonormal of the feature c lies on
 *    (Baerentzen & Aanaes 2005): the face, one of its three edges or one of its three vertices.  A point on the surface gives +0.
 *  - Distance.  Where c lies on an edge or a vertex, d2 = dot(p - c, p - c) summed x, y, z left to right.  Where it lies on the face,
 *    d2 = h * h with h = dot(p - a, n), a the triangle's first corner and n its unit face normal from the table below (float32, x, y, z
 *    left to right), and s is the sign of h: the height over the plane, which does not depend on where in the face c was found
 *    (the face's c is not read: on a narrow triangle its three areas cancel and |p - c| near the face was off by more than 1e-6).
 *  - Closest point.  The seven-region test of Ericson, Real-Time Collision Detection §5.1.5, float32, nothing fused, regions tested in
 *    the order vertex A, vertex B, edge AB, vertex C, edge AC, edge BC, face with the book's comparisons (<= 0, >= 0); the two edge
 *    parameters and the face's 1 / (va + vb + vc) are IEEE divisions.
 *  - Winner.  The lexicographic minimum of (d2, triangle index in the caller's order): the value depends on no visiting order, BVH
 *    shape or thread count.  A candidate whose d2 is NaN never wins (its comparisons are false).
 *  - Dropped triangles.  A triangle whose float32 cross product (b - a) x (c - a), unfused, is exactly {0, 0, 0} takes no part in
 *    distances or normals and is counted in dropped_triangles.  If none is left: VPT_ERR_INVALID_ARG.
 *  - Feature normals.  Computed on the host only, in double, once per bake, by vpt_bake_feature_normals (plain C++, no device call:
 *    the host's libm is the only one involved), 21 floats per triangle rounded to float32: face, edge ab, edge bc, edge ca, vertex a,
 *    b, c.  Face: the unit normal.  Edge: the sum of the unit face normals of every kept triangle on that edge.  Vertex: the sum over
 *    incident kept triangles of (angle at the vertex) * (unit face normal), the angle by acos of the clamped cosine.  Nothing is
 *    normalised: only the sign is read.  Adjacency is by POSITION BITS, not by index: two vertices whose three floats have the same
 *    bit patterns (after -0 becomes +0) are one vertex, so UV seams and per-face duplicated vertices do not open the surface.
 *    A dropped triangle's 21 floats are 0 and kept[t] = 0.
 *  - Validation, before any device call (VPT_ERR_INVALID_ARG, the message names the entry; `voxels` / `normals` untouched): non-null
 *    pointers, num_triangles >= 1, indices in range, every position, origin and step float finite, whd >= 1 with a product < 2^31.
 *    vpt_bake_feature_normals validates the whole descriptor too.
 *  - Stack.  The kernel walks a BVH over the kept triangles (the project's builder) with a per-lane stack of fixed capacity; the depth
 *    of the built tree is computed on the host, and a tree that needs more gives VPT_ERR_UNSUPPORTED with no kernel launched
 *    (stats->launches == 0), as vpt_scene_create does for its stacks.
 *  - VPT_BAKE_BRUTE=1 in the environment, read per call: no BVH, every voxel over every kept triangle.  The same bits (the tests' and
 *    the measurement's A/B switch).
 *  - Synchronous.  stats (nullable): bvh_nodes / bvh_depth (root = 0) of the tree (0 in the brute form), launches = bake kernels
 *    launched, device_ms = their time by HIP events. */
typedef struct vpt_bake_desc {
  int32_t num_vertices;  const float*   positions;  /* float3, grid-local space */
  int32_t num_triangles; const int32_t* triangles;  /* int3 */
  int32_t whd[3];                                   /* voxels per axis, each >= 1, product < 2^31 */
  float   origin[3], step[3];                       /* sample point of voxel (i,j,k), float32, unfused:
                                                       origin + (float)i * step  per axis */
} vpt_bake_desc;
typedef struct vpt_bake_stats { int32_t dropped_triangles, bvh_nodes, bvh_depth, launches; float device_ms; } vpt_bake_stats;
int vpt_bake_sdf(int device, const vpt_bake_desc* desc, float* voxels /* x + y*W + z*W*H */, vpt_bake_stats* stats /* may be NULL */);
int vpt_bake_feature_normals(const vpt_bake_desc* desc, float* normals /* 21 floats per triangle */, int32_t* kept /* 1/0 per triangle, may be NULL */);

/* ---- a quad mesh out of a signed-distance voxel grid --------------------------------------------------------------
 * The way back from vpt_bake_sdf and the sculpt: the iso surface of a grid as positions, normals and quads (naive surface nets), what
 * vpt_shape_data takes.  The reference has no mesher: an extension.  The rule, which csrc/vpt_sdf_mesh_rule.h states operation by
 * operation for the kernels (csrc/vpt_sdf_mesh.hip) and for the host mirror (host/vpt_sdf_mesh.cpp: the same bits; float32, unfused,
 * IEEE divisions):
 *  - Grid.  whd = (W, H, D), voxel (x, y, z) at voxels[x + y*W + z*W*H], sampled at origin + (float)i * step per axis (the bake's and the
 *    sculpt's voxel space).  inside(v) = v < iso: a NaN voxel is outside.
 *  - Cells.  Cell (x, y, z), 0 <= x < W-1 (and so on), has the corners (x+dx, y+dy, z+dz); it is active when 1 to 7 of them are inside.
 *  - Vertex of an active cell.  The twelve edges in order: the four x-edges at (dy,dz) = (0,0), (1,0), (0,1), (1,1), the four y-edges at
 *    (dz,dx) in the same order, the four z-edges at (dx,dy).  An edge from the lower corner a to the upper b crosses when inside(va) !=
 *    inside(vb), at t = (iso - va) / (vb - va), and t = 0.5f if !(t >= 0 && t <= 1).  The crossing point in unit-cell coordinates is t
 *    along the edge's axis and the edge's 0 / 1 offsets on the others; each coordinate is summed from 0 in edge order, u = sum /
 *    (float)count, and the position per axis is origin + ((float)x + u) * step: add, multiply, add.
 *  - Normal.  The gradient of the cell's trilinear interpolant at u (term order in the header), each component divided by its step, then
 *    the reference's normalize (the vector itself when its length is 0).  A component that comes out NaN is written as +0.
 *  - Ids.  A vertex's id is the rank of its cell among the active cells in voxel index order (x fastest).
 *  - Quads.  The grid edge from voxel X along axis a emits one quad when inside(X) != inside(X + e_a) and, with (a, b, c) a cyclic
 *    permutation of (x, y, z), 1 <= X_b <= dim_b - 2 and 1 <= X_c <= dim_c - 2 (all four cells around it exist).  Its corners are the
 *    vertices of the cells X - e_b - e_c, X - e_c, X, X - e_b in that order when X is inside; when X + e_a is inside the first is kept
 *    and the other three are reversed: the quads face out of the inside.  Quads are ordered by the owner voxel's index, then by axis.
 *    A sign change on an edge at the border of the grid emits nothing: the mesh is open where the surface leaves the grid.
 *  Every id and every float depends on no launch shape, block size or thread count.
 *  - Validation, before any device call (VPT_ERR_INVALID_ARG, the message names the entry; the outputs and *stats untouched): non-null
 *    desc, voxels and stats, whd >= 1 with a product < 2^31, origin, step and iso finite, every step > 0, capacities >= 0.
 *  - Outputs.  stats->num_vertices / num_quads are set first.  positions / normals: float3 per vertex (normals may be NULL), quads: int4
 *    per quad.  As with vpt_scene_get_lights, a NULL array is not written, and a capacity below the count of an array that is given is
 *    VPT_ERR_INVALID_ARG with the counts set and nothing written.  positions and quads NULL: only the counts are made (classify and scan).
 *    More than 2^31 - 1 quads: VPT_ERR_UNSUPPORTED.
 *  - A grid with an axis of one voxel has no cells: 0 vertices, 0 quads, no kernel launched (stats->launches == 0), no device looked
 *    for.  A grid without a sign change gives 0 / 0 as well: vpt_mesh_sdf finds that out from its host array (launches == 0, no device
 *    looked for), vpt_scene_mesh_volume from its two counting launches (launches == 2).
 *  - Synchronous.  launches: kernels and scans launched; device_ms: their time by HIP events.
 * vpt_mesh_sdf takes the grid from host memory.  vpt_scene_mesh_volume takes volume `volume` of a resident scene where it lies in the
 * voxel pool - no voxel crosses PCIe - and writes nothing to the scene.  desc NULL: iso 0, origin 0, step = res * W / (W - 1) per axis
 * (W - 1 taken as 1 on an axis of one voxel), the space the renderer's lookup reads the grid in before scalef; a desc that is given carries the
 * volume's whd.  region (nullable): a box of voxels inside the grid, meshed as a grid of its own - ids and order are those of the
 * rule applied to the sub-grid alone - with its vertices in place: cell x of the region lies at origin + ((float)(lo + x) + u) * step.
 * The host-array entry, the resident entry and the resident entry with a region of the whole grid give the same bytes. */
typedef struct vpt_sdf_mesh_desc { int32_t whd[3]; float origin[3], step[3], iso; } vpt_sdf_mesh_desc;
typedef struct vpt_sdf_mesh_region { int32_t lo[3], whd[3]; } vpt_sdf_mesh_region;
typedef struct vpt_sdf_mesh_stats { int32_t num_vertices, num_quads, launches; float device_ms; } vpt_sdf_mesh_stats;
int vpt_mesh_sdf(int device, const vpt_sdf_mesh_desc* desc, const float* voxels, float* positions, float* normals /* may be NULL */,
                 int32_t vertex_capacity, int32_t* quads, int32_t quad_capacity, vpt_sdf_mesh_stats* stats);
int vpt_scene_mesh_volume(vpt_scene* scene, int volume, const vpt_sdf_mesh_desc* desc /* may be NULL */, const vpt_sdf_mesh_region* region /* may be NULL */,
                          float* positions, float* normals, int32_t vertex_capacity, int32_t* quads, int32_t quad_capacity, vpt_sdf_mesh_stats* stats);

/* Device self-test of an arithmetic shortcut the kernels rely on for bit-exact parity: the reference divides
 * (1 / d per ray, yocto_bvh.cpp:806-808; 1 / det per triangle, yocto_geometry.h:690), the kernels use
 * v_rcp_f32 + one Newton step where every lane's operand has a biased exponent in 1..250.  Runs all 2^32 bit
 * patterns on `device` and returns in *mismatches how many in-range inputs differ from the IEEE quotient
 * (must be 0), in *fallbacks how many patterns are out of range (handled by a real division). */
int vpt_selftest_reciprocal(int device, unsigned long long* mismatches, unsigned long long* fallbacks);
/* Device self-test of the search structure that replaces std::upper_bound over a light's CDF in sample_discrete
 * (yocto_sampling.h:385-390; 21 dependent probes on a 2 M-texel environment map): `n` probe values - CDF
 * entries, their float neighbours, both ends, uniform values - are looked up through the guide table / 16-ary
 * levels and through the plain binary search; *mismatches must come back 0.  *indexed: 0 the light's CDF is
 * short and uses the binary search itself, 1 16-ary levels, 2 levels + guide table. */
int vpt_selftest_light_cdf(vpt_scene* scene, int light, int n, unsigned long long* mismatches, int* indexed);

#ifdef __cplusplus
}
#endif
#endif /* VPT_H_ */
