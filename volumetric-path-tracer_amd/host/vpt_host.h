// vpt_host.h — host-side mirror of the reference's renderer interface
// (libs/yocto_pathtrace/yocto_pathtrace.h:57-139): same type and function names, same
// argument meaning, same error behaviour, so a caller of the reference can switch by
// changing the namespace.  Everything that is *hot* (pathtrace_samples) goes through the
// C-ABI in include/vpt.h to the HIP kernels; everything here is load-time host work:
// scene containers, flattening, BVH build (yocto_bvh.cpp:411-611), light CDFs
// (yocto_pathtrace.cpp:983-1049) and per-pixel PCG32 seeding (yocto_pathtrace.cpp:960-980).
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "vpt.h"

namespace vpt {

using std::string;
using std::vector;

inline const int invalidid = -1;

// ---- small POD math (only what load-time code needs; no operator zoo) ----------------------
struct vec2f { float x = 0, y = 0; };
struct vec3f { float x = 0, y = 0, z = 0; };
struct vec4f { float x = 0, y = 0, z = 0, w = 0; };
struct vec2i { int x = 0, y = 0; };
struct vec3i { int x = 0, y = 0, z = 0; };
struct vec4i { int x = 0, y = 0, z = 0, w = 0; };
struct vec4b { uint8_t x = 0, y = 0, z = 0, w = 0; };
struct frame3f {
  vec3f x = {1, 0, 0}, y = {0, 1, 0}, z = {0, 0, 1}, o = {0, 0, 0};
};
static_assert(sizeof(frame3f) == sizeof(vpt_frame), "frame layout");

// ---- scene containers (yocto_scene.h:84-250, yocto_shape.h:74-87) ---------------------------
struct camera_data {
  frame3f frame        = {};
  bool    orthographic = false;
  float   lens = 0.050f, film = 0.036f, aspect = 1.500f, focus = 10000, aperture = 0;
};
struct texture_data {
  int           width = 0, height = 0;
  bool          linear  = false;
  vector<vec4f> pixelsf = {};
  vector<vec4b> pixelsb = {};
};
enum struct material_type { matte, glossy, reflective, transparent, refractive, subsurface, volumetric, gltfpbr };
inline const auto material_type_names = vector<string>{"matte", "glossy", "reflective",
    "transparent", "refractive", "subsurface", "volumetric", "gltfpbr"};
struct material_data {
  material_type type = material_type::matte;
  vec3f emission = {0, 0, 0}, color = {0, 0, 0};
  float roughness = 0, metallic = 0, ior = 1.5f;
  vec3f scattering   = {0, 0, 0};
  float scanisotropy = 0, trdepth = 0.01f, opacity = 1;
  int   emission_tex = invalidid, color_tex = invalidid, roughness_tex = invalidid,
      scattering_tex = invalidid, normal_tex = invalidid;
};
struct shape_data {
  vector<int>   points    = {};
  vector<vec2i> lines     = {};
  vector<vec3i> triangles = {};
  vector<vec4i> quads     = {};
  vector<vec3f> positions = {};
  vector<vec3f> normals   = {};
  vector<vec2f> texcoords = {};
  vector<vec4f> colors    = {};
  vector<float> radius    = {};
};
struct instance_data {
  frame3f frame = {};
  int     shape = invalidid, material = invalidid;
};
struct environment_data {
  frame3f frame        = {};
  vec3f   emission     = {0, 0, 0};
  int     emission_tex = invalidid;
};
enum struct sdf_type { bbox, box, capped_cone, plane, sphere, torus };
inline const auto sdf_type_names = vector<string>{"bbox", "box", "capped_cone", "plane", "sphere", "torus"};
struct sdf_data {  // tagged union instead of std::function (yocto_scene.h:194-200)
  int      material = invalidid;
  frame3f  frame    = {};
  vec3f    whd      = {0, 0, 0};
  sdf_type type     = sdf_type::plane;
  float    p[4]     = {0, 0, 0, 0};
};
struct volume_data {  // volume<float>
  vec3i         whd = {0, 0, 0};
  vector<float> vol = {};
  float         res = 0;
};
struct volume_instance {
  int     volume = invalidid, material = invalidid;
  float   scalef = 1;
  frame3f frame  = {};
};
struct subdiv_data {  // yocto_scene.h:161-183: face-varying control cage + subdivision / displacement settings
  vector<vec4i> quadspos = {}, quadsnorm = {}, quadstexcoord = {};
  vector<vec3f> positions = {}, normals = {};
  vector<vec2f> texcoords = {};
  int   subdivisions = 0;
  bool  catmullclark = true, smooth = true;
  float displacement     = 0;
  int   displacement_tex = invalidid;
  int   shape            = invalidid;
};
struct scene_data {
  vector<camera_data>      cameras       = {};
  vector<instance_data>    instances     = {};
  vector<environment_data> environments  = {};
  vector<shape_data>       shapes        = {};
  vector<texture_data>     textures      = {};
  vector<material_data>    materials     = {};
  vector<volume_data>      volumes       = {};
  vector<volume_instance>  vol_instances = {};
  vector<sdf_data>         sdfs          = {};
  vector<subdiv_data>      subdivs       = {};
  string                   copyright     = "";
};

// ---- bvh (yocto_bvh.h:73-92) ----------------------------------------------------------------
using bvh_node = vpt_bvh_node;
struct bvh_data {
  vector<bvh_node> nodes      = {};
  vector<int>      primitives = {};
  vector<bvh_data> shapes     = {};
};
using bvh_scene = bvh_data;

// ---- renderer API (yocto_pathtrace.h:57-139) ------------------------------------------------
struct rng_state {
  uint64_t state = 0x853c49e6748fea9bULL, inc = 0xda3e39cb94b95bdbULL;
};
struct pathtrace_state {
  int               width = 0, height = 0, samples = 0;
  vector<vec4f>     image = {};
  vector<int>       hits  = {};
  vector<rng_state> rngs  = {};
};
enum struct pathtrace_shader_type { volpathtrace, pathtrace, naive, eyelight, normal, texcoord, color, implicit, implicit_normal };
inline const auto pathtrace_shader_names = vector<string>{"volpathtrace", "pathtrace", "naive",
    "eyelight", "normal", "texcoord", "color", "implicit", "implicit_normal"};
// Extension: the shaders the reference does not have, beside its list - name and id (include/vpt.h: ids 9 .. 15 name nothing).
// A pathtrace_params carries one as (pathtrace_shader_type)id.
inline const auto pathtrace_extension_shaders = vector<std::pair<string, int>>{{"volgrid", 16}};
inline bool pathtrace_shader_known(pathtrace_shader_type shader) {
  if ((int)shader >= 0 && (int)shader <= (int)pathtrace_shader_type::implicit_normal) return true;
  for (auto& [name, id] : pathtrace_extension_shaders)
    if (id == (int)shader) return true;
  return false;
}
struct pathtrace_params {
  int                   camera              = 0;
  int                   resolution          = 720;
  pathtrace_shader_type shader              = pathtrace_shader_type::pathtrace;
  int                   samples             = 512;
  int                   bounces             = 4;
  bool                  noparallel          = false;
  int                   pratio              = 8;
  float                 exposure            = 0;
  bool                  filmic              = false;
  bool                  noimplicit_mis      = false;
  int                   spheretrace_maxiter = 450;
};
struct pathtrace_light {
  int           instance = invalidid, environment = invalidid, sdf = invalidid;
  vector<float> elements_cdf = {};
};
struct pathtrace_lights {
  vector<pathtrace_light> lights = {};
};
struct color_image {
  int           width = 0, height = 0;
  bool          linear = true;
  vector<vec4f> pixels = {};
};

pathtrace_state  make_state(const scene_data& scene, const pathtrace_params& params);
// `quality`: VPT_BVH_MIDDLE (the reference's highquality = false, what every caller of the reference uses) or VPT_BVH_SAH (highquality =
// true: split_sah, the rule at vpt_build_bvh_quality in include/vpt.h), for every tree of the scene; another value throws
// std::invalid_argument.  The host build is the plain form of the rule: 45 passes over a node's primitives.
bvh_scene        make_bvh(const scene_data& scene, const pathtrace_params& params, int quality = VPT_BVH_MIDDLE);
// Extension: the same trees (node for node, hash-equal) built on GPU `device` by vpt_build_bvh_quality; throws if that fails.
bvh_scene        make_bvh_device(const scene_data& scene, const pathtrace_params& params, int device = 0, int quality = VPT_BVH_MIDDLE);
// update_bvh(bvh, scene, updated_instances, updated_shapes) of the reference (yocto_bvh.h:100-103, yocto_bvh.cpp:509-524, 613-689): a
// refit.  Topology, node ids and primitive order stay; the boxes of the named shapes' BVHs, then of the scene BVH (from ALL
// instances: the reference does not read `updated_instances` either) are recomputed from invalidb3f with the bounds routines of
// make_bvh.  An instance of a shape without nodes gets invalidb3f as in make_bvh (the reference reads nodes[0] of an empty vector).
// The device counterpart is vpt_scene_update (include/vpt.h).
void             update_bvh(bvh_scene& bvh, const scene_data& scene, const vector<int>& updated_instances, const vector<int>& updated_shapes);
// make_bvh again for part of a scene (the host side of vpt_scene_rebuild_bvh, include/vpt.h): the named shapes' BVHs from their current
// vertices, then - `scene_level`, forced when a shape is named - the scene BVH over the current instances and roots.  Throws
// std::invalid_argument for a shape id out of range or repeated, or an unknown quality.  Every tree the call builds is built at
// `quality`; the trees it leaves alone keep theirs.
void             rebuild_bvh(bvh_scene& bvh, const scene_data& scene, const vector<int>& shapes, bool scene_level, int quality = VPT_BVH_MIDDLE);
// The set of instances changed (the host side of vpt_scene_update_instances, include/vpt.h): `set` entries replace the instances named
// by current ids, then the instances of `remove` (current ids) are erased - survivors keep their order, ids close up - then `add` is
// appended; the scene BVH is built anew over the new list (rebuild_bvh(bvh, scene, {}, true): the shapes' trees stay) and the lights
// are make_lights of the new scene.  Throws std::invalid_argument for an id out of range or repeated, an id both set and removed, or
// a shape or material out of range; the scene is untouched then.
void             edit_instances(scene_data& scene, bvh_scene& bvh, pathtrace_lights& lights, const vector<int>& remove, const vector<int>& set_ids,
                const vector<instance_data>& set, const vector<instance_data>& add);
// The shape list changed (the host side of vpt_scene_update_shapes, include/vpt.h): `set` entries replace the shapes named by current
// ids, then the shapes of `remove` (current ids) are erased - from the back; survivors keep their order, ids close up, every
// instance's shape id follows - then `add` is appended; make_bvh builds the trees of the replaced and the added shapes, the scene BVH
// is built anew when, and only when, a shape was replaced, and the lights are make_lights of the new scene.  Throws
// std::invalid_argument, the scene untouched, for an id out of range or repeated, an id both set and removed, a removed shape that an
// instance still names, or a shape vpt_scene_create would refuse (a vertex index out of range, both triangles and quads, points or
// lines mixed with other elements or without one radius per vertex, an attribute that differs from the positions in number).
void             edit_shapes(scene_data& scene, bvh_scene& bvh, pathtrace_lights& lights, const vector<int>& remove, const vector<int>& set_ids,
                const vector<shape_data>& set, const vector<shape_data>& add);
// build_bvh over `n` boxes {min.xyz, max.xyz} on the host (what make_bvh runs per shape and for the instances)
bvh_data         build_bvh_host(const float* bboxes, int n, int quality = VPT_BVH_MIDDLE);
pathtrace_lights make_lights(const scene_data& scene, const pathtrace_params& params);
// tesselate_surfaces (yocto_pathtrace.cpp:1119-1280): Catmull-Clark subdivision of every subdiv's cage (positions with
// creased boundaries, texcoords with locked boundaries), split_facevarying, quads_to_triangles, displacement along the
// vertex normals by the mean of the displacement texture (- 0.5 for 8-bit ones), smooth normals; replaces the subdiv's shape.
// Host arithmetic in the reference's order: the same float bits (tests/golden/*_stats.json hold the reference's hashes).
void             tesselate_surfaces(scene_data& scene);
// one level of the reference's tesselate_catmullclark (cpp:1119-1226) on a quad mesh whose vertices have `dim` (2 or 3)
// floats; a quad with z == w is a triangle.  quads / verts are replaced by the next level's.
void             tesselate_catmullclark(vector<vec4i>& quads, vector<float>& verts, int dim, bool lock_boundary);
// The two halves of a level.  Topology (integers): the refined faces and, per refined vertex, the ordered list of items the
// reference's averaging pass adds to it (layout: vpt_subdiv_level of include/vpt.h).  Vertices (float32): host form.
struct subdiv_level {
  int           nv = 0, ne = 0, nf = 0;
  vector<int>   edges;    // 2 per edge
  vector<vec4i> faces, tquads;
  vector<int>   valence, offsets, items;
};
void catmullclark_topology(const vector<vec4i>& quads, int num_vertices, bool lock_boundary, subdiv_level& level);
void subdivide_vertices(const subdiv_level& level, int dim, const vector<float>& verts, vector<float>& out);
// The integer half of one subdiv's tesselate_surface as the tesselation itself made it (the plan of vpt_scene_attach_subdiv,
// include/vpt.h): the position levels in order, quadspos after the last level, and split_facevarying's table - per shape vertex the
// indices {position, normal or -1, texcoord or -1} it was copied from.
struct subdiv_plan_host {
  vector<subdiv_level> levels;
  vector<vec4i>        quads;
  vector<vec3i>        verts;
};
// tesselate_surface of subdiv `index` as it is now (host arithmetic) into `shape` - the scene's own shape or a copy; plan: null, or
// where the run records its integer half.  One code path: the table the shape is gathered through IS the plan's.
void tesselate_subdiv(const scene_data& scene, int index, shape_data& shape, subdiv_plan_host* plan = nullptr);
// Extension: the same with every float stage on GPU `device` - the per-level vertex arithmetic (edge and face points, the
// averaging pass in face order, the correction pass: vpt_subdivide_vertices), the smooth normals before and after the
// displacement (vpt_vertex_normals) and the displacement itself (vpt_displace_vertices); the integer work - topology,
// split_facevarying, quads_to_triangles - stays on the host.  Same bits.
void             tesselate_surfaces_device(scene_data& scene, int device = 0);
// Single stages of tesselate_surface (device < 0: the host loops; else GPU `device`: vpt_vertex_normals / vpt_displace_vertices):
// quads_normals / triangles_normals (yocto_shape.cpp:1478-1512; corners = 4 / 3) and the displacement step (cpp:1259-1265).
vector<vec3f>    vertex_normals(const vector<vec3f>& positions, const int* faces, int num_faces, int corners, int device = -1);
vector<vec3f>    displace_vertices(const texture_data& texture, float displacement, const vector<vec3f>& positions, const vector<vec3f>& normals,
       const vector<vec2f>& texcoords, int device = -1);
// Progressively computes an image: ONE sample per pixel per call, on the GPU (vpt_render).
// Throws std::runtime_error("sampler unknown") for a bad shader (reference cpp:947-950) and
// std::runtime_error with vpt_last_error() if the HIP path is unavailable — there is no CPU
// fallback.
void pathtrace_samples(pathtrace_state& state, const scene_data& scene, const bvh_scene& bvh,
    const pathtrace_lights& lights, const pathtrace_params& params);
// Extension: `count` consecutive calls in one launch batch (same result).
void pathtrace_samples(pathtrace_state& state, const scene_data& scene, const bvh_scene& bvh,
    const pathtrace_lights& lights, const pathtrace_params& params, int count);
// Drop the cached device copy of `scene`.  pathtrace_samples notices by itself a scene rebuilt at the same address and every
// in-place edit of the small tables (cameras, instances, materials, environments, volume instances, SDFs, lights: hashed in full
// on each call; a camera edited in place goes to the resident copy through vpt_scene_update, anything else makes a new copy); in-place edits of BULK data - vertex arrays, texels, voxels, BVH nodes, light CDFs - are only sampled at head
// and tail and have to be announced with this call.
void pathtrace_release(const scene_data& scene);
// Extension: the GPUs pathtrace_samples renders on (default {0}).  With more than one, the frame's 8x8 tiles are dealt
// round-robin to them (vpt_multi of include/vpt.h); the result does not depend on the list.  Drops the cached copies.
void pathtrace_set_devices(const vector<int>& devices);
color_image get_render(const pathtrace_state& state);
void        get_render(color_image& render, const pathtrace_state& state);
// Extension: adaptive sampling (vpt_render_adaptive of include/vpt.h, whose rule decides when a pixel stops).  Every pixel renders
// in rounds of `step` samples until its noise meets `threshold` (relative standard error of its mean luminance; 0: never stops early),
// never before `min_samples` and at most params.samples; state.hits[] must be equal on entry (a fresh state: 0).  Renders on the
// first GPU of pathtrace_set_devices' list and refuses a list of several (std::invalid_argument).  state.samples becomes the largest
// hits[p]; the pixels keep their own counts, so the image is read with get_render_hits.
struct pathtrace_adaptive_params {
  float threshold   = 0;
  int   min_samples = 16;
  int   step        = 32;   // fewer rounds, fewer launch tails; a 32-spp round of the headline frame takes ~34 ms
};
struct pathtrace_adaptive_stats {
  int     rounds  = 0;   // rounds rendered
  int64_t samples = 0;   // samples taken over all pixels
};
pathtrace_adaptive_stats pathtrace_adaptive(pathtrace_state& state, const scene_data& scene, const bvh_scene& bvh,
    const pathtrace_lights& lights, const pathtrace_params& params, const pathtrace_adaptive_params& adaptive);
// get_render with each pixel's own sample count: image[p] * (1 / hits[p]), 0 where hits[p] == 0
color_image get_render_hits(const pathtrace_state& state);
void        get_render_hits(color_image& render, const pathtrace_state& state);
// Extension: denoise_render, which the reference declares beside get_albedo / get_normal and, without OpenImageDenoise, fills with a
// copy (yocto_trace.h:176-190, yocto_trace.cpp:1602-1604).  Here: the edge-avoiding à-trous filter whose rule include/vpt.h states
// word for word (vpt_denoise_params), on the CPU - the restatement the HIP kernels are held to bit for bit, usable without a GPU.
// `albedo` / `normal` are resolved renders of the `color` / `normal` (`implicit_normal`) shaders, `variance` an estimate of the variance of
// each pixel's mean luminance; an empty image / vector means "not given" (no variance: the spatial seed).  denoised.w == render.w.
struct denoise_params {
  int   iterations      = VPT_DENOISE_DEFAULT_ITERATIONS;
  float sigma_luminance = VPT_DENOISE_DEFAULT_SIGMA_LUMINANCE;
  float sigma_normal    = VPT_DENOISE_DEFAULT_SIGMA_NORMAL;
  float sigma_albedo    = VPT_DENOISE_DEFAULT_SIGMA_ALBEDO;
};
void denoise_render(color_image& denoised, const color_image& render, const color_image& albedo, const color_image& normal,
    const vector<float>& variance = {}, const denoise_params& params = {});
// the same on GPU `device` (vpt_denoise): same bits; throws std::runtime_error with vpt_last_error() if that fails
void denoise_render_device(color_image& denoised, const color_image& render, const color_image& albedo, const color_image& normal,
    const vector<float>& variance = {}, const denoise_params& params = {}, int device = 0);
// The variance of each pixel's mean luminance from two points of one sample chain: the radiance sums (pathtrace_state::image) after
// the first a samples and after all n, 0 < a < n (rule: include/vpt.h).  device < 0: host loops; else GPU `device`: same bits.
vector<float> half_variance(int width, int height, const vector<vec4f>& sum_a, int a, const vector<vec4f>& sum_n, int n, int device = -1);
// Extension: the first-hit AOVs of `params`' camera and resolution in one pass (include/vpt.h: vpt_render_aov): a fresh make_state,
// `samples` samples of one scene copy on the first device of pathtrace_set_devices, every ray traced once.  normal / albedo / texcoord
// have the bits of get_render after `samples` passes of the `normal` / `color` / `texcoord` shader; depth is {mean distance over the
// samples, 0, 0, coverage}; ids / uvt are {instance, element} and {u, v, distance} of each pixel's first sample (-1, -1 and zeros on a
// miss).  params.shader is ignored; SDFs and voxel grids are not seen.  Throws std::runtime_error with vpt_last_error() on failure.
// `planes`: which of them to render (aov_ids brings uvt along); the others are left empty.
enum aov_plane : unsigned { aov_normal = 1, aov_albedo = 2, aov_texcoord = 4, aov_depth = 8, aov_ids = 16, aov_all = 31 };
struct pathtrace_aov_images {
  color_image   normal = {}, albedo = {}, texcoord = {}, depth = {};
  vector<vec2i> ids = {};
  vector<vec3f> uvt = {};
};
pathtrace_aov_images pathtrace_aovs(const scene_data& scene, const bvh_scene& bvh, const pathtrace_lights& lights, const pathtrace_params& params,
    int samples = 16, unsigned planes = aov_all);
// Extension: the first-hit AOVs of the implicit shaders in one sphere-traced pass (include/vpt.h: vpt_render_sdf_aov), as pathtrace_aovs:
// a fresh make_state, `samples` samples, every camera ray marched once through spheretrace(scene, ray, params.spheretrace_maxiter).
// normal has the bits of get_render after `samples` passes of `implicit_normal`; albedo is the hit material's colour; depth is {mean t
// over the samples, 0, 0, coverage}; ids / hit are {vol_instance, sdf} and {position, t} of each pixel's first sample ({-1, -1} and
// zeros on a miss).  A first hit is reported whatever its material's opacity.  params.shader is ignored; meshes are not seen.
// `planes`: which of them to render (sdf_aov_ids brings hit along); the others are left empty.
enum sdf_aov_plane : unsigned { sdf_aov_normal = 1, sdf_aov_albedo = 2, sdf_aov_depth = 4, sdf_aov_ids = 8, sdf_aov_all = 15 };
struct pathtrace_sdf_aov_images {
  color_image   normal = {}, albedo = {}, depth = {};
  vector<vec2i> ids = {};
  vector<vec4f> hit = {};
};
pathtrace_sdf_aov_images pathtrace_sdf_aovs(const scene_data& scene, const bvh_scene& bvh, const pathtrace_lights& lights,
    const pathtrace_params& params, int samples = 16, unsigned planes = sdf_aov_all);
// The two guide renders of `params`' camera and resolution: a fresh make_state, `samples` passes of the `normal` and the `color` shader,
// get_render - for the mesh shaders both out of one pathtrace_aovs pass (the same bits).  For the implicit shaders: `implicit_normal`
// through pathtrace_samples, and no albedo (left empty).
struct denoise_guides {
  color_image normal = {}, albedo = {};
};
denoise_guides pathtrace_guides(const scene_data& scene, const bvh_scene& bvh, const pathtrace_lights& lights, const pathtrace_params& params,
    int samples = 16);

// ---- display: tone mapping, the preview, progressive sessions (include/vpt.h: vpt_session) ---------------------
// tonemap_image of the reference (yocto_image.h:242-250, yocto_image.cpp:877-888): tonemap(hdr, exposure, filmic, srgb) of
// yocto_color.h:306-316 per pixel, to floats or through float_to_byte (:207-211) to bytes.  Host arithmetic in the reference's order -
// the restatement vpt_tonemap_device is held to (bit for bit without srgb; with it the device's powf differs from libm's by ulps).
void tonemap_image(vector<vec4f>& ldr, const vector<vec4f>& hdr, float exposure, bool filmic = false, bool srgb = true);
void tonemap_image(vector<vec4b>& ldr, const vector<vec4f>& hdr, float exposure, bool filmic = false, bool srgb = true);
// the preview replicated to full size (apps/ypathtrace/ypathtrace.cpp:164-169): out[j * width + i] = preview[min(j / pratio, ph - 1)][min(i / pratio, pw - 1)]
void upscale_preview(color_image& out, const color_image& preview, int pratio, int width, int height);
// make_state's rngs for a width x height frame, every pixel by a jump of the master stream (csrc/vpt_rng_jump.h, which the kernel of
// vpt_state_init_device compiles too) instead of make_state's sequential draws: the same bits.  For the tests; make_state stays as it is.
vector<rng_state> make_state_rngs_jump(int width, int height);
// A progressive render of one camera on one GPU: vpt_session over the scene flattened and sent to `device` once.  reset() is the
// reference's reset_display (preview included), advance(n) n more samples and a fresh display; nothing but what display() / image() /
// state() fetch crosses PCIe.  Every member throws std::runtime_error with vpt_last_error() where the C-ABI fails.
struct render_session_params {
  pathtrace_params render   = {};   // pratio, exposure and filmic are read here
  bool             denoise  = false;
  denoise_params   filter   = {};
  int              guide_samples = 16;
};
class render_session {
 public:
  render_session(const scene_data& scene, const bvh_scene& bvh, const pathtrace_lights& lights, const render_session_params& params, int device = 0);
  ~render_session();
  render_session(const render_session&)            = delete;
  render_session& operator=(const render_session&) = delete;
  void reset();
  void reset(const render_session_params& params);
  void advance(int nsamples);
  void set_display(float exposure, bool filmic);
  // adaptive sampling in the session (vpt_session_set_adaptive): these settings from now on, params.render.samples being the per-pixel
  // cap, and a reset; a threshold < 0 switches the mode off.  advance(n) then runs ceil(n / step) whole rounds over the pixels still
  // rendering, samples() is the largest hit count, and image() holds every pixel over its own count.
  void set_adaptive(const pathtrace_adaptive_params& adaptive);
  struct progress_stats {
    int     rounds  = 0;   // rounds run since the reset
    int64_t samples = 0;   // samples taken over all pixels
    int     active  = 0;   // pixels still rendering
  };
  progress_stats progress() const;    // adaptive mode only
  bool           converged() const;   // adaptive mode only: no pixel is still rendering
  vector<int>    hits();              // adaptive mode only: the samples every pixel has taken, row-major
  int  width() const;
  int  height() const;
  int  samples() const;
  vector<vec4b>   display();                 // RGBA8, the device's tone map
  color_image     image(bool denoised = false);   // the linear image (get_render or the preview); denoised: the filtered one
  pathtrace_state state();

 private:
  vpt_scene*   scene_   = nullptr;
  vpt_session* session_ = nullptr;
};

// ---- baking a mesh into a signed-distance grid (include/vpt.h: vpt_bake_sdf; host/vpt_bake.cpp) ---------------------------------
// Extension: the producer of the volume<float> grids the implicit shaders render (the reference only loads them).
// fit_volume: the grid of `whd` voxels around the box [bmin, bmax] that the renderer's lookup (eval_sdf / eval_volume,
// yocto_sdfs.cpp:30-49, 92-127) reads back in place: that lookup puts voxel i of an axis at i * (res * W) / (W - 1) and knows one scalar
// `res` for all three, so step_a = (res * (float)W_a) / (float)(W_a - 1) with the smallest res for which the box plus `padding` voxels
// on each side fits on every axis, the box centred.  whd >= 2 * padding + 3 per axis, padding >= 0 (std::invalid_argument otherwise).
// instance: identity axes, frame.o = -origin, scalef = 1 (the reference reads the grid at transform_point(frame, world point)).
struct volume_fit {
  float           res    = 0;
  vec3f           origin = {}, step = {};
  volume_instance instance = {};
};
volume_fit fit_volume(const vec3f& bmin, const vec3f& bmax, const vec3i& whd, int padding = 2);
// the triangles of a shape: its own, and its quads split as the reference's geometry code does, (x, y, w) and (z, w, y); a quad
// with z == w is the triangle (x, y, z)
vector<vec3i> bake_triangles(const shape_data& shape);
// the host mirror of vpt_bake_sdf: the rule header over every voxel and every kept triangle on `threads` CPU threads (1..16), the same
// bits as the device; throws std::invalid_argument with the C-ABI's message for a descriptor it refuses (voxels untouched)
void bake_sdf(vector<float>& voxels, const vector<vec3f>& positions, const vector<vec3i>& triangles, const vec3i& whd, const vec3f& origin,
    const vec3f& step, vpt_bake_stats* stats = nullptr, int threads = 16);
// the same on GPU `device` (vpt_bake_sdf); throws std::runtime_error with vpt_last_error() if that fails
void bake_sdf_device(vector<float>& voxels, const vector<vec3f>& positions, const vector<vec3i>& triangles, const vec3i& whd,
    const vec3f& origin, const vec3f& step, int device, vpt_bake_stats* stats = nullptr);
// fit_volume around the mesh, then bake_sdf (device < 0) or bake_sdf_device: the volume and the instance that puts it where the mesh was
struct baked_volume {
  volume_data     volume   = {};
  volume_instance instance = {};
  vpt_bake_stats  stats    = {};
};
baked_volume bake_volume(const vector<vec3f>& positions, const vector<vec3i>& triangles, const vec3i& whd, int padding = 2, int device = -1);
// the binary .sdf layout load_volume reads: int32 w h d, float res, 16 floats (the identity; no reader uses them), the voxels
bool save_volume(const string& filename, const volume_data& vol, string& error);

// ---- sculpting a voxel grid with analytic SDF brushes (include/vpt.h: vpt_scene_sculpt_volumes; host/vpt_sculpt.cpp) -------------
// the host mirror of one entry: the rule header (csrc/vpt_sculpt_rule.h) in a plain loop over the entry's region of `volume`, its
// stamps taken from `stamps` (the edit's list of `num_stamps`) - the same bits as the device.  Refuses what the C-ABI refuses, in its
// words (false, `error` set, the volume untouched); entry.volume is the caller's to resolve.
bool sculpt_volume(volume_data& volume, const vpt_sculpt_entry& entry, const vpt_sculpt_stamp* stamps, int num_stamps, string& error);

// ---- a quad mesh out of a signed-distance voxel grid (include/vpt.h: vpt_mesh_sdf; host/vpt_sdf_mesh.cpp) ---------------------------
struct sdf_mesh {
  vector<vec3f> positions = {}, normals = {};
  vector<vec4i> quads     = {};
};
// the host mirror of vpt_mesh_sdf: the rule header (csrc/vpt_sdf_mesh_rule.h) in plain serial loops over the grid, or over `region` of it as
// vpt_scene_mesh_volume takes one - the same bits as the device; throws std::invalid_argument with the C-ABI's words for what it refuses
sdf_mesh mesh_sdf(const float* voxels, const vpt_sdf_mesh_desc& desc, const vpt_sdf_mesh_region* region = nullptr);
// the same on GPU `device` (vpt_mesh_sdf); throws std::runtime_error with vpt_last_error() if that fails
sdf_mesh mesh_sdf_device(const float* voxels, const vpt_sdf_mesh_desc& desc, int device);
// positions, normals (unless empty) and quads as a binary little-endian PLY file, which load_shape reads back with the same bits
bool save_mesh_ply(const string& filename, const sdf_mesh& mesh, string& error);

// ---- flattening to the C-ABI ----------------------------------------------------------------
struct flat_scene {
  vpt_scene_desc desc = {};
  // backing storage for desc
  vector<vpt_camera> cameras; vector<vpt_instance> instances; vector<vpt_shape> shapes;
  vector<vpt_material> materials; vector<vpt_texture> textures;
  vector<vpt_environment> environments; vector<vpt_volume> volumes;
  vector<vpt_volume_instance> vol_instances; vector<vpt_sdf> sdfs; vector<vpt_light> lights;
  vector<vec3f> positions, normals; vector<vec2f> texcoords; vector<vec4f> colors;
  vector<vec3i> triangles; vector<vec4i> quads;
  vector<vpt_shape_curves> shape_curves; vector<int> points; vector<vec2i> lines; vector<float> radius;
  vpt_scene_curves curves = {};   // points and lines beside desc (include/vpt.h); shape_curves null: no shape has any
  const vpt_scene_curves* curves_or_null() const { return curves.shape_curves ? &curves : nullptr; }
  vector<vec4f> texels_f; vector<vec4b> texels_b; vector<float> voxels, light_cdf;
  vector<bvh_node> scene_nodes, shape_nodes; vector<int> scene_prims, shape_prims;
  flat_scene() = default;
  flat_scene(const flat_scene&) = delete;
  flat_scene& operator=(const flat_scene&) = delete;
};
// Throws std::invalid_argument for a shape that mixes points, lines and faces (vpt.h: vpt_shape_curves).
void flatten_scene(flat_scene& flat, const scene_data& scene, const bvh_scene& bvh,
    const pathtrace_lights& lights);
vpt_params to_abi(const pathtrace_params& params);

// ---- scene / image IO (yocto_sceneio.h:89-211 subset: JSON 4.2, binary+ascii PLY, OBJ geometry (v / vn / vt / f / l / p),
//      PNG, HDR, .sdf text/binary) ----------------------------------------------------------------------
bool load_scene(const string& filename, scene_data& scene, string& error);
bool load_shape(const string& filename, shape_data& shape, string& error, bool flip_texcoord);
bool load_subdiv(const string& filename, subdiv_data& subdiv, string& error);
bool load_texture(const string& filename, texture_data& texture, string& error);
bool load_volume(const string& filename, volume_data& vol, bool binary, string& error);
bool save_image(const string& filename, const color_image& image, string& error);
// a JSON array of camera objects with the keys of a scene file's "cameras" entries (ypathtrace --cameras); not empty
bool load_cameras(const string& filename, vector<camera_data>& cameras, string& error);
// the members of a --config file (yocto_cli.cpp:912-945) as (option name, value text) pairs
bool load_cli_config(const string& filename, vector<std::pair<string, string>>& options, string& error);
// output quantisation (yocto_color.h:207-231, yocto_image.cpp:870-874)
vector<vec4b> linear_to_srgb8(const color_image& image);
// bit-faithful restatement of the reference's baseline JPEG writer at quality 75
// (libs/yocto/ext/stb_image_write.h:1250-1611); needed by the parity metric
vector<uint8_t> encode_jpeg_q75(int width, int height, const vector<vec4b>& rgba);
vector<uint8_t> encode_png(int width, int height, const vector<vec4b>& rgba);

}  // namespace vpt
