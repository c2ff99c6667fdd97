// vpt_capi.hip — implementation of the C-ABI in include/vpt.h: upload of the scene tables vpt_scene_prep.cpp builds
// (the device layout of vpt_device.h), kernel launches.  The kernels are declared in vpt_launch.h and
// compiled in the kernel units it lists; this unit holds none of their bodies.  The launch schedule is vpt_schedule.hip's,
// the movement of a state between host arrays and tile-major slots vpt_layout.hip's.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared (see __graft_entry__.py).
// There is NO CPU fallback in this library: without a gfx950 device every compute entry point
// fails with VPT_ERR_NO_DEVICE.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <climits>
#include <memory>
#include <type_traits>
#include <string>
#include <vector>

#include "vpt_adaptive.h"
#include "vpt_bvh_rebuild.h"
#include "vpt_device_buffer.h"
#include "vpt_instance_update.h"
#include "vpt_error.h"
#include "vpt_kat.h"
#include "vpt_launch.h"
#include "vpt_layout.h"
#include "vpt_light_update.h"
#include "vpt_resident.h"
#include "vpt_schedule.h"
#include "vpt_scene_prep.h"
#include "vpt_scene_update.h"
#include "vpt_subdiv_update.h"
#include "vpt_shape_update.h"
#include "vpt_texture_update.h"
#include "vpt_sculpt.h"
#include "vpt_volume_update.h"

static std::string& g_error_text() {   // the message of the last failure on the calling thread (vpt_last_error)
  thread_local std::string text;
  return text;
}

int vpt_set_error(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error_text() = buf;
  return code;
}

struct vpt_scene : resident {   // the tables and what edits them (vpt_resident.h), and the render side
  int                        stack_cap = 16;    // binary-BVH walk of the implicit kernels' mesh-light pdf: refs only
  int                        stack_lds4 = 8, stack_spill4 = 0;   // quad-node traversal: (ref, t0) entries in LDS / in HBM
  device_buffer              spill;
  long long                  spill_lanes = 0;
  launch_schedule sched;   // per-wave costs, launch order, tile splitting (vpt_schedule.h)
  layout_staging staging;   // of the host-state entry points vpt_render() and vpt_render_adaptive(): allocated once per frame size
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool       timed = false;
  device_buffer d_watchdog;   // unsigned: waves of the implicit kernel that gave up (must stay 0; vpt_implicit_kernel.hip.h)
  bool       curves = false;          // some instanced shape holds points or lines: the VPT_FEAT_CURVES instances of K1
};

namespace {

// one allocation per table, never empty: no kernel is handed a null table
template <typename T>
int upload(vpt_scene* s, const T** out, const T* host, size_t count) {
  s->tables.emplace_back();
  if (int rc = s->tables.back().allocate(count * sizeof(T))) return rc;
  *out = s->tables.back().get<const T>();
  if (count) HIP_TRY(hipMemcpy(s->tables.back().get(), host, count * sizeof(T), hipMemcpyHostToDevice));
  return VPT_OK;
}
template <typename T>
int upload(vpt_scene* s, const T** out, const std::vector<T>& host) { return upload(s, out, host.data(), host.size()); }

// light_prims: corners and element normals of the single-leaf mesh lights, by the device's own eval_element_normal
int light_setup(vpt_scene* s) {
  if (s->d.num_lights <= 0) return VPT_OK;
  hipLaunchKernelGGL(vpt_light_setup_kernel, dim3(s->d.num_lights), dim3(64), 0, 0, s->d, const_cast<float4*>(s->d.light_prims));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return VPT_OK;
}

// the medium records behind the light records, by the device's own eval_material_at: at creation and whenever an edit has
// rewritten materials or rebuilt the table
int medium_setup(vpt_scene* s) {
  if (s->d.num_materials <= 0) return VPT_OK;
  hipLaunchKernelGGL(vpt_medium_setup_kernel, dim3((s->d.num_materials + 63) / 64), dim3(64), 0, 0, s->d, const_cast<float4*>(s->d.light_rec) + 8 * (size_t)s->d.num_lights);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  return VPT_OK;
}

}  // namespace

extern "C" {

const char* vpt_last_error(void) { return g_error_text().c_str(); }
const char* vpt_version(void) { return "vpt-mi355x 0.1 (gfx950)"; }

int vpt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void vpt_scene_destroy(vpt_scene* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);   // the scene's buffers are freed on its device when it goes
  for (hipEvent_t e : {s->ev0, s->ev1, s->upd_ev0, s->upd_ev1})
    if (e) (void)hipEventDestroy(e);
  delete s;
}

int vpt_scene_create(const vpt_scene_desc* desc, int device, vpt_scene** out) { return vpt_scene_create_curves(desc, nullptr, device, out); }

int vpt_scene_create_curves(const vpt_scene_desc* desc, const vpt_scene_curves* curves, int device, vpt_scene** out) {
  if (!desc || !out) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  scene_tables t;   // every host-side refusal happens here, before any device call
  if (int rc = prepare_scene(*desc, curves, t)) return rc;
  int ndev = vpt_device_count();
  if (ndev <= 0) return vpt_set_error(VPT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return vpt_set_error(VPT_ERR_INVALID_ARG, "device %d out of range (%d devices)", device, ndev);
  (void)hipGetLastError();   // start from a clean slate: an error left behind by an unrelated earlier call is not this call's
  HIP_TRY(hipSetDevice(device));
  const vpt_scene_desc& d = *desc;
  vpt_scene* s = new vpt_scene{};
  s->device    = device;
  struct guard { vpt_scene*& s; ~guard() { if (s) vpt_scene_destroy(s); } } g{s};
  DScene& D = s->d = t.d;   // the scalar fields; the tables follow, the descriptor's own ones straight from its arrays
  static_assert(sizeof(vpt_bvh_node) == 2 * sizeof(float4), "bvh node = 2 x float4");
  int rc = VPT_OK;
#define UP(...) if ((rc = upload(s, __VA_ARGS__)) != VPT_OK) return rc
  UP(&D.scene_nodes, (const float4*)d.scene_bvh_nodes, 2 * (size_t)d.num_scene_bvh_nodes); UP(&D.scene_prims, d.scene_bvh_prims, d.num_scene_bvh_prims);
  UP(&D.shape_nodes, (const float4*)d.shape_bvh_nodes, 2 * (size_t)d.num_shape_bvh_nodes);
  UP(&D.leaf_prims, t.leaf_prims); UP(&D.leaf_attrs, t.leaf_attrs);
  if (!t.tri_prims.empty()) { UP(&D.tri_prims, t.tri_prims); UP(&D.tri_attrs, t.tri_attrs); }   // else null: a scene with quads
  UP(&D.scene_wnodes, t.wnodes); UP(&D.scene_enter, t.enter); UP(&D.slot_of_instance, t.h.slot_of);
  UP(&D.instances, t.instances); UP(&D.shapes, t.shapes); UP(&D.elems, t.elems);
  UP(&D.positions, t.positions); UP(&D.normals, t.normals); UP(&D.texcoords, t.texcoords); UP(&D.colors, t.colors);
  UP(&D.materials, d.materials, d.num_materials); UP(&D.textures, d.textures, d.num_textures);
  UP(&D.texels_f, (const float4*)d.texels_f, d.num_texels_f); UP(&D.texels_b, (const uchar4*)d.texels_b, d.num_texels_b);
  UP(&D.srgb_lut, t.srgb_lut); UP(&D.environments, d.environments, d.num_environments); UP(&D.env_inv, t.env_inv);
  UP(&D.lights, d.lights, d.num_lights); UP(&D.light_cdf, d.light_cdf, d.num_light_cdf);
  UP(&D.light_index, t.light_index); UP(&D.light_index_pool, t.light_index_pool); UP(&D.light_guide, t.light_guide); UP(&D.light_rec, t.light_rec);
  UP(&D.light_prims, std::vector<float4>(20 * (size_t)d.num_lights, make_float4(0, 0, 0, 0)));   // vpt_light_setup_kernel fills it
  UP(&D.volumes, d.volumes, d.num_volumes); UP(&D.voxels, d.voxels, d.num_voxels); UP(&D.vol_instances, d.vol_instances, d.num_vol_instances);
  UP(&D.sdfs, d.sdfs, d.num_sdfs); UP(&D.sdf_inv, t.sdf_inv); UP(&D.sdf_fn_rec, t.sdf_fn_rec); UP(&D.sdf_grid_rec, t.sdf_grid_rec);
  UP(&D.cameras, d.cameras, d.num_cameras);
#undef UP
  D.shape_wnodes = D.scene_wnodes + t.scene_wnodes;
  s->stack_cap = t.stack_cap, s->stack_lds4 = t.stack_lds4, s->stack_spill4 = t.stack_spill4, s->light_features = t.light_features;
  s->curves = t.curves, s->varying_media = t.varying_media, s->num_shape_nodes = d.num_shape_bvh_nodes;
  s->num_shape_wnodes = (long long)t.shape_wnodes, s->shape_depth = t.shape_depths, s->shape_need4 = t.shape_need4s, s->shape_quads = t.shape_quads;
  s->scene_depth = t.scene_depth, s->scene_need4 = t.scene_need4;
  s->num_positions = d.num_positions, s->num_normals = d.num_normals, s->num_texcoords = d.num_texcoords, s->num_colors = d.num_colors;
  s->h = std::move(t.h), s->m = std::move(t.m);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  s->sched.compute_units = prop.multiProcessorCount;
  if ((rc = light_setup(s)) != VPT_OK) return rc;
  if ((rc = medium_setup(s)) != VPT_OK) return rc;
  for (hipEvent_t* e : {&s->ev0, &s->ev1}) HIP_TRY(hipEventCreate(e));
  if ((rc = s->d_watchdog.allocate(4)) != VPT_OK) return rc;
  HIP_TRY(hipMemset(s->d_watchdog.get(), 0, 4));
  HIP_TRY(hipDeviceSynchronize());
  *out = s;
  s    = nullptr;   // release the guard
  return VPT_OK;
}

}  // extern "C"

// HBM part of the traversal stacks for a launch of `lanes` lanes (only scenes whose worst case exceeds the LDS part)
static int stack_config(vpt_scene* s, long long lanes, stack_cfg& cfg) {
  if (s->stack_spill4 > 0 && lanes > s->spill_lanes) {
    s->spill_lanes = 0;
    if (int rc = s->spill.allocate((size_t)lanes * (size_t)s->stack_spill4 * sizeof(int2))) return rc;
    s->spill_lanes = lanes;
  }
  cfg.cap = s->stack_lds4, cfg.spill = s->stack_spill4, cfg.mem = s->spill.get<int2>(), cfg.lanes = lanes;
  return VPT_OK;
}

// what a call that renders hands to the kernel launchers, whatever the grid and the sample count of a launch
struct launch_ctx {
  vpt_scene*        s;
  hipStream_t       st;
  float4*           img;
  int*              hit;
  ulonglong2*       rng;
  stack_cfg         stack;
};

// K1 (mesh shaders): the instance compiled for the features this scene has (vpt_scene.hip.h: VPT_FEAT_*), launched over `grid`
// with the schedule `sch` - by launch_schedule::run (vpt_render_device) and by the rounds of vpt_render_device_adaptive
template <int K>
static void launch_mesh_instance(const launch_ctx& L, bool is_pilot, dim3 grid, const DParams& pr, const sched_cfg& sch) {
  vpt_scene* s = L.s;
  size_t lds = (size_t)s->stack_lds4 * 2 * VPT_BLOCK * sizeof(int) + 5 * VPT_BLOCK * sizeof(float);   // (ref, t0) pairs + the parked words
  // (the general instance also for a scene whose media vary over the surface: the others read a medium from its material's record;
  // VPT_MEDIUM_REGS=1, read per launch, sends any scene there - same bits: the tests' and the measurements' A/B switch)
  const int need = getenv("VPT_NO_LEAN") || getenv("VPT_MEDIUM_REGS") || s->varying_media ? VPT_FEAT_ALL : s->light_features;
  auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(VPT_BLOCK), lds, L.st, s->d, pr, L.img, L.hit, L.rng, L.stack, sch); };
  auto launch_feat = [&](auto feat) {
    constexpr int F = decltype(feat)::value;
    if (is_pilot && L.stack.spill) launch(vpt_mesh_pilot_kernel<K, true, F>);
    else if (is_pilot) launch(vpt_mesh_pilot_kernel<K, false, F>);
    else if (L.stack.spill) launch(vpt_mesh_kernel<K, true, F>);
    else launch(vpt_mesh_kernel<K, false, F>);
  };
  // three instances: single-leaf mesh lights only / + emissive meshes with a BVH / everything (SDF lights too)
  // (+ the compact-record form of the first for the two path tracers on scenes of triangles; the pilot runs on the general records)
  // (a scene with points or lines: the one instance with every light feature and the point / line tests, vpt_k1_curves.hip)
  if (s->curves) launch_feat(std::integral_constant<int, VPT_FEAT_ALL | VPT_FEAT_CURVES>{});
  else if ((K == K_VOLPATH || K == K_PATH) && (need & (VPT_FEAT_LARGE_LIGHTS | VPT_FEAT_SDF_LIGHTS)) == 0 && s->d.tri_prims && !is_pilot) {
    if constexpr (K == K_VOLPATH || K == K_PATH) {
      if (L.stack.spill) launch(vpt_mesh_kernel<K, true, VPT_FEAT_SMALL_LIGHTS | VPT_FEAT_COMPACT_TRIS>);
      else launch(vpt_mesh_kernel<K, false, VPT_FEAT_SMALL_LIGHTS | VPT_FEAT_COMPACT_TRIS>);
    }
  } else if ((need & (VPT_FEAT_LARGE_LIGHTS | VPT_FEAT_SDF_LIGHTS)) == 0) launch_feat(std::integral_constant<int, VPT_FEAT_SMALL_LIGHTS>{});
  else if ((need & VPT_FEAT_SDF_LIGHTS) == 0) launch_feat(std::integral_constant<int, VPT_FEAT_SMALL_LIGHTS | VPT_FEAT_LARGE_LIGHTS>{});
  else launch_feat(std::integral_constant<int, VPT_FEAT_ALL>{});
}
// K2 (implicit shaders): LDS of a launch (the refs-only stack + the scene's SDF records); VPT_ERR_UNSUPPORTED when they do not fit
static int implicit_lds(const vpt_scene* s, size_t* bytes = nullptr) {
  const size_t lds = (size_t)s->stack_cap * VPT_BLOCK * sizeof(int) +                                      // refs-only stack
        (6 * (size_t)s->d.num_sdfs + 7 * (size_t)s->d.num_vol_instances) * sizeof(float4);   // the SDF records
  if (lds > 64 * 1024) return vpt_set_error(VPT_ERR_UNSUPPORTED, "scene has too many SDFs for the implicit kernel's LDS copy of their records (%d + %d)", s->d.num_sdfs, s->d.num_vol_instances);
  if (bytes) *bytes = lds;
  return VPT_OK;
}
// the instance for the features this scene's lights have (VPT_FEAT_*): SDF scenes without emissive meshes run one without the mesh-light walks
template <int K>
static void launch_implicit_instance(const launch_ctx& L, bool is_pilot, dim3 grid, const DParams& pr, const sched_cfg& sch) {
  vpt_scene* s = L.s;
  size_t     lds = 0;
  (void)implicit_lds(s, &lds);   // checked by the callers before they launch
  unsigned long long watchdog_ticks = VPT_K2_WATCHDOG_TICKS;
  if (const char* e = getenv("VPT_K2_WATCHDOG_MS")) watchdog_ticks = strtoull(e, nullptr, 10) * 100000ull;   // tests of the error path
  const bool lean = (s->light_features & (VPT_FEAT_LARGE_LIGHTS | VPT_FEAT_SMALL_LIGHTS)) == 0 && !getenv("VPT_NO_LEAN");
  auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(VPT_BLOCK), lds, L.st, s->d, pr, L.img, L.hit, L.rng, s->stack_cap, sch, s->d_watchdog.get<unsigned>(), watchdog_ticks); };
  if (is_pilot && lean) launch(vpt_render_pilot_kernel<K, VPT_FEAT_SDF_LIGHTS>);
  else if (is_pilot) launch(vpt_render_pilot_kernel<K, VPT_FEAT_ALL>);
  else if (lean) launch(vpt_render_kernel<K, VPT_FEAT_SDF_LIGHTS>);
  else launch(vpt_render_kernel<K, VPT_FEAT_ALL>);
}
// the launcher of the kernel instances of `shader`: the one table of vpt_render_device and of the rounds of
// vpt_render_device_adaptive (both have checked the shader's range)
using instance_launcher = void (*)(const launch_ctx&, bool is_pilot, dim3 grid, const DParams&, const sched_cfg&);
static instance_launcher launcher_of(int shader) {
  switch (shader) {
    case VPT_SHADER_VOLPATHTRACE: return launch_mesh_instance<K_VOLPATH>;
    case VPT_SHADER_PATHTRACE: return launch_mesh_instance<K_PATH>;
    case VPT_SHADER_NAIVE: return launch_mesh_instance<K_NAIVE>;
    case VPT_SHADER_EYELIGHT: return launch_mesh_instance<K_EYELIGHT>;
    case VPT_SHADER_IMPLICIT: return launch_implicit_instance<K_IMPLICIT>;
    case VPT_SHADER_IMPLICIT_NORMAL: return launch_implicit_instance<K_IMPLICIT_NORMAL>;
    default: return launch_mesh_instance<K_DEBUG>;   // VPT_SHADER_NORMAL, _TEXCOORD, _COLOR
  }
}

// vpt_resolve_device / vpt_resolve_srgb8_device: the accumulators of every rank's tiles, over `samples`, as row-major pixels
template <typename Kernel, typename Pixel>
static int resolve(Kernel kernel, const vpt_layout* layout, const void* d_tiles_all_ranks, int samples, Pixel* d_rowmajor, void* stream) {
  if (!layout || !d_tiles_all_ranks || !d_rowmajor || samples <= 0) return vpt_set_error(VPT_ERR_INVALID_ARG, "bad argument");
  DParams pr;
  if (int rc = vpt_layout_dparams(layout, pr)) return rc;
  long long total = (long long)pr.nslots * pr.nranks;
  if (total >= (1LL << 31)) return vpt_set_error(VPT_ERR_INVALID_ARG, "image too large");
  int blocks = (int)((total + 255) / 256);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, pr, (const float4*)d_tiles_all_ranks, 1.0f / (float)samples, d_rowmajor);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

extern "C" {

int vpt_render_device(vpt_scene* s, const vpt_params* params, const vpt_layout* layout, int nsamples, void* d_image,
    void* d_hits, void* d_rng, void* stream) {
  if (!s || !params || !layout || !d_image || !d_hits || !d_rng) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  if (params->shader < 0 || params->shader > VPT_SHADER_IMPLICIT_NORMAL) return vpt_set_error(VPT_ERR_UNKNOWN_SHADER, "sampler unknown");
  if (params->camera < 0 || params->camera >= s->d.num_cameras) return vpt_set_error(VPT_ERR_INVALID_ARG, "camera %d out of range", params->camera);
  if (nsamples < 0 || params->bounces < 0) return vpt_set_error(VPT_ERR_INVALID_ARG, "negative sample/bounce count");
  if (nsamples == 0) return VPT_OK;
  DParams pr;
  if (int rc = make_dparams(params, layout, nsamples, pr)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  dim3   grid((pr.nslots + VPT_BLOCK - 1) / VPT_BLOCK);
  stack_cfg stack;
  if (int rc = stack_config(s, (long long)grid.x * VPT_BLOCK, stack)) return rc;
  // K1 considers tile splitting when the launch is short of waves (vpt_split_policy.cpp).  K2 considers it on every layout (unless
  // VPT_SPLIT=0): K2's launches hold two waves per wave slot at 1280 x 533, so the longest-first schedule ends well above both of
  // its bounds (226 ms against a longest wave of 192 and 191 of work per slot); the costliest tiles as partly filled waves - whose
  // scene rounds run in the group form: four lanes per ray - pack better.
  const bool k2 = params->shader >= VPT_SHADER_IMPLICIT;
  if (k2)
    if (int rc = implicit_lds(s)) return rc;   // the scene's SDF records must fit the kernel's LDS
  const bool may_split = k2 ? split_mode() != 0
                            : !stack.spill && (split_mode() == 1 || split_forced_k() >= 0 ||
                                               (split_mode() < 0 && (pr.nranks > 1 || (long long)grid.x < 3ll * s->sched.wave_slots(false))));
  const long long key[10] = {pr.nslots, pr.width, pr.height, params->shader, params->camera, params->bounces, pr.rank, pr.nranks, pr.tile_w, pr.tile_h};
  HIP_TRY(hipEventRecord(s->ev0, st));
  const launch_ctx L = {s, st, (float4*)d_image, (int*)d_hits, (ulonglong2*)d_rng, stack};
  if (int rc = s->sched.run(key, grid, nsamples, st, may_split, k2,
          [&](bool is_pilot, dim3 part_grid, int part_samples, const sched_cfg& sch) {
            DParams part = pr;
            part.nsamples = part_samples;
            launcher_of(params->shader)(L, is_pilot, part_grid, part, sch);
          }))
    return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev1, st));
  s->timed = true;
  return VPT_OK;
}

int vpt_scene_get_device(const vpt_scene* s) { return s ? s->device : vpt_set_error(VPT_ERR_INVALID_ARG, "null argument"); }

int vpt_scene_record_bytes(const vpt_scene* s, int* leaf_bytes, int* attribute_bytes) {
  if (!s || !leaf_bytes || !attribute_bytes) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  *leaf_bytes = s->d.tri_prims ? 48 : 64, *attribute_bytes = s->d.tri_attrs ? 64 : 96;
  return VPT_OK;
}

}  // extern "C"

// ---- editing a resident scene (include/vpt.h; the work is the update units') -------------------------------------------------
const resident& resident_of(const vpt_scene* s) { return *s; }   // for vpt_scene_inspect.hip, which reads the tables back

static bool moves_geometry(const vpt_scene_edit& e) { return e.num_instances > 0 || e.num_shapes > 0; }
static bool moves_geometry(const vpt_subdiv_edit& e) { return e.num > 0; }
static bool writes_materials(const vpt_scene_edit& e) { return e.num_materials > 0; }
template <typename Edit> static bool moves_geometry(const Edit&) { return false; }   // environments, textures, volumes, SDFs
template <typename Edit> static bool writes_materials(const Edit&) { return false; }

// One edit, from the idle device it needs to what the render side owes it afterwards.  apply(resident&, edit, edit_outcome&): the
// unit's work (vpt_resident.h says what it reports).
template <typename Edit, typename Apply>
static int edit_scene(vpt_scene* s, const Edit* edit, Apply apply) {
  if (!s || !edit) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipDeviceSynchronize());   // launches on any stream may still read the tables this call rewrites or replaces
  edit_outcome out = {false, false, false, s->stack_cap, s->stack_lds4, s->stack_spill4, s->curves};
  if (int rc = apply(*s, *edit, out)) return rc;
  if (!out.changed) return VPT_OK;   // an empty request: the schedule and the counters of the last edit stay
  if (out.topology) {   // new trees or lists: the stack sizes and the kernel instances follow
    if (out.stack_spill4 != s->stack_spill4) s->spill_lanes = 0;   // the HBM part is sized per entry: made anew by the next launch
    s->stack_cap = out.stack_cap, s->stack_lds4 = out.stack_lds4, s->stack_spill4 = out.stack_spill4;
    s->curves = out.curves;
  }
  // light_prims hold world-space normals of the moved lights, name instances and read the leaf records through the shape table
  if (out.lights_rebuilt || out.topology || moves_geometry(*edit))
    if (int rc = light_setup(s)) return rc;
  if (out.lights_rebuilt || writes_materials(*edit))   // the medium records follow the materials and sit behind the light records
    if (int rc = medium_setup(s)) return rc;
  s->sched.forget();   // the camera index may be the same, the picture is not
  return VPT_OK;
}

extern "C" {

int vpt_scene_update(vpt_scene* s, const vpt_scene_edit* edit) {
  return edit_scene(s, edit, [](resident& r, const vpt_scene_edit& e, edit_outcome& out) { return scene_update_apply(r, e, out); });
}
// the two refusals about lights are lifted and the light tables follow the edit
int vpt_scene_update_lights(vpt_scene* s, const vpt_scene_edit* edit) {
  return edit_scene(s, edit, [](resident& r, const vpt_scene_edit& e, edit_outcome& out) {
    const int rc = scene_update_apply(r, e, out, true);
    return rc ? rc : light_update_apply(r, e, &out.lights_rebuilt);
  });
}
// the light tables follow when an environment's light does / when the SDF lights do
int vpt_scene_update_textures(vpt_scene* s, const vpt_texture_edit* edit) { return edit_scene(s, edit, texture_update_apply); }
int vpt_scene_update_volumes(vpt_scene* s, const vpt_volume_edit* edit) { return edit_scene(s, edit, volume_update_apply); }
// voxels alone, from analytic brushes evaluated where they live (vpt_sculpt.hip)
int vpt_scene_sculpt_volumes(vpt_scene* s, const vpt_sculpt_edit* edit) { return edit_scene(s, edit, sculpt_apply); }
// the BVHs built anew (vpt_bvh_rebuild.hip), the set of instances changed (vpt_instance_update.hip), the shape list changed (vpt_shape_update.hip)
int vpt_scene_rebuild_bvh(vpt_scene* s, const vpt_bvh_rebuild* what) { return vpt_scene_rebuild_bvh_quality(s, what, VPT_BVH_MIDDLE); }
int vpt_scene_rebuild_bvh_quality(vpt_scene* s, const vpt_bvh_rebuild* what, int quality) {
  return edit_scene(s, what, [quality](resident& r, const vpt_bvh_rebuild& w, edit_outcome& out) { return bvh_rebuild_apply(r, w, out, quality); });
}
int vpt_scene_update_instances(vpt_scene* s, const vpt_instance_edit* edit) { return edit_scene(s, edit, instance_update_apply); }
int vpt_scene_update_shapes(vpt_scene* s, const vpt_shape_edit* edit) { return edit_scene(s, edit, shape_update_apply); }
// the subdivision surfaces (vpt_subdiv_update.hip): a plan attached or freed changes no table of the scene - the render side owes it nothing
int vpt_scene_attach_subdiv(vpt_scene* s, const vpt_subdiv_plan* plan, int* subdiv_id_out) {
  if (!s || !plan) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  return subdiv_attach(*s, *plan, subdiv_id_out);
}
int vpt_scene_detach_subdiv(vpt_scene* s, int subdiv_id) {
  if (!s) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipDeviceSynchronize());   // nothing reads the plan's tables when they go
  return subdiv_detach(*s, subdiv_id);
}
int vpt_scene_subdiv_count(const vpt_scene* s) {
  if (!s) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  int n = 0;
  for (const subdiv_plan_dev& p : s->subdivs) n += p.shape >= 0;
  return n;
}
int vpt_scene_subdiv_shape(const vpt_scene* s, int subdiv_id) { return s && subdiv_id >= 0 && subdiv_id < (int)s->subdivs.size() ? s->subdivs[(size_t)subdiv_id].shape : -1; }
int vpt_scene_update_subdivs(vpt_scene* s, const vpt_subdiv_edit* edit) { return edit_scene(s, edit, subdiv_update_apply); }

int vpt_last_wave_costs(vpt_scene* s, unsigned* ticks, int capacity, int* count) {
  if (!s || !count || capacity < 0 || (capacity > 0 && !ticks)) return vpt_set_error(VPT_ERR_INVALID_ARG, "bad argument");
  if (!s->timed) return vpt_set_error(VPT_ERR_INVALID_ARG, "no launch recorded");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipEventSynchronize(s->ev1));
  return s->sched.last_wave_costs(ticks, capacity, count);
}

// synchronous: waves of the implicit kernel that hit their watchdog since the scene was created (a defect, never a workload)
int vpt_check_watchdog(vpt_scene* s) {
  if (!s) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  unsigned n = 0;
  HIP_TRY(hipMemcpy(&n, s->d_watchdog.get(), 4, hipMemcpyDeviceToHost));
  if (n) return vpt_set_error(VPT_ERR_HIP, "%u wave(s) of the implicit kernel gave up after their watchdog time: the result is incomplete", n);
  return VPT_OK;
}

int vpt_last_kernel_ms(vpt_scene* s, float* ms) {
  if (!s || !ms) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  if (!s->timed) return vpt_set_error(VPT_ERR_INVALID_ARG, "no launch recorded");
  HIP_TRY(hipEventSynchronize(s->ev1));
  HIP_TRY(hipEventElapsedTime(ms, s->ev0, s->ev1));
  float pause = 0;
  if (int rc = s->sched.paused_ms(&pause)) return rc;
  *ms -= pause;
  return vpt_check_watchdog(s);
}

int vpt_resolve_device(const vpt_layout* layout, const void* d_tiles_all_ranks, int samples, void* d_image_rowmajor, void* stream) {
  return resolve(vpt_resolve_kernel, layout, d_tiles_all_ranks, samples, (float4*)d_image_rowmajor, stream);
}

int vpt_resolve_srgb8_device(const vpt_layout* layout, const void* d_tiles_all_ranks, int samples, void* d_rgba8_rowmajor, void* stream) {
  return resolve(vpt_resolve_srgb8_kernel, layout, d_tiles_all_ranks, samples, (uchar4*)d_rgba8_rowmajor, stream);
}

}  // extern "C"

// the conditions on the planes of a first-hit pass (include/vpt.h), device or host pointers alike
static int check_given(const vpt_aov_planes* p) {
  REQUIRE(p, "null planes");
  const void* const        given[6] = {p->normal, p->albedo, p->texcoord, p->depth, p->ids, p->uvt};
  static const char* const name[6]  = {"normal", "albedo", "texcoord", "depth", "ids", "uvt"};
  return check_plane_set(name, given, 6, 4, 5);
}
static aov_planes device_planes(const vpt_aov_planes& p) {
  return {(float4*)p.normal, (float4*)p.albedo, (float4*)p.texcoord, (float4*)p.depth, (int2*)p.ids, (float*)p.uvt};
}

extern "C" {

int vpt_render_aov_device(vpt_scene* s, const vpt_params* params, const vpt_layout* layout, int nsamples, const vpt_aov_planes* planes,
    void* d_hits, void* d_rng, void* stream) {
  if (int rc = check_given(planes)) return rc;
  REQUIRE(s && params && layout && d_hits && d_rng, "null argument");
  REQUIRE(params->camera >= 0 && params->camera < s->d.num_cameras, "camera %d out of range", params->camera);
  REQUIRE(nsamples >= 0, "negative sample count");
  if (nsamples == 0) return VPT_OK;
  DParams pr;
  if (int rc = make_dparams(params, layout, nsamples, pr)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const dim3 grid((pr.nslots + VPT_BLOCK - 1) / VPT_BLOCK);
  stack_cfg  stack;
  if (int rc = stack_config(s, (long long)grid.x * VPT_BLOCK, stack)) return rc;
  const size_t lds = (size_t)s->stack_lds4 * 2 * VPT_BLOCK * sizeof(int);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(VPT_BLOCK), lds, (hipStream_t)stream, s->d, pr, device_planes(*planes), (int*)d_hits, (ulonglong2*)d_rng, stack);
  };
  if (s->curves) {
    if (stack.spill) launch(vpt_aov_kernel<true, true>);
    else launch(vpt_aov_kernel<false, true>);
  } else if (stack.spill) launch(vpt_aov_kernel<true, false>);
  else launch(vpt_aov_kernel<false, false>);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

int vpt_resolve_ids_device(const vpt_layout* layout, const void* d_ids, const void* d_uvt, void* d_ids_rowmajor, void* d_uvt_rowmajor, void* stream) {
  REQUIRE(layout && d_ids && d_ids_rowmajor, "null argument");
  REQUIRE((d_uvt != nullptr) == (d_uvt_rowmajor != nullptr), "d_uvt and d_uvt_rowmajor must be null together");
  const layout_plane planes[2] = {{(void*)d_ids, d_ids_rowmajor, 8}, {(void*)d_uvt, d_uvt_rowmajor, 12}};
  return layout_copy(layout, LAYOUT_ALL_TILES_TO_ROWS, planes, d_uvt ? 2 : 1, (hipStream_t)stream);
}

int vpt_render_aov(vpt_scene* s, const vpt_params* params, int nsamples, int width, int height, const vpt_aov_planes* planes, int32_t* hits,
    uint64_t* rng, int* samples_io) {
  if (int rc = check_given(planes)) return rc;
  REQUIRE(params, "null params");
  REQUIRE(hits, "null hits");
  REQUIRE(rng, "null rng");
  REQUIRE(samples_io, "null samples_io");
  REQUIRE(width >= 1 && height >= 1 && width < 32768 && height < 32768, "bad image size: width %d, height %d", width, height);
  REQUIRE(nsamples >= 0, "nsamples %d is negative", nsamples);
  REQUIRE(s, "null scene");
  REQUIRE(params->camera >= 0 && params->camera < s->d.num_cameras, "camera %d out of range", params->camera);
  const int todo = std::min(nsamples, params->samples - *samples_io);   // no-op once reached, as vpt_render
  if (todo <= 0) return VPT_OK;
  HIP_TRY(hipSetDevice(s->device));
  const vpt_layout lay      = {width, height, 8, 8, 0, 1};
  const host_plane parts[8] = {{planes->normal, 16}, {planes->albedo, 16}, {planes->texcoord, 16}, {planes->depth, 16}, {planes->ids, 8},
      {planes->uvt, 12}, {hits, 4}, {rng, 16}};
  if (int rc = layout_round_trip(lay, parts, 8, nullptr, [&](const vpt_layout* l, void* const* t) {
        const vpt_aov_planes tiles = {t[0], t[1], t[2], t[3], t[4], t[5]};
        return vpt_render_aov_device(s, params, l, todo, &tiles, t[6], t[7], nullptr);
      }))
    return rc;
  *samples_io += todo;
  return VPT_OK;
}

}  // extern "C"

// vpt_render / vpt_render_adaptive: the host state through the scene handle's staging (one rank, 8x8 tiles) and render(layout, tiles)
template <typename Render>
static int render_staged(vpt_scene* s, int width, int height, float* image_rgba, int32_t* hits, uint64_t* rng, Render&& render) {
  HIP_TRY(hipSetDevice(s->device));
  const vpt_layout lay      = {width, height, 8, 8, 0, 1};
  const host_plane state[3] = {{image_rgba, 16}, {hits, 4}, {rng, 16}};
  if (int rc = layout_round_trip(lay, state, 3, &s->staging, render)) return rc;
  return vpt_check_watchdog(s);
}

// vpt_adaptive_run (include/vpt.h): what the round loop of an adaptive render holds between rounds
struct vpt_adaptive_run {
  vpt_scene*       s = nullptr;
  vpt_params       params = {};
  vpt_adaptive     a = {};
  DParams          pr = {};
  hipStream_t      st = nullptr;
  float4*          img = nullptr;
  int*             hit = nullptr;
  ulonglong2*      rng = nullptr;
  bool             implicit = false;
  device_buffer    d_stats, d_wave_count, d_lane_slot, d_info;   // vpt_adaptive.h, sized for the full layout
  adaptive_buffers b = {};
  int              info[4] = {0, 0, 0, 0};   // the last read-back: {pixels still rendering, min hits, max hits on entry, unused}
  int              h = 0, n = 0;             // hits of every pixel still rendering, rounds so far
  long long        taken = 0;                // samples so far
  bool             timing_open = false;      // ev0 was recorded by create and no round has run since
  int read_info() {   // the one read-back of a round: what sizes the next launch
    HIP_TRY(hipMemcpyAsync(info, b.info, sizeof(info), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return VPT_OK;
  }
};

// the arguments of an adaptive render, checked before anything touches the device
static int check_adaptive(const vpt_scene* s, const vpt_params* params, const vpt_adaptive* a) {
  if (!params || !a) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  if (!std::isfinite(a->threshold) || a->threshold < 0) return vpt_set_error(VPT_ERR_INVALID_ARG, "adaptive threshold must be finite and >= 0");
  if (a->step < 1) return vpt_set_error(VPT_ERR_INVALID_ARG, "adaptive step must be >= 1");
  if (params->samples < 1) return vpt_set_error(VPT_ERR_INVALID_ARG, "params->samples (the per-pixel cap) must be >= 1");
  if (a->min_samples < 1 || a->min_samples > params->samples)
    return vpt_set_error(VPT_ERR_INVALID_ARG, "adaptive min_samples must be in 1 .. params->samples (%d)", params->samples);
  if (params->bounces < 0) return vpt_set_error(VPT_ERR_INVALID_ARG, "negative bounce count");
  if (!s) return vpt_set_error(VPT_ERR_INVALID_ARG, "null scene");
  if (params->shader < 0 || params->shader > VPT_SHADER_IMPLICIT_NORMAL) return vpt_set_error(VPT_ERR_UNKNOWN_SHADER, "sampler unknown");
  if (params->camera < 0 || params->camera >= s->d.num_cameras) return vpt_set_error(VPT_ERR_INVALID_ARG, "camera %d out of range", params->camera);
  return VPT_OK;
}

extern "C" {

// Adaptive sampling (include/vpt.h): rounds of one launch each over the pixels still rendering, packed 64 to a
// wave through sched_cfg::lane_slot by the kernels of vpt_adaptive.hip.  No pilot, no order, no costs, no tile splitting: the handle's
// launch schedule for the layout stays as vpt_render_device left it.  A run holds what the round loop holds, so that the loop can
// stop after any round and go on in a later call.
int vpt_adaptive_run_create(vpt_scene* s, const vpt_params* params, const vpt_adaptive* a, const vpt_layout* layout, void* d_image,
    void* d_hits, void* d_rng, void* stream, vpt_adaptive_run** out) {
  if (!out) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (int rc = check_adaptive(s, params, a)) return rc;
  if (!layout || !d_image || !d_hits || !d_rng) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  std::unique_ptr<vpt_adaptive_run> r(new vpt_adaptive_run{});
  if (int rc = make_dparams(params, layout, 0, r->pr)) return rc;
  r->s = s, r->params = *params, r->a = *a, r->st = (hipStream_t)stream;
  r->img = (float4*)d_image, r->hit = (int*)d_hits, r->rng = (ulonglong2*)d_rng;
  r->implicit = params->shader >= VPT_SHADER_IMPLICIT;
  if (r->implicit)
    if (int rc = implicit_lds(s)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  const DParams&  pr   = r->pr;
  const long long full = (pr.nslots + VPT_BLOCK - 1) / VPT_BLOCK;
  stack_cfg stack;   // the spilled stacks are indexed by global lane: sized for the full layout, a compacted grid is never larger
  if (int rc = stack_config(s, full * VPT_BLOCK, stack)) return rc;
  if (int rc = r->d_stats.allocate((size_t)pr.nslots * 16)) return rc;
  if (int rc = r->d_wave_count.allocate((size_t)full * 4)) return rc;
  if (int rc = r->d_lane_slot.allocate((size_t)pr.nslots * 4)) return rc;
  if (int rc = r->d_info.allocate(16)) return rc;
  r->b = {r->d_stats.get<float4>(), r->d_wave_count.get<int>(), r->d_lane_slot.get<int>(), r->d_info.get<int>()};
  HIP_TRY(hipEventRecord(s->ev0, r->st));
  s->sched.no_pause();
  if (int rc = adaptive_update(pr, r->img, r->hit, r->b, 0, 0, r->a, params->samples, r->st)) return rc;
  if (int rc = r->read_info()) return rc;
  if (r->info[1] < r->info[2])
    return vpt_set_error(VPT_ERR_INVALID_ARG, "hits[] must be equal on entry (found %d .. %d)", r->info[1], r->info[2]);
  r->h = r->info[1], r->timing_open = true;
  *out = r.release();
  return VPT_OK;
}

int vpt_adaptive_run_rounds(vpt_adaptive_run* r, int max_rounds, int* rounds_done, int64_t* rendered, int* active) {
  if (rounds_done) *rounds_done = 0;
  if (rendered) *rendered = 0;
  if (active) *active = 0;
  if (!r) return vpt_set_error(VPT_ERR_INVALID_ARG, "null run");
  if (max_rounds < 0) return vpt_set_error(VPT_ERR_INVALID_ARG, "negative round count");
  vpt_scene* s   = r->s;
  const int  cap = r->params.samples;
  if (active) *active = r->info[0];
  if (max_rounds == 0 || r->info[0] <= 0 || r->h >= cap) return VPT_OK;   // nothing is enqueued
  HIP_TRY(hipSetDevice(s->device));
  const DParams& pr = r->pr;
  stack_cfg      stack;   // taken per call: a larger launch on the handle in between may have moved the spilled stacks
  if (int rc = stack_config(s, (long long)((pr.nslots + VPT_BLOCK - 1) / VPT_BLOCK) * VPT_BLOCK, stack)) return rc;
  const launch_ctx L = {s, r->st, r->img, r->hit, r->rng, stack};
  if (!r->timing_open) {   // the first call's timing starts where the run was created; a later call's at its own first round
    HIP_TRY(hipEventRecord(s->ev0, r->st));
    s->sched.no_pause();
  }
  r->timing_open = false;
  int       done  = 0;
  long long taken = 0;
  for (int act = r->info[0]; done < max_rounds && act > 0 && r->h < cap; act = r->info[0]) {
    DParams rp  = pr;
    rp.nsamples = std::min(r->a.step, cap - r->h);
    const sched_cfg sch = {nullptr, nullptr, r->b.lane_slot};
    launcher_of(r->params.shader)(L, false, dim3((unsigned)((act + VPT_BLOCK - 1) / VPT_BLOCK)), rp, sch);
    HIP_TRY(hipGetLastError());
    taken += (long long)act * rp.nsamples, r->h += rp.nsamples, r->n++, done++;
    if (int rc = adaptive_update(pr, r->img, r->hit, r->b, r->n, rp.nsamples, r->a, cap, r->st)) return rc;
    if (int rc = r->read_info()) return rc;
    if (r->implicit)
      if (int rc = vpt_check_watchdog(s)) return rc;
  }
  HIP_TRY(hipEventRecord(s->ev1, r->st));
  s->timed = true;
  r->taken += taken;
  if (rounds_done) *rounds_done = done;
  if (rendered) *rendered = taken;
  if (active) *active = r->info[0];
  return VPT_OK;
}

int vpt_adaptive_run_progress(const vpt_adaptive_run* r, int* rounds, int64_t* rendered, int* active, int* max_hits) {
  if (!r) return vpt_set_error(VPT_ERR_INVALID_ARG, "null run");
  if (rounds) *rounds = r->n;
  if (rendered) *rendered = r->taken;
  if (active) *active = r->h >= r->params.samples ? 0 : r->info[0];
  if (max_hits) *max_hits = r->h;
  return VPT_OK;
}

int vpt_adaptive_run_noise_device(vpt_adaptive_run* r, void* d_se2_rowmajor, void* d_hits_rowmajor, void* stream) {
  if (!r || !d_se2_rowmajor) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  HIP_TRY(hipSetDevice(r->s->device));
  return adaptive_noise(r->pr, r->b, r->hit, r->a.step, (float*)d_se2_rowmajor, (int*)d_hits_rowmajor, nullptr, nullptr, (hipStream_t)stream);
}

int vpt_adaptive_run_stats_device(vpt_adaptive_run* r, void* d_mean_rowmajor, void* d_m2_rowmajor, void* stream) {
  if (!r || !d_mean_rowmajor || !d_m2_rowmajor) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  HIP_TRY(hipSetDevice(r->s->device));
  return adaptive_noise(r->pr, r->b, r->hit, r->a.step, nullptr, nullptr, (float*)d_mean_rowmajor, (float*)d_m2_rowmajor, (hipStream_t)stream);
}

void vpt_adaptive_run_destroy(vpt_adaptive_run* r) {
  if (!r) return;
  (void)hipSetDevice(r->s->device);
  (void)hipStreamSynchronize(r->st);   // nothing reads the scratch when it goes
  delete r;
}

int vpt_render_device_adaptive(vpt_scene* s, const vpt_params* params, const vpt_adaptive* a, const vpt_layout* layout, void* d_image,
    void* d_hits, void* d_rng, void* stream, int* rounds, int64_t* rendered) {
  if (rounds) *rounds = 0;
  if (rendered) *rendered = 0;
  vpt_adaptive_run* r = nullptr;
  if (int rc = vpt_adaptive_run_create(s, params, a, layout, d_image, d_hits, d_rng, stream, &r)) return rc;
  struct guard { vpt_adaptive_run* r; ~guard() { vpt_adaptive_run_destroy(r); } } g{r};
  int     n     = 0;
  int64_t taken = 0;
  if (int rc = vpt_adaptive_run_rounds(r, INT_MAX, &n, &taken, nullptr)) return rc;
  if (n == 0) {   // nothing to render: the call's timing still closes, as it always has
    HIP_TRY(hipEventRecord(s->ev1, (hipStream_t)stream));
    s->timed = true;
  }
  if (rounds) *rounds = n;
  if (rendered) *rendered = taken;
  return VPT_OK;
}

int vpt_render_adaptive(vpt_scene* s, const vpt_params* params, const vpt_adaptive* a, int width, int height, float* image_rgba,
    int32_t* hits, uint64_t* rng, int* samples_io, int64_t* rendered) {
  if (rendered) *rendered = 0;
  if (int rc = check_adaptive(s, params, a)) return rc;
  if (!image_rgba || !hits || !rng || !samples_io) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  if (width <= 0 || height <= 0) return vpt_set_error(VPT_ERR_INVALID_ARG, "bad image size");
  const long long pixels = (long long)width * height;
  for (long long i = 1; i < pixels; i++)
    if (hits[i] != hits[0]) return vpt_set_error(VPT_ERR_INVALID_ARG, "hits[] must be equal on entry (pixel %lld has %d, pixel 0 %d)", i, hits[i], hits[0]);
  *samples_io = hits[0];
  if (hits[0] >= params->samples) return VPT_OK;
  if (int rc = render_staged(s, width, height, image_rgba, hits, rng, [&](const vpt_layout* lay, void* const* t) {
        return vpt_render_device_adaptive(s, params, a, lay, t[0], t[1], t[2], nullptr, nullptr, rendered);
      }))
    return rc;
  *samples_io = *std::max_element(hits, hits + pixels);
  return VPT_OK;
}

int vpt_render(vpt_scene* s, const vpt_params* params, int nsamples, int width, int height, float* image_rgba,
    int32_t* hits, uint64_t* rng, int* samples_io) {
  if (!s || !params || !image_rgba || !hits || !rng || !samples_io) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  if (width <= 0 || height <= 0) return vpt_set_error(VPT_ERR_INVALID_ARG, "bad image size");
  if (params->shader < 0 || params->shader > VPT_SHADER_IMPLICIT_NORMAL) return vpt_set_error(VPT_ERR_UNKNOWN_SHADER, "sampler unknown");
  int todo = params->samples - *samples_io;   // no-op once reached, yocto_pathtrace.cpp:1055
  if (nsamples < todo) todo = nsamples;
  if (todo <= 0) return VPT_OK;
  if (int rc = render_staged(s, width, height, image_rgba, hits, rng, [&](const vpt_layout* lay, void* const* t) {
        return vpt_render_device(s, params, lay, todo, t[0], t[1], t[2], nullptr);
      }))
    return rc;
  *samples_io += todo;
  return VPT_OK;
}

int vpt_selftest_reciprocal(int device, unsigned long long* mismatches, unsigned long long* fallbacks) {
  if (!mismatches || !fallbacks) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  HIP_TRY(hipSetDevice(device));
  device_buffer d;
  if (int rc = d.allocate(16)) return rc;
  HIP_TRY(hipMemset(d.get(), 0, 16));
  hipLaunchKernelGGL(vpt_reciprocal_selftest_kernel, dim3(4096), dim3(256), 0, 0, d.get<unsigned long long>());
  unsigned long long h[2] = {0, 0};
  int rc = hipMemcpy(h, d.get(), 16, hipMemcpyDeviceToHost) == hipSuccess ? VPT_OK : vpt_set_error(VPT_ERR_HIP, "reciprocal self-test failed to run");
  *mismatches = h[0], *fallbacks = h[1];
  return rc;
}

int vpt_intersect(vpt_scene* s, int n, const float* rays, int instance, int32_t* ids, float* uvt) {
  if (!s || !rays || !ids || !uvt || n < 0) return vpt_set_error(VPT_ERR_INVALID_ARG, "bad argument");
  if (instance < -1 || instance >= s->d.num_instances) return vpt_set_error(VPT_ERR_INVALID_ARG, "instance %d out of range", instance);
  if (instance >= 0 && s->h.slot_of[(size_t)instance] < 0) return vpt_set_error(VPT_ERR_INVALID_ARG, "instance %d is not in the scene BVH", instance);
  if (n == 0) return VPT_OK;
  HIP_TRY(hipSetDevice(s->device));
  device_buffer d_rays, d_ids, d_uvt;
  if (d_rays.allocate((size_t)n * 24) || d_ids.allocate((size_t)n * 8) || d_uvt.allocate((size_t)n * 12) ||
      hipMemcpy(d_rays.get(), rays, (size_t)n * 24, hipMemcpyHostToDevice) != hipSuccess)
    return vpt_set_error(VPT_ERR_HIP, "vpt_intersect: device buffers");
  int       blocks = (n + VPT_BLOCK - 1) / VPT_BLOCK;
  stack_cfg stack;
  if (int rc = stack_config(s, (long long)blocks * VPT_BLOCK, stack)) return rc;
  size_t lds = (size_t)s->stack_lds4 * 2 * VPT_BLOCK * sizeof(int);
  auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(blocks), dim3(VPT_BLOCK), lds, 0, s->d, n, d_rays.get<const float>(), instance, d_ids.get<int>(), d_uvt.get<float>(), stack); };
  if (s->curves) {   // points or lines: the leaf tests of the VPT_FEAT_CURVES instances
    if (stack.spill) launch(vpt_intersect_curves_kernel<true>);
    else launch(vpt_intersect_curves_kernel<false>);
  } else if (s->d.tri_prims) {   // a scene of triangles: through the short leaf records, as its path tracers go
    if (stack.spill) launch(vpt_intersect_kernel<true, true>);
    else launch(vpt_intersect_kernel<false, true>);
  } else if (stack.spill) launch(vpt_intersect_kernel<true, false>);
  else launch(vpt_intersect_kernel<false, false>);
  bool ok = hipMemcpy(ids, d_ids.get(), (size_t)n * 8, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(uvt, d_uvt.get(), (size_t)n * 12, hipMemcpyDeviceToHost) == hipSuccess;
  return ok ? VPT_OK : vpt_set_error(VPT_ERR_HIP, "vpt_intersect failed to run");
}

// ---- known-answer-test entry points (include/vpt_kat.h) ------------------------------------------------------------
static const int k_kat_strides[VPT_KAT_OP_COUNT][2] = {{19, 22}, {15, 10}, {4, 4}, {5, 6}, {7, 5}, {7, 24}, {3, 3}, {7, 3}, {6, 1},
    {6, 1}, {4, 3}, {6, 3}, {7, 4}, {4, 1}, {4, 1}};

int vpt_kat_strides(int op, int* in_stride, int* out_stride) {
  if (op < 0 || op >= VPT_KAT_OP_COUNT || !in_stride || !out_stride) return vpt_set_error(VPT_ERR_INVALID_ARG, "unknown KAT op %d", op);
  *in_stride = k_kat_strides[op][0], *out_stride = k_kat_strides[op][1];
  return VPT_OK;
}

int vpt_kat(vpt_scene* s, int op, int iparam, int n, const float* in, float* out) {
  if (!s || n < 0 || (n > 0 && (!in || !out))) return vpt_set_error(VPT_ERR_INVALID_ARG, "bad argument");
  if (op < 0 || op >= VPT_KAT_OP_COUNT) return vpt_set_error(VPT_ERR_INVALID_ARG, "unknown KAT op %d", op);
  if (n == 0) return VPT_OK;
  const int si = k_kat_strides[op][0], so = k_kat_strides[op][1];
  const DScene& D = s->d;
  // every id a record carries is checked here, so that no batch can index outside the scene's tables
  std::vector<int> aux((size_t)n, 0);
  auto id_ok = [](float v, int count) { return v >= 0 && v < (float)count && v == (float)(int)v; };
  for (int i = 0; i < n; i++) {
    const float* a = in + (size_t)i * si;
    bool ok = true;
    switch (op) {
      case VPT_KAT_LOBES: ok = id_ok(a[0], VPT_MAT_GLTFPBR + 1); break;
      case VPT_KAT_TEXTURE: ok = id_ok(a[0], D.num_textures); break;
      case VPT_KAT_CAMERA: ok = id_ok(a[0], D.num_cameras); break;
      case VPT_KAT_INTERSECT: ok = a[6] == -1.0f || (id_ok(a[6], D.num_instances) && s->h.slot_of[(size_t)a[6]] >= 0); break;
      case VPT_KAT_SURFACE:
        ok = id_ok(a[0], D.num_instances) && id_ok(a[1], s->h.shape_elems[(size_t)s->h.inst_shape[(size_t)a[0]]]);
        if (ok) aux[(size_t)i] = s->h.prim_slot[(size_t)s->h.shape_elem_offset[(size_t)s->h.inst_shape[(size_t)a[0]]] + (size_t)a[1]];
        break;
      case VPT_KAT_SAMPLE_LIGHTS:
      case VPT_KAT_LIGHTS_PDF:
      case VPT_KAT_LIGHTS_PDF_K2: ok = D.num_lights > 0; break;
      case VPT_KAT_SDF_NORMAL: ok = a[0] == 0.0f ? id_ok(a[1], D.num_vol_instances) : (a[0] == 1.0f && id_ok(a[1], D.num_sdfs)); break;
      case VPT_KAT_SPHERETRACE: ok = a[6] == -1.0f || id_ok(a[6], D.num_sdfs); break;
      case VPT_KAT_VOLUME: ok = id_ok(a[0], D.num_volumes); break;
      case VPT_KAT_SDF_FUNCTION: ok = id_ok(a[0], D.num_sdfs); break;
      default: break;
    }
    if (!ok) return vpt_set_error(VPT_ERR_INVALID_ARG, "KAT op %d record %d: id out of range", op, i);
  }
  if ((op == VPT_KAT_LIGHTS_PDF || op == VPT_KAT_LIGHTS_PDF_K2 || op == VPT_KAT_SPHERETRACE) && (iparam < 0 || iparam > (1 << 20)))
    return vpt_set_error(VPT_ERR_INVALID_ARG, "KAT op %d: iteration limit %d out of range", op, iparam);
  HIP_TRY(hipSetDevice(s->device));
  device_buffer d_in, d_out, d_aux;
  if (d_in.allocate((size_t)n * si * 4) || d_out.allocate((size_t)n * so * 4) || d_aux.allocate((size_t)n * 4) ||
      hipMemcpy(d_in.get(), in, (size_t)n * si * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_aux.get(), aux.data(), (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess)
    return vpt_set_error(VPT_ERR_HIP, "vpt_kat: device buffers");
  int       blocks = (n + VPT_BLOCK - 1) / VPT_BLOCK;
  stack_cfg stack;
  if (int rc = stack_config(s, (long long)blocks * VPT_BLOCK, stack)) return rc;
  size_t lds4 = (size_t)s->stack_lds4 * 2 * VPT_BLOCK * sizeof(int), lds2 = (size_t)s->stack_cap * VPT_BLOCK * sizeof(int);
  size_t lds  = lds4 > lds2 ? lds4 : lds2;
  if (stack.spill) hipLaunchKernelGGL(vpt_kat_kernel<true>, dim3(blocks), dim3(VPT_BLOCK), lds, 0, s->d, op, iparam, n, si, so, d_in.get<const float>(), d_aux.get<const int>(), d_out.get<float>(), stack, s->stack_cap);
  else hipLaunchKernelGGL(vpt_kat_kernel<false>, dim3(blocks), dim3(VPT_BLOCK), lds, 0, s->d, op, iparam, n, si, so, d_in.get<const float>(), d_aux.get<const int>(), d_out.get<float>(), stack, s->stack_cap);
  bool ok = hipGetLastError() == hipSuccess && hipMemcpy(out, d_out.get(), (size_t)n * so * 4, hipMemcpyDeviceToHost) == hipSuccess;
  return ok ? VPT_OK : vpt_set_error(VPT_ERR_HIP, "vpt_kat failed to run");
}

int vpt_spheretrace(vpt_scene* s, int n, const float* rays, int sdf, int maxiter, int32_t* ids, float* t) {
  if (!s || n < 0 || (n > 0 && (!rays || !ids || !t))) return vpt_set_error(VPT_ERR_INVALID_ARG, "bad argument");
  std::vector<float> in((size_t)n * 7), out((size_t)n * 4);
  for (int i = 0; i < n; i++) {
    memcpy(&in[(size_t)i * 7], rays + (size_t)i * 6, 24);
    in[(size_t)i * 7 + 6] = (float)(sdf < 0 ? -1 : sdf);
  }
  if (int rc = vpt_kat(s, VPT_KAT_SPHERETRACE, maxiter, n, in.data(), out.data())) return rc;
  for (int i = 0; i < n; i++) {
    ids[3 * (size_t)i] = (int)out[4 * (size_t)i], ids[3 * (size_t)i + 1] = (int)out[4 * (size_t)i + 2], ids[3 * (size_t)i + 2] = (int)out[4 * (size_t)i + 3];
    t[i] = out[4 * (size_t)i + 1];
  }
  return VPT_OK;
}

int vpt_eval_lobes(vpt_scene* s, int n, const float* in19, float* out22) { return vpt_kat(s, VPT_KAT_LOBES, 0, n, in19, out22); }

int vpt_selftest_light_cdf(vpt_scene* s, int light, int n, unsigned long long* mismatches, int* indexed) {
  if (!s || !mismatches || !indexed || n <= 0) return vpt_set_error(VPT_ERR_INVALID_ARG, "bad argument");
  if (light < 0 || light >= s->d.num_lights) return vpt_set_error(VPT_ERR_INVALID_ARG, "light %d out of range", light);
  HIP_TRY(hipSetDevice(s->device));
  DCdfIndex ix;
  HIP_TRY(hipMemcpy(&ix, s->d.light_index + light, sizeof(ix), hipMemcpyDeviceToHost));
  *indexed = ix.levels > 0 ? (ix.guide_buckets > 0 ? 2 : 1) : 0, *mismatches = 0;
  if (!ix.levels) return VPT_OK;   // short CDFs use the reference's binary search itself
  device_buffer d;
  if (int rc = d.allocate(8)) return rc;
  HIP_TRY(hipMemset(d.get(), 0, 8));
  hipLaunchKernelGGL(vpt_light_cdf_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, s->d, light, n, d.get<unsigned long long>());
  return hipMemcpy(mismatches, d.get(), 8, hipMemcpyDeviceToHost) == hipSuccess ? VPT_OK : vpt_set_error(VPT_ERR_HIP, "light CDF self-test failed to run");
}

}  // extern "C"
