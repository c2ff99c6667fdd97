// vpt_capi.hip — the scene handle of the C-ABI in include/vpt.h: the error text, creation (upload of the scene tables
// vpt_scene_prep.cpp builds: the device layout of vpt_device.h) and destruction, and the edit entry points, which forward to the
// update units and then tell the render side what it owes the edit.  It launches the two setup kernels of a scene's light and
// medium records (vpt_kernels.hip) and nothing else: rendering is vpt_render.hip's, adaptive sampling vpt_adaptive.hip's, the
// first-hit pass vpt_aov.hip's, the probes and self-tests vpt_probes.hip's.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared (see __graft_entry__.py).
// There is NO CPU fallback in this library: without a gfx950 device every compute entry point
// fails with VPT_ERR_NO_DEVICE.
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "vpt_bvh_rebuild.h"
#include "vpt_instance_update.h"
#include "vpt_light_update.h"
#include "vpt_scene_handle.h"
#include "vpt_scene_update.h"
#include "vpt_subdiv_update.h"
#include "vpt_shape_update.h"
#include "vpt_texture_update.h"
#include "vpt_sculpt.h"
#include "vpt_volume_set.h"
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
int vpt_shader_known(int id) { return (id >= 0 && id <= VPT_SHADER_IMPLICIT_NORMAL) || id == VPT_SHADER_VOLGRID; }

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
  REQUIRE(desc && out, "null argument");
  *out = nullptr;
  scene_tables t;   // every host-side refusal happens here, before any device call
  if (int rc = prepare_scene(*desc, curves, t)) return rc;
  int ndev = vpt_device_count();
  if (ndev <= 0) return vpt_set_error(VPT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
  REQUIRE(device >= 0 && device < ndev, "device %d out of range (%d devices)", device, ndev);
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

int vpt_scene_get_device(const vpt_scene* s) { REQUIRE(s, "null argument"); return s->device; }

int vpt_scene_record_bytes(const vpt_scene* s, int* leaf_bytes, int* attribute_bytes) {
  REQUIRE(s && leaf_bytes && attribute_bytes, "null argument");
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
static bool writes_voxels(const vpt_volume_edit&) { return true; }   // voxels in place, baked into the pool, or moved into a grown pool
static bool writes_voxels(const vpt_sculpt_edit&) { return true; }
static bool writes_voxels(const vpt_volume_set_edit&) { return true; }   // a pool laid out anew, volumes under other ids: the brick tables are indexed by volume
template <typename Edit> static bool writes_voxels(const Edit&) { return false; }

// One edit, from the idle device it needs to what the render side owes it afterwards.  apply(resident&, edit, edit_outcome&): the
// unit's work (vpt_resident.h says what it reports).
template <typename Edit, typename Apply>
static int edit_scene(vpt_scene* s, const Edit* edit, Apply apply) {
  REQUIRE(s && edit, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipDeviceSynchronize());   // launches on any stream may still read the tables this call rewrites or replaces
  edit_outcome out = {false, false, false, s->stack_cap, s->stack_lds4, s->stack_spill4, s->curves};
  if (int rc = apply(*s, *edit, out)) return rc;
  if (!out.changed) return VPT_OK;   // an empty request: the schedule and the counters of the last edit stay
  s->edit_generation++;                  // K3's tables (vpt_scene_handle.h: volgrid_tables) are made anew by the next volgrid launch
  if (writes_voxels(*edit)) s->voxel_generation++;
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
// volumes, grid instances and SDFs added and removed (vpt_volume_set.hip): the pool compacted by one gather, the lights following the SDFs
int vpt_scene_update_volume_set(vpt_scene* s, const vpt_volume_set_edit* edit) { return edit_scene(s, edit, volume_set_apply); }
// the BVHs built anew (vpt_bvh_rebuild.hip), the set of instances changed (vpt_instance_update.hip), the shape list changed (vpt_shape_update.hip)
int vpt_scene_rebuild_bvh(vpt_scene* s, const vpt_bvh_rebuild* what) { return vpt_scene_rebuild_bvh_quality(s, what, VPT_BVH_MIDDLE); }
int vpt_scene_rebuild_bvh_quality(vpt_scene* s, const vpt_bvh_rebuild* what, int quality) {
  return edit_scene(s, what, [quality](resident& r, const vpt_bvh_rebuild& w, edit_outcome& out) { return bvh_rebuild_apply(r, w, out, quality); });
}
int vpt_scene_update_instances(vpt_scene* s, const vpt_instance_edit* edit) { return edit_scene(s, edit, instance_update_apply); }
int vpt_scene_update_shapes(vpt_scene* s, const vpt_shape_edit* edit) { return edit_scene(s, edit, shape_update_apply); }
// the subdivision surfaces (vpt_subdiv_update.hip): a plan attached or freed changes no table of the scene - the render side owes it nothing
int vpt_scene_attach_subdiv(vpt_scene* s, const vpt_subdiv_plan* plan, int* subdiv_id_out) {
  REQUIRE(s && plan, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  return subdiv_attach(*s, *plan, subdiv_id_out);
}
int vpt_scene_detach_subdiv(vpt_scene* s, int subdiv_id) {
  REQUIRE(s, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipDeviceSynchronize());   // nothing reads the plan's tables when they go
  return subdiv_detach(*s, subdiv_id);
}
int vpt_scene_subdiv_count(const vpt_scene* s) {
  REQUIRE(s, "null argument");
  int n = 0;
  for (const subdiv_plan_dev& p : s->subdivs) n += p.shape >= 0;
  return n;
}
int vpt_scene_subdiv_shape(const vpt_scene* s, int subdiv_id) { return s && subdiv_id >= 0 && subdiv_id < (int)s->subdivs.size() ? s->subdivs[(size_t)subdiv_id].shape : -1; }
int vpt_scene_update_subdivs(vpt_scene* s, const vpt_subdiv_edit* edit) { return edit_scene(s, edit, subdiv_update_apply); }

}  // extern "C"
