// vpt_render.hip — the launch path of the C-ABI in include/vpt.h: vpt_render_device and vpt_render, the setup every traversal launch
// shares, the choice of a kernel instance for a scene, the two resolves, the read-backs of the last launch (time, wave costs, watchdog).
// Host code only: the kernels are declared in vpt_launch.h and compiled in the kernel units it lists; the launch schedule is
// vpt_schedule.hip's, the movement of a state between host arrays and tile-major slots vpt_layout.hip's.
#include <cstdlib>
#include "vpt_scene_handle.h"

int traversal_setup(vpt_scene* s, long long items, traversal_launch& out) {
  out.grid = dim3((unsigned)((items + VPT_BLOCK - 1) / VPT_BLOCK));
  out.lds  = (size_t)s->stack_lds4 * 2 * VPT_BLOCK * sizeof(int);
  const long long lanes = (long long)out.grid.x * VPT_BLOCK;
  if (s->stack_spill4 > 0 && lanes > s->spill_lanes) {   // the HBM part of the stacks: only scenes whose worst case exceeds the LDS part
    s->spill_lanes = 0;
    if (int rc = s->spill.allocate((size_t)lanes * (size_t)s->stack_spill4 * sizeof(int2))) return rc;
    s->spill_lanes = lanes;
  }
  out.stack = {s->stack_lds4, s->stack_spill4, s->spill.get<int2>(), lanes};
  return VPT_OK;
}

// K1 (mesh shaders): the instance compiled for the features this scene has (vpt_scene.hip.h: VPT_FEAT_*), launched over `grid`
// with the schedule `sch` - by launch_schedule::run (vpt_render_device) and by the rounds of an adaptive run (vpt_adaptive.hip)
template <int K>
static void launch_mesh_instance(const launch_ctx& L, bool is_pilot, dim3 grid, const DParams& pr, const sched_cfg& sch) {
  vpt_scene* s = L.s;
  const size_t lds = L.lds + 5 * VPT_BLOCK * sizeof(float);   // (ref, t0) pairs + the parked words
  // (the general instance also for a scene whose media vary over the surface: the others read a medium from its material's record;
  // VPT_MEDIUM_REGS=1, read per launch, sends any scene there - same bits: the tests' and the measurements' A/B switch)
  const int need = getenv("VPT_NO_LEAN") || getenv("VPT_MEDIUM_REGS") || s->varying_media ? VPT_FEAT_ALL : s->light_features;
  auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(VPT_BLOCK), lds, L.st, s->d, pr, L.img, L.hit, L.rng, L.stack, sch); };
  auto launch_feat = [&](auto feat) {
    constexpr int F = decltype(feat)::value;
    with_flags([&](auto spill) {
      if (is_pilot) launch(vpt_mesh_pilot_kernel<K, spill, F>);
      else launch(vpt_mesh_kernel<K, spill, F>);
    }, L.stack.spill);
  };
  // three instances: single-leaf mesh lights only / + emissive meshes with a BVH / everything (SDF lights too)
  // (+ the compact-record form of the first for the two path tracers on scenes of triangles; the pilot runs on the general records)
  // (a scene with points or lines: the one instance with every light feature and the point / line tests, vpt_k1_curves.hip)
  if (s->curves) launch_feat(std::integral_constant<int, VPT_FEAT_ALL | VPT_FEAT_CURVES>{});
  else if ((K == K_VOLPATH || K == K_PATH) && (need & (VPT_FEAT_LARGE_LIGHTS | VPT_FEAT_SDF_LIGHTS)) == 0 && s->d.tri_prims && !is_pilot) {
    if constexpr (K == K_VOLPATH || K == K_PATH)
      with_flags([&](auto spill) { launch(vpt_mesh_kernel<K, spill, VPT_FEAT_SMALL_LIGHTS | VPT_FEAT_COMPACT_TRIS>); }, L.stack.spill);
  } else if ((need & (VPT_FEAT_LARGE_LIGHTS | VPT_FEAT_SDF_LIGHTS)) == 0) launch_feat(std::integral_constant<int, VPT_FEAT_SMALL_LIGHTS>{});
  else if ((need & VPT_FEAT_SDF_LIGHTS) == 0) launch_feat(std::integral_constant<int, VPT_FEAT_SMALL_LIGHTS | VPT_FEAT_LARGE_LIGHTS>{});
  else launch_feat(std::integral_constant<int, VPT_FEAT_ALL>{});
}
int implicit_lds(const vpt_scene* s, size_t* bytes) {
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
// K3: one instance and its pilot; LDS holds the records of the grid instances (volgrid_prepare has checked that they fit)
static void launch_volgrid_instance(const launch_ctx& L, bool is_pilot, dim3 grid, const DParams& pr, const sched_cfg& sch) {
  const volgrid_args va  = volgrid_arguments(L.s);
  const size_t       lds = (size_t)va.num_instances * 128;
  if (is_pilot) hipLaunchKernelGGL(vpt_volgrid_kernel<true>, grid, dim3(VPT_BLOCK), lds, L.st, L.s->d, pr, va, L.img, L.hit, L.rng, sch);
  else hipLaunchKernelGGL(vpt_volgrid_kernel<false>, grid, dim3(VPT_BLOCK), lds, L.st, L.s->d, pr, va, L.img, L.hit, L.rng, sch);
}
instance_launcher launcher_of(int shader) {
  switch (shader) {
    case VPT_SHADER_VOLGRID: return launch_volgrid_instance;
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
  REQUIRE(layout && d_tiles_all_ranks && d_rowmajor && samples > 0, "bad argument");
  DParams pr;
  if (int rc = vpt_layout_dparams(layout, pr)) return rc;
  long long total = (long long)pr.nslots * pr.nranks;
  REQUIRE(total < (1LL << 31), "image too large");
  int blocks = (int)((total + 255) / 256);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, pr, (const float4*)d_tiles_all_ranks, 1.0f / (float)samples, d_rowmajor);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

extern "C" {

int vpt_render_device(vpt_scene* s, const vpt_params* params, const vpt_layout* layout, int nsamples, void* d_image,
    void* d_hits, void* d_rng, void* stream) {
  REQUIRE(s && params && layout && d_image && d_hits && d_rng, "null argument");
  if (int rc = check_shader(params)) return rc;
  if (int rc = check_camera(s, params)) return rc;
  REQUIRE(nsamples >= 0 && params->bounces >= 0, "negative sample/bounce count");
  if (nsamples == 0) return VPT_OK;
  DParams pr;
  if (int rc = make_dparams(params, layout, nsamples, pr)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  traversal_launch t;
  if (int rc = traversal_setup(s, pr.nslots, t)) return rc;
  // K1 considers tile splitting when the launch is short of waves (vpt_split_policy.cpp).  K2 considers it on every layout (unless
  // VPT_SPLIT=0): K2's launches hold two waves per wave slot at 1280 x 533, so the longest-first schedule ends well above both of
  // its bounds (226 ms against a longest wave of 192 and 191 of work per slot); the costliest tiles as partly filled waves - whose
  // scene rounds run in the group form: four lanes per ray - pack better.
  // K3 (volgrid, id 16) is scheduled like K2: its waves have K2's character - chains of dependent steps whose length varies by orders of
  // magnitude between tiles (its own occupancy: vpt_launch.h, VPT_K3_WAVES; the split policy reads K2.s tables for it)
  const bool k2 = params->shader >= VPT_SHADER_IMPLICIT;
  if (int rc = shader_setup(s, params, st)) return rc;   // K2: the scene's SDF records must fit the kernel's LDS; K3: its refusals and tables
  const bool may_split = k2 ? split_mode() != 0
                            : !t.stack.spill && (split_mode() == 1 || split_forced_k() >= 0 ||
                                                 (split_mode() < 0 && (pr.nranks > 1 || (long long)t.grid.x < 3ll * s->sched.wave_slots(false))));
  const long long key[10] = {pr.nslots, pr.width, pr.height, params->shader, params->camera, params->bounces, pr.rank, pr.nranks, pr.tile_w, pr.tile_h};
  HIP_TRY(hipEventRecord(s->ev0, st));
  const launch_ctx L = {s, st, (float4*)d_image, (int*)d_hits, (ulonglong2*)d_rng, t.stack, t.lds};
  if (int rc = s->sched.run(key, t.grid, nsamples, st, may_split, k2,
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

int vpt_render(vpt_scene* s, const vpt_params* params, int nsamples, int width, int height, float* image_rgba,
    int32_t* hits, uint64_t* rng, int* samples_io) {
  REQUIRE(s && params && image_rgba && hits && rng && samples_io, "null argument");
  REQUIRE(width > 0 && height > 0, "bad image size");
  if (int rc = check_shader(params)) return rc;
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

int vpt_last_wave_costs(vpt_scene* s, unsigned* ticks, int capacity, int* count) {
  REQUIRE(s && count && capacity >= 0 && (capacity == 0 || ticks), "bad argument");
  REQUIRE(s->timed, "no launch recorded");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipEventSynchronize(s->ev1));
  return s->sched.last_wave_costs(ticks, capacity, count);
}

// synchronous: waves of the implicit kernel that hit their watchdog since the scene was created (a defect, never a workload)
int vpt_check_watchdog(vpt_scene* s) {
  REQUIRE(s, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  unsigned n = 0;
  HIP_TRY(hipMemcpy(&n, s->d_watchdog.get(), 4, hipMemcpyDeviceToHost));
  if (n) return vpt_set_error(VPT_ERR_HIP, "%u wave(s) of the implicit kernel gave up after their watchdog time: the result is incomplete", n);
  return VPT_OK;
}

int vpt_last_kernel_ms(vpt_scene* s, float* ms) {
  REQUIRE(s && ms, "null argument");
  REQUIRE(s->timed, "no launch recorded");
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
