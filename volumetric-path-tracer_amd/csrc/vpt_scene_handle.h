// vpt_scene_handle.h — the scene handle of include/vpt.h, declared once: a `resident` (vpt_resident.h) plus its render side, and the few
// render-side functions more than one unit needs (vpt_render.hip defines them).  For vpt_capi.hip, vpt_render.hip, vpt_adaptive.hip,
// vpt_aov.hip and vpt_probes.hip; the update units, vpt_scene_inspect.hip, vpt_sdf_aov.hip and vpt_sdf_mesh.hip see vpt_resident.h alone.
#pragma once
#include <type_traits>

#include "vpt_launch.h"
#include "vpt_layout.h"
#include "vpt_resident.h"
#include "vpt_schedule.h"

// K3's tables (vpt_volgrid.hip): the grid instances as media and the brick majorants of the volumes, built by the first volgrid launch or
// query of a handle and again whenever the scene has changed since - a scene that never renders `volgrid` never builds them
struct volgrid_tables {
  unsigned long long built_edits = 0, built_voxels = 0;   // vpt_scene::edit_generation / voxel_generation they were built at (0: never)
  device_buffer      recs, bricks, steps;                 // vpt_volgrid_record per grid instance; the brick pool; the step counter
  std::vector<int>   brick_offset;                        // per volume: its table in the pool (nbx * nby * nbz majorants, then their maximum)
  long long          num_bricks = 0;                      // floats of the pool
  int                num_env_lights = 0;
  int                rebuilds = 0;                        // brick-table builds so far (tests of staleness, measurements)
};

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
  // every edit that changed the scene bumps edit_generation, every one that wrote voxels (vpt_scene_update_volumes with its bakes and pool
  // growth, vpt_scene_sculpt_volumes) voxel_generation too (vpt_capi.hip: edit_scene); creation is generation 1
  unsigned long long edit_generation = 1, voxel_generation = 1;
  volgrid_tables     volgrid;
};

// What every launch of a kernel that traverses the BVHs is set up with, for `items` lanes of work (state slots, rays, records): the grid
// of VPT_BLOCK lanes, the stack configuration - its HBM part grown to the grid's lanes where the scene has one - and the bytes of the
// (ref, t0) stack in LDS.  What else a kernel keeps in LDS its caller adds.
struct traversal_launch { dim3 grid; stack_cfg stack; size_t lds; };
int traversal_setup(vpt_scene* s, long long items, traversal_launch& out);

// f(std::bool_constant<flag>{}...) for run-time flags.  Every combination is instantiated: each must name a kernel instance that some
// kernel unit defines, or the link (--no-undefined) fails
template <typename F> void with_flags(F&& f) { f(); }
template <typename F, typename... Flags> void with_flags(F&& f, bool flag, Flags... rest) {
  if (flag) with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// what a call that renders hands to the kernel launchers, whatever the grid and the sample count of a launch
struct launch_ctx {
  vpt_scene*        s;
  hipStream_t       st;
  float4*           img;
  int*              hit;
  ulonglong2*       rng;
  stack_cfg         stack;   // and lds: of traversal_setup over the full layout
  size_t            lds;
};
// the launcher of the kernel instances of `shader`: the one table of vpt_render_device and of the rounds of an adaptive run (both
// have checked the shader's range)
using instance_launcher = void (*)(const launch_ctx&, bool is_pilot, dim3 grid, const DParams&, const sched_cfg&);
instance_launcher launcher_of(int shader);
// K2 (implicit shaders): LDS of a launch (the refs-only stack + the scene's SDF records); VPT_ERR_UNSUPPORTED when they do not fit
int implicit_lds(const vpt_scene* s, size_t* bytes = nullptr);

// K3 (volgrid): the refusals of a render (a grid instance whose material has no usable trdepth: VPT_ERR_INVALID_ARG, nothing touched), then
// the tables brought up to date on `st` (vpt_volgrid.hip)
int volgrid_prepare(vpt_scene* s, hipStream_t st);
// the kernel argument of a prepared handle
volgrid_args volgrid_arguments(const vpt_scene* s);
// what a shader's kernel needs of the scene before its launches: K2 room for the SDF records in LDS, K3 its tables, K1 nothing
inline int shader_setup(vpt_scene* s, const vpt_params* p, hipStream_t st) {
  if (p->shader == VPT_SHADER_VOLGRID) return volgrid_prepare(s, st);
  return p->shader >= VPT_SHADER_IMPLICIT ? implicit_lds(s) : VPT_OK;
}

// the two checks on vpt_params that every entry point that renders makes.  Ids 0-8 are the reference's, 9-15 stay unknown, 16 is volgrid
inline int check_shader(const vpt_params* p) { return vpt_shader_known(p->shader) ? VPT_OK : vpt_set_error(VPT_ERR_UNKNOWN_SHADER, "sampler unknown"); }
inline int check_camera(const vpt_scene* s, const vpt_params* p) { REQUIRE(p->camera >= 0 && p->camera < s->d.num_cameras, "camera %d out of range", p->camera); return VPT_OK; }

// vpt_render / vpt_render_adaptive: the host state through the scene handle's staging (one rank, 8x8 tiles) and render(layout, tiles)
template <typename Render>
int render_staged(vpt_scene* s, int width, int height, float* image_rgba, int32_t* hits, uint64_t* rng, Render&& render) {
  HIP_TRY(hipSetDevice(s->device));
  const vpt_layout lay      = {width, height, 8, 8, 0, 1};
  const host_plane state[3] = {{image_rgba, 16}, {hits, 4}, {rng, 16}};
  if (int rc = layout_round_trip(lay, state, 3, &s->staging, render)) return rc;
  return vpt_check_watchdog(s);
}
