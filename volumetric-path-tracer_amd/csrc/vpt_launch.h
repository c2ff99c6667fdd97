// vpt_launch.h — the kernels the host launches (vpt_render.hip, vpt_probes.hip, vpt_capi.hip, vpt_schedule.hip): declarations only, with their launch bounds, the types of their
// arguments and the launch constants both sides need.  Those units see no kernel body: each kernel is defined, and its instances
// instantiated, in exactly one kernel unit, so that a host-side edit recompiles no kernel and no kernel is compiled twice:
//   vpt_k1_volpath.hip, vpt_k1_path.hip   K1 (vpt_mesh_kernel.hip.h) for the two path tracers        (the instance lists:
//   vpt_k1_curves.hip                     K1 for scenes with points or lines, + vpt_intersect on them   vpt_k1_instances.hip.h)
//   vpt_k1_simple.hip                     K1 for naive, eyelight and the debug shaders
//   vpt_k2.hip                            K2 (vpt_implicit_kernel.hip.h)
//   vpt_k3.hip                            K3 (vpt_volgrid_kernel.hip.h)
//   vpt_aov.hip                           the first-hit pass (vpt_aov_kernel.hip.h)
//   vpt_kernels.hip                       vpt_intersect, the KAT kernel, the self-tests, light setup, launch schedule, output resolve
// (the copies between row-major pixels and tile-major slots are one kernel of vpt_layout.hip, launched there: not declared here)
// The launch bounds live here only: a definition inherits them from these declarations.
#pragma once
#include "vpt_device.h"

#define VPT_WAVES_PER_SIMD 3   // K1's waves per SIMD (v10 at 2 / 4: 511 / 468 Msamples/s against 578-586 at 3; v16 at 2: 629 against 766-769)
#define VPT_K2_WAVES 5         // K2's waves per SIMD (round 3, with the settings of vpt_implicit_kernel.hip.h: 4: 324, 5: 341, 6: 284 Msamples/s on 06_gridsdf_full; round 2's kernel lost at 5)
#define VPT_K2_WATCHDOG_TICKS 30000000000ull   // 300 s: two orders of magnitude above the longest wave of any test workload (the launch passes it as an argument; VPT_K2_WATCHDOG_MS overrides it for the tests of the error path)

enum { K_VOLPATH = 0, K_PATH = 1, K_NAIVE = 2, K_EYELIGHT = 3, K_DEBUG = 4, K_IMPLICIT = 5, K_IMPLICIT_NORMAL = 6 };

// (ref, t0) stack of one lane: the first `cap` entries live in LDS (entry-major: conflict-free), deeper
// ones in a per-launch HBM array (entry-major too: coalesced).  `cap` covers what traversals use in
// practice; the HBM part only makes the worst case (three pending siblings on every quad level) safe.
struct stack_cfg {
  int        cap;      // entries per lane in LDS
  int        spill;    // entries per lane in HBM
  int2*      mem;      // spill * lanes entries
  long long  lanes;    // lanes of the launch (= entry stride)
};

// Launch schedule.  A wave's 64 pixels run all their samples in sequence, so a wave's duration is fixed by its
// tile's content and varies 15x across 03_volume; in tile order the launch ends with a third of the GPU idle
// behind a few long waves.  Every wave records its duration; the next launch on the same layout starts the
// waves longest first (order[] = wave indices by descending cost: LPT list scheduling).  Results do not depend
// on the order (pixels are independent), only the makespan does.
struct sched_cfg {
  const int* order;       // blockIdx.x -> wave index, or null: identity
  unsigned*  cost;        // per wave: duration of this launch in 100 MHz ticks, or null
  const int* lane_slot;   // [wave][64] -> state slot of the lane (-1: none), or null: slot = wave * 64 + lane (one tile per wave).
                          // Set when costly tiles run as several partly filled waves (vpt_schedule.hip: tile splitting)
};

// ---- K1: the mesh shaders (vpt_mesh_kernel.hip.h); the pilot is the same kernel under another name --------------------------
template <int SH, bool SPILL, int FEAT>
__global__ void __launch_bounds__(VPT_BLOCK, VPT_WAVES_PER_SIMD) vpt_mesh_kernel(DScene sc, DParams pr, float4* __restrict__ image,
    int* __restrict__ hits, ulonglong2* __restrict__ rngs, stack_cfg stack, sched_cfg sched);
template <int SH, bool SPILL, int FEAT>
__global__ void __launch_bounds__(VPT_BLOCK, VPT_WAVES_PER_SIMD) vpt_mesh_pilot_kernel(DScene sc, DParams pr, float4* __restrict__ image,
    int* __restrict__ hits, ulonglong2* __restrict__ rngs, stack_cfg stack, sched_cfg sched);
#include "vpt_k1_instances.hip.h"
VPT_K1_SPLIT_INSTANCES(VPT_K1_DECLARE, K_VOLPATH)
VPT_K1_SPLIT_INSTANCES(VPT_K1_DECLARE, K_PATH)
VPT_K1_SIMPLE_INSTANCES(VPT_K1_DECLARE, K_NAIVE)
VPT_K1_SIMPLE_INSTANCES(VPT_K1_DECLARE, K_EYELIGHT)
VPT_K1_SIMPLE_INSTANCES(VPT_K1_DECLARE, K_DEBUG)
VPT_K1_CURVES_INSTANCES(VPT_K1_DECLARE, K_VOLPATH)
VPT_K1_CURVES_INSTANCES(VPT_K1_DECLARE, K_PATH)
VPT_K1_CURVES_INSTANCES(VPT_K1_DECLARE, K_NAIVE)
VPT_K1_CURVES_INSTANCES(VPT_K1_DECLARE, K_EYELIGHT)
VPT_K1_CURVES_INSTANCES(VPT_K1_DECLARE, K_DEBUG)

// ---- K2: the implicit shaders (vpt_implicit_kernel.hip.h), for K_IMPLICIT / K_IMPLICIT_NORMAL x VPT_FEAT_SDF_LIGHTS / VPT_FEAT_ALL --
template <int SH, int FEAT>
__global__ void __launch_bounds__(VPT_BLOCK, VPT_K2_WAVES) vpt_render_kernel(DScene sc, DParams pr, float4* __restrict__ image,
    int* __restrict__ hits, ulonglong2* __restrict__ rngs, int stack_cap, sched_cfg sched, unsigned* __restrict__ watchdog, unsigned long long watchdog_ticks);
template <int SH, int FEAT>
__global__ void __launch_bounds__(VPT_BLOCK, VPT_K2_WAVES) vpt_render_pilot_kernel(DScene sc, DParams pr, float4* __restrict__ image,
    int* __restrict__ hits, ulonglong2* __restrict__ rngs, int stack_cap, sched_cfg sched, unsigned* __restrict__ watchdog, unsigned long long watchdog_ticks);

// ---- K3: the volgrid shader (vpt_volgrid_kernel.hip.h; instances: vpt_k3.hip) ---------------------------------------------------
// K3's tables travel in an argument of their own: DScene stays byte for byte what the other kernels are compiled for
struct vpt_volgrid_record;   // vpt_volgrid_rule.h
struct volgrid_args {
  const vpt_volgrid_record* recs;     // one per grid instance, in instance order
  const float*              bricks;   // the brick pool: per volume its nbx * nby * nbz majorants (x fastest), then their maximum
  int                       num_instances;
  int                       num_env_lights;   // light-list entries with an environment
  int                       no_bricks;        // VPT_VOLGRID_NO_BRICKS=1: one majorant per volume (the A/B switch of the tests and the measurements)
  unsigned*                 watchdog;         // the handle's counter: free flights that ran into VPT_VOLGRID_MAX_STEPS
  unsigned long long*       steps;            // tracking steps taken since the handle was made (vpt_scene_volgrid_stats)
};
#define VPT_K3_WAVES 4   // K3's waves per SIMD: 115 VGPRs and no scratch; at 5 (K2's) the allocator's 96 VGPRs leave 11 spilled, 48 bytes of scratch per lane
template <bool PILOT>
__global__ void __launch_bounds__(VPT_BLOCK, VPT_K3_WAVES) vpt_volgrid_kernel(DScene sc, DParams pr, volgrid_args va, float4* __restrict__ image,
    int* __restrict__ hits, ulonglong2* __restrict__ rngs, sched_cfg sched);
// the free-flight probe of vpt_scene_volgrid_track: one lane per record through K3's vg_start / vg_track_step (defined in vpt_k3.hip)
__global__ void vpt_volgrid_track_kernel(DScene sc, volgrid_args va, int n, const float* __restrict__ rays, const ulonglong2* __restrict__ rng_in,
    int* __restrict__ event, int* __restrict__ instance, float* __restrict__ t, int* __restrict__ steps, ulonglong2* __restrict__ rng_out);

// ---- vpt_intersect, KAT, self-tests (vpt_kernels.hip, but for vpt_intersect_curves_kernel: vpt_k1_curves.hip) ----------------
template <bool SPILL, bool COMPACT>
__global__ void __launch_bounds__(VPT_BLOCK, VPT_WAVES_PER_SIMD) vpt_intersect_kernel(DScene sc, int n, const float* rays, int instance,
    int* ids, float* uvt, stack_cfg stack);
template <bool SPILL>
__global__ void __launch_bounds__(VPT_BLOCK, VPT_WAVES_PER_SIMD) vpt_intersect_curves_kernel(DScene sc, int n, const float* rays, int instance,
    int* ids, float* uvt, stack_cfg stack);
template <bool SPILL>
__global__ void __launch_bounds__(VPT_BLOCK, VPT_WAVES_PER_SIMD) vpt_kat_kernel(DScene sc, int op, int iparam, int n, int si, int so,
    const float* __restrict__ in, const int* __restrict__ aux, float* __restrict__ out, stack_cfg stack, int stack_cap);
__global__ void vpt_reciprocal_selftest_kernel(unsigned long long* out);
__global__ void vpt_light_cdf_selftest_kernel(DScene sc, int light_id, int n, unsigned long long* out);

// ---- the first-hit pass (vpt_aov_kernel.hip.h; instances: vpt_aov.hip, and vpt_k1_curves.hip for scenes with points or lines) ----
// the planes of include/vpt.h's vpt_aov_planes as the kernels see them: tile-major, one entry per state slot, any of them null
struct aov_planes {
  float4 *normal, *albedo, *texcoord, *depth;   // sums over the samples
  int2*   ids;                                  // {instance, element} of the state's first sample
  float*  uvt;                                  // 3 per slot: {u, v, distance} of the same
};
template <bool SPILL, bool CURVES>
__global__ void __launch_bounds__(VPT_BLOCK, VPT_WAVES_PER_SIMD) vpt_aov_kernel(DScene sc, DParams pr, aov_planes pl, int* __restrict__ hits,
    ulonglong2* __restrict__ rngs, stack_cfg stack);

// ---- scene setup, launch schedule and output resolve (vpt_kernels.hip) --------------------------------------------------------
__global__ void vpt_light_setup_kernel(DScene sc, float4* out);
__global__ void vpt_medium_setup_kernel(DScene sc, float4* out);
__global__ void vpt_cost_average_kernel(const unsigned* __restrict__ cost, float* __restrict__ avg, unsigned* __restrict__ key, int n, float nsamples, float weight);
__global__ void vpt_resolve_kernel(DParams pr, const float4* tiles_all, float scale, float4* rows_image);
__global__ void vpt_resolve_srgb8_kernel(DParams pr, const float4* tiles_all, float scale, uchar4* rows_rgba8);
