// vpt_volgrid_aov_kernel.hip.h — the first-collision pass of the volgrid shader (include/vpt.h: vpt_render_volgrid_aov_device, DESIGN.md
// §31): per sample the camera ray of K3's V_NEW block, ONE free flight made of K3's vg_start / vg_track_step calls
// (vpt_volgrid_kernel.hip.h: included, not copied - the draws, the t sequence and the collision are K3's bit for bit), and every
// first-collision quantity the caller asked for: an opacity sum, the colliding instance's albedo, a depth sum, the normal of the density
// (csrc/vpt_volgrid_rule.h: vpt_volgrid_normal), the {grid instance, volume} pair and the position of the chain's first collision.
//
// Design.  K3's tile shape: one workgroup = one wave64 = one 8x8 tile of the tile-major state, one lane per slot for the whole launch,
// the records of the grid instances in LDS.  The lane keeps its stream, its walk and the sums of the planes asked for in registers: HBM
// is read once and written once per launch.  There is no quorum and no shading block: the wave runs rounds of VPT_K3_STEPS tracking
// steps for the lanes that track; at the end of a round the lanes whose flight ended in it accumulate their sample and start the next
// one TOGETHER, and the wave ends when no lane tracks.  A lane waits at most the rest of one round, never for twenty others.
// Measured: the first form of this kernel ended and started samples inside the step loop, under the exec mask of the
// few lanes whose flight ended at that very step - the end of a flight plus a camera ray (four draws, two divisions, eval_camera) is
// not small against a tracking step, and it ran up to twelve times a round at a few lanes' worth of use: 12.9 ms against 9.7 ms for
// this form on the dense scene.  What is left against K3 at bounces = 1 (5.7 ms) is the launch, not the kernel: the issue asks for one
// plain launch, and the same kernel launched through K3's longest-first schedule with tile splitting ran at 5.4 ms.
// Every loop is bounded: a flight by VPT_VOLGRID_MAX_STEPS (vg_track_step's own test; the lane then adds to the handle's watchdog
// word, as K3 does), a lane by nsamples flights.
//
// MASK names the planes an instance can write (VA_*): sums the instance does not hold cost no register, and a plane of the mask whose
// pointer is null is skipped at run time.  Three instances are built - opacity alone, ids / hit alone, everything - and the launcher
// takes the smallest that covers the request (vpt_volgrid_aov.hip; the compiler's figures for each: DESIGN.md §31).
#pragma once
#include "vpt_volgrid_kernel.hip.h"

// the planes of include/vpt.h's vpt_volgrid_aov_planes as the kernels see them: tile-major, one entry per state slot, any of them null
struct volgrid_aov_planes {
  float4 *opacity, *albedo, *depth, *normal;   // sums over the samples
  int2*   ids;                                 // {grid instance, volume} of the chain's first collision
  float4* hit;                                 // {position, t} of the same
};
enum { VA_OPACITY = 1, VA_ALBEDO = 2, VA_DEPTH = 4, VA_NORMAL = 8, VA_IDS = 16, VA_ALL = 31 };

// one sample's value into a sum held in registers; a value that is not finite counts as zeros, decided per plane (vpt_aov_add.hip.h's rule)
VPT_DEV void va_add(f4& sum, float x, float y, float z, float alpha) {
  f4 v = mk4(x, y, z, alpha);
  if (!(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w))) v = mk4(0, 0, 0, 0);
  sum = sum + v;
}
VPT_DEV f4 va_load(const float4* __restrict__ plane, int slot) {
  const float4 a = plane[slot];
  return mk4(a.x, a.y, a.z, a.w);
}

template <int MASK>
__global__ void __launch_bounds__(VPT_BLOCK, VPT_K3_WAVES) vpt_volgrid_aov_kernel(DScene sc, DParams pr, volgrid_args va, volgrid_aov_planes pl,
    int* __restrict__ hits, ulonglong2* __restrict__ rngs) {
  extern __shared__ int4 lds_aov_recs4[];
  {   // the records, copied once into LDS (read at every tracking step), as K3 copies them
    const int4* src = (const int4*)va.recs;
    const int   n4  = va.num_instances * (int)(sizeof(vpt_volgrid_record) / sizeof(int4));
    for (int i = threadIdx.x; i < n4; i += VPT_BLOCK) lds_aov_recs4[i] = src[i];
  }
  __syncthreads();
  const vpt_volgrid_record* recs = (const vpt_volgrid_record*)lds_aov_recs4;

  const int slot = blockIdx.x * VPT_BLOCK + threadIdx.x;
  int       px = 0, py = 0;
  const bool owner = slot < pr.nslots && slot_to_pixel(pr, slot, px, py);   // padding lanes, other ranks' slots: V_DONE from the start
  if (__builtin_amdgcn_ballot_w64(owner) == 0) return;

  const bool want_opacity = (MASK & VA_OPACITY) && pl.opacity, want_albedo = (MASK & VA_ALBEDO) && pl.albedo;
  const bool want_depth = (MASK & VA_DEPTH) && pl.depth, want_normal = (MASK & VA_NORMAL) && pl.normal;
  const bool want_ids = (MASK & VA_IDS) && pl.ids, want_hit = want_ids && pl.hit;

  rng_t rng = {0, 1};
  f4    s_opacity = mk4(0, 0, 0, 0), s_albedo = s_opacity, s_depth = s_opacity, s_normal = s_opacity, first_hit = s_opacity;
  int2  first_id = make_int2(-1, -1);
  if (owner) {
    const ulonglong2 r_in = rngs[slot];
    rng.state = r_in.x, rng.inc = r_in.y;
    if (want_opacity) s_opacity = va_load(pl.opacity, slot);
    if (want_albedo) s_albedo = va_load(pl.albedo, slot);
    if (want_depth) s_depth = va_load(pl.depth, slot);
    if (want_normal) s_normal = va_load(pl.normal, slot);
    if (want_ids && hits[slot] != 0) {   // a chain under way: what its earlier launches found; a state at hits == 0 starts from {-1, -1}
      first_id = pl.ids[slot];
      if (want_hit) first_hit = va_load(pl.hit, slot);
    }
  }
  const vpt_camera& cam = sc.cameras[pr.camera];

  int     mode = V_DONE, sample = 0, aborted = 0;
  f3      ro = mk3(0, 0, 0), rd = mk3(0, 0, 1);
  vg_walk w;
  vg_start(w);

  // K3's V_NEW block: u, v, lens in its order (the pixel-centre branch draws no jitter), the camera ray, a fresh walk
  auto begin_sample = [&]() {
    if (sample == pr.nsamples) {
      mode = V_DONE;
      return;
    }
    float u, v;
    if (pr.preview) {
      u = (px + 0.5f) / pr.width, v = (py + 0.5f) / pr.height;
    } else {
      u = (px + rand1f(rng)) / pr.width;
      v = (py + rand1f(rng)) / pr.height;
    }
    f2 lens;
    lens.x = rand1f(rng);
    lens.y = rand1f(rng);
    const ray_t ray = eval_camera(cam, mk2(u, v), lens);
    ro = ray.o, rd = ray.d, mode = V_TRACK;
    vg_start(w);
  };
  // the flight ended in `ended` (V_COLLIDE, V_ESCAPE, V_ABORT): this sample's value into every sum; an escape or an abort adds zeros
  auto end_sample = [&](int ended) {
    sample++;
    if (ended == V_ABORT) aborted++;
    if (ended != V_COLLIDE) return;
    const vpt_volgrid_record& rec = recs[w.hit_g];
    const float t = w.tmax;
    const f3    position = ro + rd * t;   // K3's collision point, in its order
    if (want_opacity) va_add(s_opacity, 1, 1, 1, 1);
    if (want_albedo) va_add(s_albedo, rec.albedo[0], rec.albedo[1], rec.albedo[2], 1);
    if (want_depth) va_add(s_depth, t, 0, 0, 1);
    if (want_normal) {   // the eight voxels of the collision cell, fetched once for the three components
      float n[3];
      vpt_volgrid_normal(rec, sc.voxels, position.x, position.y, position.z, n, nullptr);
      va_add(s_normal, n[0] * 0.5f + 0.5f, n[1] * 0.5f + 0.5f, n[2] * 0.5f + 0.5f, 1);
    }
    if (want_ids && first_id.x == -1 && first_id.y == -1) {   // the chain's first collision
      first_id = make_int2(w.hit_g, rec.volume);
      first_hit = mk4(0, 0, 0, 0);
      va_add(first_hit, position.x, position.y, position.z, t);
    }
  };

  if (owner) begin_sample();
  while (__builtin_amdgcn_ballot_w64(mode == V_TRACK) != 0) {
    for (int k = 0; k < VPT_K3_STEPS; k++)
      if (mode == V_TRACK) mode = vg_track_step(sc, va, recs, ro, rd, rng, w);
    if (mode != V_TRACK && mode != V_DONE) {   // the lanes whose flight ended in this round, together
      end_sample(mode);
      begin_sample();
    }
  }

  if (aborted > 0 && va.watchdog) atomicAdd(va.watchdog, (unsigned)aborted);
  if (owner) {
    if (want_opacity) pl.opacity[slot] = make_float4(s_opacity.x, s_opacity.y, s_opacity.z, s_opacity.w);
    if (want_albedo) pl.albedo[slot] = make_float4(s_albedo.x, s_albedo.y, s_albedo.z, s_albedo.w);
    if (want_depth) pl.depth[slot] = make_float4(s_depth.x, s_depth.y, s_depth.z, s_depth.w);
    if (want_normal) pl.normal[slot] = make_float4(s_normal.x, s_normal.y, s_normal.z, s_normal.w);
    if (want_ids) pl.ids[slot] = first_id;
    if (want_hit) pl.hit[slot] = make_float4(first_hit.x, first_hit.y, first_hit.z, first_hit.w);
    hits[slot] += pr.nsamples;
    ulonglong2 r_out;
    r_out.x = rng.state, r_out.y = rng.inc;
    rngs[slot] = r_out;
  }
}

// The 48 bytes of a vpt_volgrid_pick for one pixel of the row-major id frame: the ids and {position, t} as the pass left them, the
// material from the resident instance table, the normal and the density by the rule's functions at the stored position
__global__ void vpt_volgrid_pick_kernel(DScene sc, volgrid_args va, const int2* __restrict__ ids, const float4* __restrict__ hit, long long pixel,
    int* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int2   id = ids[pixel];
  const float4 h  = hit[pixel];
  for (int c = 0; c < 12; c++) out[c] = c >= 1 && c <= 3 ? -1 : 0;   // a miss: hit 0, the three ids -1, the floats 0
  if (!(id.x >= 0 && id.x < va.num_instances)) return;
  const vpt_volgrid_record& rec = va.recs[id.x];
  float n[3];
  vpt_volgrid_normal(rec, sc.voxels, h.x, h.y, h.z, n, nullptr);
  out[0] = 1, out[1] = id.x, out[2] = rec.volume, out[3] = sc.vol_instances[id.x].material;
  out[4] = __float_as_int(h.w);
  out[5] = __float_as_int(h.x), out[6] = __float_as_int(h.y), out[7] = __float_as_int(h.z);
  out[8] = __float_as_int(n[0]), out[9] = __float_as_int(n[1]), out[10] = __float_as_int(n[2]);
  out[11] = __float_as_int(vpt_volgrid_density(rec, sc.voxels, h.x, h.y, h.z));
}
