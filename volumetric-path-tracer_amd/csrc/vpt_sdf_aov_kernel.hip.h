// vpt_sdf_aov_kernel.hip.h — the first-hit pass of the implicit shaders (include/vpt.h: vpt_render_sdf_aov_device): per
// sample the camera ray of K2's M_NEW block, ONE whole-scene march made of K2's scene_march_step calls (vpt_implicit_kernel.hip.h: the t
// sequence, the hit test and the early-miss rule are K2's bit for bit), and every first-hit quantity the caller asked for - the value
// of shade_implicit_normal, the hit material's colour, a depth sum, the hit's {grid instance, analytic SDF} pair and its position.
//  * one lane per state slot, no regeneration, as vpt_aov_kernel: every lane renders the launch's nsamples one after the other; a lane
//    without a pixel stays in the wave as a helper (the group round moves rays between lanes: it needs every lane);
//  * the march loop is wave-level: rounds of VPT_K2_STEPS steps while any lane marches.  A round with at most VPT_K2_GROUP_MAX rays
//    runs four lanes per ray (K2's group form, here as one function); otherwise each lane steps its own ray;
//  * every loop is bounded: a march ends after at most spheretrace_maxiter steps (scene_march_step's own test), every round gives
//    every marching ray at least one step, so a sample takes at most maxiter + 1 rounds and a launch nsamples times that.  No watchdog;
//  * the SDF records sit in LDS, copied once per block as K2 does; there is no BVH stack;
//  * the accumulators never sit in registers across the march: a requested plane is read, added to and written once per sample.
#pragma once
#include "vpt_implicit_kernel.hip.h"
#include "vpt_aov_add.hip.h"

// the planes of include/vpt.h's vpt_sdf_aov_planes as the kernels see them: tile-major, one entry per state slot, any of them null
struct sdf_aov_planes {
  float4 *normal, *albedo, *depth;   // sums over the samples
  int2*   ids;                       // {grid instance, analytic SDF} of the state's first sample
  float4* hit;                       // {position, t} of the same
};

// One round of the scene march for a SMALL set of rays (`ms`: the lanes whose mode is M_SCENE, at most 16 of them): ray k of the set
// moves to lanes 4k .. 4k+3 - whoever owns them - each of which evaluates a quarter of the scene's SDFs per step
// (eval_sdf_scene_group), takes up to `steps` steps there and goes back to its owner.  A ray's t sequence is the sequential one, step
// for step.  The WHOLE wave must be in the call (DPP and ds_bpermute read 0 from a lane that is switched off); lanes that own no ray
// of the set keep mode, t, it, hit_instance and hit_sdf.
VPT_DEV void scene_march_group_round(const DScene& sc, const sdf_recs& recs, unsigned long long ms, f3 ro, f3 rd, int maxiter, int steps,
    int& mode, float& t, int& it, int& hit_instance, int& hit_sdf) {
  const int  lane = threadIdx.x & 63, gj = lane & 3;
  const bool mine = (ms >> lane) & 1;
  const int  rank = lanes_below(ms), nrays = __popcll(ms);
  int        gowner = quad_lane0(__builtin_amdgcn_ds_permute(mine ? rank << 4 : 4, lane));   // ray k's owner posts its lane number to lane 4k
  const bool gact = (lane >> 2) < nrays;
  if (!gact) gowner = lane;
  const f3 gro = pull(gowner, ro), grd = pull(gowner, rd);
  float    gt  = pull(gowner, t);
  int      git = pull(gowner, it), gmode = gact ? M_SCENE : M_DONE, ghi = -1, ghs = -1;
  for (int k = 0; k < steps && __builtin_amdgcn_ballot_w64(gmode == M_SCENE) != 0; k++)
    if (gmode == M_SCENE) gmode = scene_march_step<true>(sc, recs, gro, grd, maxiter, gt, git, ghi, ghs, gj);
  const int   src = mine ? rank << 2 : 0;   // the owner of ray k reads lane 4k
  const int   nmode = pull(src, gmode), nit = pull(src, git), nhi = pull(src, ghi), nhs = pull(src, ghs);
  const float nt = pull(src, gt);
  if (mine) {
    mode = nmode, t = nt, it = nit;
    if (nmode == M_HIT) hit_instance = nhi, hit_sdf = nhs;
  }
}

// (launch bounds: K2's waves per SIMD - the march is K2's, and so is its register budget)
__global__ void __launch_bounds__(VPT_BLOCK, VPT_K2_WAVES) vpt_sdf_aov_kernel(DScene sc, DParams pr, sdf_aov_planes pl, int* __restrict__ hits,
    ulonglong2* __restrict__ rngs) {
  extern __shared__ __attribute__((aligned(16))) float4 lds_rec[];   // the SDF records (read at every march step, the same address by all lanes)
  const int nfn4 = 6 * sc.num_sdfs, ngrid4 = 7 * sc.num_vol_instances;
  for (int i = threadIdx.x; i < nfn4; i += VPT_BLOCK) lds_rec[i] = sc.sdf_fn_rec[i];
  for (int i = threadIdx.x; i < ngrid4; i += VPT_BLOCK) lds_rec[nfn4 + i] = sc.sdf_grid_rec[i];
  __syncthreads();
  sdf_recs recs;
  recs.fn = lds_rec, recs.grid = lds_rec + nfn4;

  int slot = blockIdx.x * VPT_BLOCK + threadIdx.x;
  int pxy  = 0;   // px | py << 16 (a frame side is below 32768)
  {
    int px = 0, py = 0;
    if (!(slot < pr.nslots && slot_to_pixel(pr, slot, px, py))) slot = -1;   // padding, or another rank's: a helper lane
    pxy = px | (py << 16);
  }
  const bool live = slot >= 0;
  if (__builtin_amdgcn_ballot_w64(live) == 0) return;   // the whole wave owns no pixel
  const ulonglong2 r_in  = live ? rngs[slot] : make_ulonglong2(0, 1);
  rng_t            rng   = {r_in.x, r_in.y};
  bool             first = live && hits[slot] == 0;   // the state's first sample writes ids / hit; later ones leave them alone
  const int        maxiter = pr.spheretrace_maxiter;

  for (int sample = 0; sample < pr.nsamples; sample++) {   // wave-uniform: every lane takes every trip
    f3 ro = mk3(0, 0, 0), rd = mk3(0, 0, 1);
    if (live) {   // K2's M_NEW block: u, v, lens in its order; the pixel-centre branch draws no jitter
      const vpt_camera& cam = sc.cameras[pr.camera];
      const int px = pxy & 0xffff, py = pxy >> 16;
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
      ro = ray.o, rd = ray.d;
    }
    // ---- spheretrace(scene, ray, maxiter), cpp:289-307 ----------------------------------------------------------------------------
    float t = VPT_RAY_EPS;
    int   it = 0, hit_instance = -1, hit_sdf = -1, mode = live ? M_SCENE : M_DONE;
    for (int round = 0; round <= maxiter; round++) {   // every round steps every marching ray at least once: maxiter + 1 rounds end them all
      const unsigned long long ms = __builtin_amdgcn_ballot_w64(mode == M_SCENE);
      if (ms == 0) break;
      if (VPT_K2_GROUP_MAX > 0 && sc.group_forms != 0 && __popcll(ms) <= VPT_K2_GROUP_MAX && __builtin_amdgcn_ballot_w64(true) == ~0ull) {
        scene_march_group_round(sc, recs, ms, ro, rd, maxiter, VPT_K2_STEPS, mode, t, it, hit_instance, hit_sdf);
      } else {
        for (int k = 0; k < VPT_K2_STEPS; k++)
          if (mode == M_SCENE) mode = scene_march_step(sc, recs, ro, rd, maxiter, t, it, hit_instance, hit_sdf);
      }
    }
    if (live) {
      const bool hit      = mode == M_HIT;
      const f3   position = ro + rd * t;
      if (pl.ids && first) {   // spheretrace_result's pair: exactly one of the two >= 0 on a hit
        pl.ids[slot] = hit ? make_int2(hit_instance, hit_sdf) : make_int2(-1, -1);
        if (pl.hit) pl.hit[slot] = hit ? make_float4(position.x, position.y, position.z, t) : make_float4(0, 0, 0, 0);
      }
      first = false;
      // shade_implicit_normal (cpp:538-562) as K2's shading block evaluates it; its miss adds radiance 0, alpha 0.  A first hit is
      // reported whatever the material's opacity: this pass draws no number after the camera ray
      f3 normal = mk3(0, 0, 0), albedo = mk3(0, 0, 0);
      if (hit) {
        if (pl.normal) {
          const f3 n = hit_instance >= 0 ? eval_sdf_normal_grid(sc, recs, hit_instance, position, t) : eval_sdf_normal_function(recs, hit_sdf, position, t);
          normal     = n * 0.5f + 0.5f;
        }
        if (pl.albedo) albedo = eval_material_plain(sc, hit_instance >= 0 ? sc.vol_instances[hit_instance].material : sc.sdfs[hit_sdf].material).color;
      }
      const float alpha = hit ? 1.0f : 0.0f;
      if (pl.normal) aov_add(pl.normal, slot, normal, alpha);
      if (pl.albedo) aov_add(pl.albedo, slot, albedo, alpha);
      if (pl.depth) aov_add(pl.depth, slot, mk3(hit ? t : 0, 0, 0), alpha);
    }
  }

  if (live) {
    hits[slot] += pr.nsamples;
    ulonglong2 r_out;
    r_out.x = rng.state, r_out.y = rng.inc;
    rngs[slot] = r_out;
  }
}

// the 48 bytes of vpt_sdf_pick for one pixel of the row-major id frame: the ids and {position, t} as the pass left them, volume and
// material from the resident tables, the normal by the function K2's shading block would call at (position, t)
__global__ void vpt_sdf_pick_kernel(DScene sc, const int2* __restrict__ ids, const float4* __restrict__ hit, long long pixel, int* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int2   id = ids[pixel];
  const float4 h  = hit[pixel];
  const bool   grid = id.x >= 0 && id.x < sc.num_vol_instances, fn = !grid && id.y >= 0 && id.y < sc.num_sdfs;
  for (int c = 0; c < 12; c++) out[c] = c >= 1 && c <= 4 ? -1 : 0;   // a miss: hit 0, the four ids -1, the floats 0
  if (!grid && !fn) return;
  const f3       position = mk3(h.x, h.y, h.z);
  const sdf_recs recs     = scene_sdf_recs(sc);
  const f3       n        = grid ? eval_sdf_normal_grid(sc, recs, id.x, position, h.w) : eval_sdf_normal_function(recs, id.y, position, h.w);
  out[0] = 1, out[1] = grid ? id.x : -1, out[2] = grid ? -1 : id.y;
  out[3] = grid ? sc.vol_instances[id.x].volume : -1;
  out[4] = grid ? sc.vol_instances[id.x].material : sc.sdfs[id.y].material;
  out[5] = __float_as_int(h.w);
  out[6] = __float_as_int(h.x), out[7] = __float_as_int(h.y), out[8] = __float_as_int(h.z);
  out[9] = __float_as_int(n.x), out[10] = __float_as_int(n.y), out[11] = __float_as_int(n.z);
}
