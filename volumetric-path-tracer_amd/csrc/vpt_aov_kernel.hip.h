// vpt_aov_kernel.hip.h — the first-hit pass (include/vpt.h: vpt_render_aov_device): per sample the camera ray of K1's
// ST_NEW block, ONE traverse(), and every first-hit quantity the caller asked for - the values of the three debug shaders (K1's
// K_DEBUG branch, function for function: the same bits), a depth sum, the hit's ids.  Instances: vpt_aov.hip (faces only) and
// vpt_k1_curves.hip (scenes with points or lines), as vpt_intersect's.
//  * one lane per state slot, no regeneration: every lane renders the launch's nsamples one after the other, so the wave stays in
//    step and the whole wave enters every traverse() (a lane without a pixel as a helper: the group forms need every lane);
//  * the accumulators never sit in registers across traverse(): a requested plane is read, added to and written once per sample
//    (a float4 per plane and sample against hundreds of node fetches of the query); what a lane carries through the query is its
//    RNG stream, its ray's direction and two words (its slot, its pixel's coordinates packed as K1 parks them);
//  * the general leaf and attribute records, as the debug shaders read them.
#pragma once
#include "vpt_mesh_kernel.hip.h"
#include "vpt_aov_add.hip.h"   // aov_add: one sample's value into a sum plane

template <bool SPILL, bool CURVES>
__global__ void vpt_aov_kernel(DScene sc, DParams pr, aov_planes pl, int* __restrict__ hits, ulonglong2* __restrict__ rngs, stack_cfg stack) {
  extern __shared__ int lds_stack[];
  const lane_stack2<SPILL> stk = make_lane_stack<SPILL>(lds_stack, stack);
  int slot = blockIdx.x * VPT_BLOCK + threadIdx.x;
  int pxy  = 0;   // px | py << 16 (a frame side is below 32768: make_dparams)
  {
    int px = 0, py = 0;
    if (!(slot < pr.nslots && slot_to_pixel(pr, slot, px, py))) slot = -1;   // padding, or another rank's: a helper lane
    pxy = px | (py << 16);
  }
  const bool       live  = slot >= 0;
  const ulonglong2 r_in  = live ? rngs[slot] : make_ulonglong2(0, 1);
  rng_t            rng   = {r_in.x, r_in.y};
  bool             first = live && hits[slot] == 0;   // the state's first sample writes ids / uvt; later ones leave them alone

  for (int sample = 0; sample < pr.nsamples; sample++) {   // wave-uniform: every lane takes every trip
    ray_t ray = make_ray(mk3(0, 0, 0), mk3(0, 0, 1));
    if (live) {   // K1's ST_NEW block: u, v, lens in its order; the pixel-centre branch draws no jitter
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
      ray    = eval_camera(cam, mk2(u, v), lens);
    }
    const hit_t h = traverse<false, CURVES>(sc, live, ray.o, ray.d, -1, stk);
    if (live) {
      if (pl.ids && first) {   // vpt_intersect's format
        pl.ids[slot] = h.hit ? make_int2(h.instance, h.element) : make_int2(-1, -1);
        if (pl.uvt) pl.uvt[3 * (long long)slot] = h.hit ? h.uv.x : 0, pl.uvt[3 * (long long)slot + 1] = h.hit ? h.uv.y : 0, pl.uvt[3 * (long long)slot + 2] = h.hit ? h.distance : 0;
      }
      first = false;
      // shade_normal / texcoord / color (cpp:893-930) as K1's K_DEBUG branch evaluates them; its miss adds radiance 0, alpha 0
      f3    normal = mk3(0, 0, 0), albedo = mk3(0, 0, 0), texcoord = mk3(0, 0, 0);
      float alpha  = 0;
      if (h.hit) {
        const DInstance& inst  = sc.instances[h.instance];
        bool             curve = false;
        if constexpr (CURVES) {   // points and lines (vpt_scene.hip.h: curve_*)
          if (inst.shape_flags & (VPT_SHP_POINTS | VPT_SHP_LINES)) {
            curve      = true;
            const f2 t = curve_texcoord(sc, inst, h.element, h.uv);
            if (pl.normal) normal = curve_shading_normal(sc, inst, h.element, h.uv, -ray.d);
            if (pl.texcoord) texcoord = mk3(t.x, t.y, 0);
            if (pl.albedo) albedo = eval_material_at(sc, sc.materials[inst.material], t, curve_color(sc, inst, h.element, h.uv)).color;
          }
        }
        if (!curve) {
          if (pl.normal) normal = eval_shading_normal(sc, inst, h.element, h.uv, -ray.d);
          if (pl.texcoord) {
            const f2 t = eval_texcoord(sc, inst, h.element, h.uv);
            texcoord   = mk3(t.x, t.y, 0);
          }
          if (pl.albedo) albedo = eval_material(sc, inst, h.element, h.uv).color;
        }
        alpha = 1;
      }
      if (pl.normal) aov_add(pl.normal, slot, normal, alpha);
      if (pl.albedo) aov_add(pl.albedo, slot, albedo, alpha);
      if (pl.texcoord) aov_add(pl.texcoord, slot, texcoord, alpha);
      if (pl.depth) aov_add(pl.depth, slot, mk3(h.hit ? h.distance : 0, 0, 0), alpha);
    }
  }

  if (live) {
    hits[slot] += pr.nsamples;
    ulonglong2 r_out;
    r_out.x = rng.state, r_out.y = rng.inc;
    rngs[slot] = r_out;
  }
}

#define VPT_AOV_DEFINE(S, C) template __global__ void vpt_aov_kernel<S, C>(DScene, DParams, aov_planes, int* __restrict__, ulonglong2* __restrict__, stack_cfg);
