// vpt_kernels.hip.h — what the render kernels share (slot map, roulette).  The render kernels themselves:
// vpt_mesh_kernel.hip.h (K1, the seven mesh shaders), vpt_implicit_kernel.hip.h (K2, the two SDF shaders); the
// output resolves: vpt_kernels.hip; the copies between the two layouts: vpt_layout.hip.  Declarations and launch types: vpt_launch.h.
#pragma once
#include "vpt_launch.h"
#include "vpt_scene.hip.h"

// slot -> pixel for the tile-major layout of include/vpt.h (vpt_layout)
VPT_DEV bool slot_to_pixel(const DParams& pr, int slot, int& px, int& py) {
  int per_tile   = pr.tile_w * pr.tile_h;
  int local_tile = slot / per_tile, p = slot - local_tile * per_tile;
  int tile       = local_tile * pr.nranks + pr.rank;
  if (tile >= pr.tiles_x * pr.tiles_y) return false;
  int ty = tile / pr.tiles_x, tx = tile - ty * pr.tiles_x;
  // inside a tile, pixels are ordered in 8x8 blocks so that a wave covers a square footprint
  int bw = pr.tile_w >> 3, blk = p >> 6, q = p & 63;
  int by = blk / bw, bx = blk - by * bw;
  px = tx * pr.tile_w + bx * 8 + (q & 7);
  py = ty * pr.tile_h + by * 8 + (q >> 3);
  return px < pr.width && py < pr.height;
}

// weight test + russian roulette, yocto_pathtrace.cpp:676-683
VPT_DEV bool survive(f3& weight, int bounce, rng_t& rng) {
  if (is_zero3(weight) || !finite3(weight)) return false;
  if (bounce > 3) {
    float rr_prob = fmin_(0.99f, max3(weight));
    if (rand1f(rng) >= rr_prob) return false;
    weight = weight * (1 / rr_prob);
  }
  return true;
}
