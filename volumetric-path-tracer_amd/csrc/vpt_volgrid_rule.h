// vpt_volgrid_rule.h — the parts of the `volgrid` shader's rule (include/vpt.h: VPT_SHADER_VOLGRID) that more than one side computes, written
// once: what a voxel counts for (clean), the brick majorants of a volume, the record of a grid instance as a medium, the density of a grid
// instance at a world point.  Compiled by K3 (csrc/vpt_volgrid_kernel.hip.h), by the table kernels and queries of csrc/vpt_volgrid.hip and by
// the host mirror (host/vpt_volgrid.cpp), all with -ffp-contract=off: float32 throughout, nothing fused, every sum in the order written
// here - so the device's tables and densities are the host mirror's bit for bit, and THIS FILE IS THEIR OPERATION ORDER.
//
// The lookup is the reference's: eval_sdf's mapping of a local point into the grid (yocto_sdfs.cpp:30-49: bbox_size = res * whd * scalef,
// uvw = p * 2 / bbox_size - 1) and eval_volume's trilerp (yocto_sdfs.cpp:92-127) in its term order - what K2's sdf_grid_world and
// eval_volume (csrc/vpt_scene.hip.h) compute for the same grid read as a distance.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "vpt.h"

#if defined(__HIPCC__)
#define VPT_VOLGRID_HD __host__ __device__ inline
#else
#define VPT_VOLGRID_HD inline
#endif

#define VPT_VOLGRID_BRICK 8   // cells per brick and axis: a brick reads nine nodes per axis

// A grid instance as a medium: 128 bytes, made on the host by vpt_volgrid_make_record from the instance, its volume and its material
struct alignas(16) vpt_volgrid_record {
  float   frame[12];       // the instance's frame x, y, z, o: transform_point(frame, p) is the point in the grid's box
  float   bbox[3];         // res * whd * scalef
  float   trdepth;         // of the material: a voxel value of 1 is a mean free path of trdepth
  float   albedo[3];       // scattering, clamped to [0, 1]
  float   g;               // scanisotropy
  float   emission[3];
  int32_t brick_offset;    // of the volume's brick table in the brick pool
  int32_t whd[3];
  int32_t volume;
  int64_t voxel_offset;    // of the volume in the voxel pool
  int32_t unused[2];
};
static_assert(sizeof(vpt_volgrid_record) == 128, "a volgrid record is eight float4");

// what a voxel counts for: itself when it is a finite positive number, else 0 (NaN, +-Inf, negative values, zero)
VPT_VOLGRID_HD float vpt_volgrid_clean(float x) { return (x > 0.0f && x <= 3.402823466e+38f) ? x : 0.0f; }

// bricks along an axis of W nodes: the W - 1 cells in runs of eight; a single node is one brick, no node none
VPT_VOLGRID_HD int vpt_volgrid_bricks(int w) { return w <= 0 ? 0 : (w == 1 ? 1 : (w - 1 + VPT_VOLGRID_BRICK - 1) / VPT_VOLGRID_BRICK); }

// the majorant of brick (bx, by, bz): the maximum of clean(node) over the nodes [8 b, min(8 b + 8, W - 1)] per axis.  The maximum of
// floats is exact, so the order of the loop is no part of the contract.
VPT_VOLGRID_HD float vpt_volgrid_brick_max(const float* vox, int w, int h, int d, int bx, int by, int bz) {
  const int x0 = bx * VPT_VOLGRID_BRICK, y0 = by * VPT_VOLGRID_BRICK, z0 = bz * VPT_VOLGRID_BRICK;
  const int x1 = x0 + VPT_VOLGRID_BRICK < w - 1 ? x0 + VPT_VOLGRID_BRICK : w - 1;
  const int y1 = y0 + VPT_VOLGRID_BRICK < h - 1 ? y0 + VPT_VOLGRID_BRICK : h - 1;
  const int z1 = z0 + VPT_VOLGRID_BRICK < d - 1 ? z0 + VPT_VOLGRID_BRICK : d - 1;
  float m = 0.0f;
  for (int z = z0; z <= z1; z++)
    for (int y = y0; y <= y1; y++)
      for (int x = x0; x <= x1; x++) {
        const float v = vpt_volgrid_clean(vox[(size_t)x + (size_t)y * (size_t)w + (size_t)z * (size_t)w * (size_t)h]);
        m = v > m ? v : m;
      }
  return m;
}

// the brick a node coordinate s in [0, W - 1] lies in (nb = vpt_volgrid_bricks(W)): that of the cell eval_volume reads, (int)s; the last
// node belongs to the last brick
VPT_VOLGRID_HD int vpt_volgrid_brick_of(float s, int nb) {
  const int b = (int)s / VPT_VOLGRID_BRICK;
  return b < nb - 1 ? b : (nb > 0 ? nb - 1 : 0);
}

// the record of a grid instance.  scalef scales the box only; the albedo is `scattering` clamped per channel
inline vpt_volgrid_record vpt_volgrid_make_record(const vpt_volume_instance& vi, const vpt_volume& vol, const vpt_material& mat, int brick_offset) {
  vpt_volgrid_record r = {};
  const float* f = (const float*)&vi.frame;
  for (int k = 0; k < 12; k++) r.frame[k] = f[k];
  for (int k = 0; k < 3; k++) {
    r.bbox[k]     = (vol.res * (float)vol.whd[k]) * vi.scalef;
    const float a = mat.scattering[k];
    r.albedo[k]   = a > 0.0f ? (a < 1.0f ? a : 1.0f) : 0.0f;   // NaN: 0
    r.emission[k] = mat.emission[k];
    r.whd[k]      = vol.whd[k];
  }
  r.trdepth = mat.trdepth, r.g = mat.scanisotropy;
  r.brick_offset = brick_offset, r.volume = vi.volume, r.voxel_offset = vol.offset;
  return r;
}
// the trdepth a medium needs: finite and > 0
inline bool vpt_volgrid_trdepth_ok(float trdepth) { return trdepth > 0.0f && trdepth <= 3.402823466e+38f; }

// transform_point(frame, p) = frame.x * p.x + frame.y * p.y + frame.z * p.z + frame.o and transform_vector (yocto_math.h), summed from the left
VPT_VOLGRID_HD void vpt_volgrid_to_local(const float* f, float px, float py, float pz, float out[3]) {
  out[0] = ((f[0] * px + f[3] * py) + f[6] * pz) + f[9];
  out[1] = ((f[1] * px + f[4] * py) + f[7] * pz) + f[10];
  out[2] = ((f[2] * px + f[5] * py) + f[8] * pz) + f[11];
}
VPT_VOLGRID_HD void vpt_volgrid_vector_to_local(const float* f, float px, float py, float pz, float out[3]) {
  out[0] = (f[0] * px + f[3] * py) + f[6] * pz;
  out[1] = (f[1] * px + f[4] * py) + f[7] * pz;
  out[2] = (f[2] * px + f[5] * py) + f[8] * pz;
}

// the node coordinate of a local coordinate pl in [0, bbox] along an axis of W nodes: eval_sdf's uvw = p * 2 / bbox - 1, then eval_volume's
// clamp((uvw + 1) * 0.5, 0, 1) * (W - 1), operation for operation
VPT_VOLGRID_HD float vpt_volgrid_node_coord(float pl, float bbox, int w) {
  const float uvw = pl * 2.f / bbox - 1;
  float       c   = (uvw + 1.0f) * 0.5f;
  c               = c > 0.0f ? c : 0.0f;   // clamp = min(max(a, lo), hi) with the ternaries of yocto_math.h
  c               = c < 1.0f ? c : 1.0f;
  return c * (w - 1);
}

// eval_volume's trilerp at node coordinates (s, t, r), in the reference's term order (yocto_sdfs.cpp:92-127)
VPT_VOLGRID_HD float vpt_volgrid_trilerp(const float* vox, int W, int H, int D, float s, float t, float r) {
  int i = (int)s, j = (int)t, k = (int)r;
  i = i > 0 ? (i < W - 1 ? i : W - 1) : 0, j = j > 0 ? (j < H - 1 ? j : H - 1) : 0, k = k > 0 ? (k < D - 1 ? k : D - 1) : 0;
  const int   ii = i + 1 < W - 1 ? i + 1 : W - 1, jj = j + 1 < H - 1 ? j + 1 : H - 1, kk = k + 1 < D - 1 ? k + 1 : D - 1;
  const float u = s - i, v = t - j, w = r - k;
  const int   WH = W * H, r0 = j * W + k * WH, r1 = jj * W + k * WH, r2 = j * W + kk * WH, r3 = jj * W + kk * WH;
  const float v000 = vox[i + r0], v100 = vox[ii + r0];
  const float v010 = vox[i + r1], v001 = vox[i + r2];
  const float v011 = vox[i + r3], v101 = vox[ii + r2];
  const float v110 = vox[ii + r1], v111 = vox[ii + r3];
  return v000 * (1 - u) * (1 - v) * (1 - w) + v100 * u * (1 - v) * (1 - w) + v010 * (1 - u) * v * (1 - w) +
         v001 * (1 - u) * (1 - v) * w + v011 * (1 - u) * v * w + v101 * u * (1 - v) * w + v110 * u * v * (1 - w) +
         v111 * u * v * w;
}

// Where a world point lies in a grid instance: false outside the box [0, bbox] (or for a grid without voxels); else the node coordinates
VPT_VOLGRID_HD bool vpt_volgrid_locate(const vpt_volgrid_record& rec, float px, float py, float pz, float node[3]) {
  if (rec.whd[0] <= 0 || rec.whd[1] <= 0 || rec.whd[2] <= 0) return false;
  float pl[3];
  vpt_volgrid_to_local(rec.frame, px, py, pz, pl);
  for (int k = 0; k < 3; k++) {
    if (!(pl[k] >= 0.0f && pl[k] <= rec.bbox[k])) return false;   // NaN: outside
    node[k] = vpt_volgrid_node_coord(pl[k], rec.bbox[k], rec.whd[k]);
  }
  return true;
}
// the extinction at node coordinates inside the box: sigma = clean(trilerp) / trdepth.  voxels: the pool
VPT_VOLGRID_HD float vpt_volgrid_sigma_at(const vpt_volgrid_record& rec, const float* voxels, const float node[3]) {
  return vpt_volgrid_clean(vpt_volgrid_trilerp(voxels + rec.voxel_offset, rec.whd[0], rec.whd[1], rec.whd[2], node[0], node[1], node[2])) / rec.trdepth;
}
// the density of a grid instance at a world point: 0 outside the box
VPT_VOLGRID_HD float vpt_volgrid_density(const vpt_volgrid_record& rec, const float* voxels, float px, float py, float pz) {
  float node[3];
  if (!vpt_volgrid_locate(rec, px, py, pz, node)) return 0.0f;
  return vpt_volgrid_sigma_at(rec, voxels, node);
}
