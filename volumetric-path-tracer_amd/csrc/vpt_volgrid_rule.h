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

// ---- coloured extinction (include/vpt.h: vpt_scene_set_volgrid_color) -----------------------------------------------------
// sigma_c(p) = k_c rho(p) / trdepth with k_c = -log(clamp(color_c, 1e-4, 1)), the density of the reference's homogeneous medium
// (eval_material).  Within an instance the channels differ by constants: the carrier kmax rho / trdepth is a grey medium of
// trdepth / kmax, flown by the grey free flight, and a carrier collision is real for channel c with probability a_c = k_c / kmax.
struct vpt_volgrid_chroma {
  float a[3];   // k_c / kmax in [0, 1]; exactly 1 for the largest channel; 0 for a transparent instance
  float kmax;   // max_c k_c; 0: the instance is transparent
};
static_assert(sizeof(vpt_volgrid_chroma) == 16, "a chroma row is one float4");
// what vpt_scene_get_volgrid_chroma and vpth_volgrid_chroma answer per grid instance: the chroma row and what the coloured record holds
struct vpt_volgrid_chroma_row {
  float   a[3], kmax;
  float   trdepth_eff;   // trdepth / kmax; the material's trdepth for a transparent instance
  int32_t whd[3];        // the coloured record's: 0 for a transparent instance
};
static_assert(sizeof(vpt_volgrid_chroma_row) == 32, "a chroma read-back row");

// Made on the host only (device and mirror hold the same logf).  clamp = min(max(x, lo), hi) with the ternaries of yocto_math.h (NaN: lo);
// k_c = 0 - logf(.), so that colour 1 gives +0; kmax by `k > kmax ? k : kmax` from 0; a_c = k_c / kmax, one division each
inline vpt_volgrid_chroma vpt_volgrid_make_chroma(const vpt_material& mat) {
  vpt_volgrid_chroma ch = {{0.0f, 0.0f, 0.0f}, 0.0f};
  float k[3];
  for (int c = 0; c < 3; c++) {
    float x = mat.color[c];
    x       = x > 0.0001f ? x : 0.0001f;
    x       = x < 1.0f ? x : 1.0f;
    k[c]    = 0.0f - logf(x);
    ch.kmax = k[c] > ch.kmax ? k[c] : ch.kmax;
  }
  for (int c = 0; c < 3; c++) ch.a[c] = ch.kmax > 0.0f ? k[c] / ch.kmax : 0.0f;
  return ch;
}
// The coloured record: the grey one with the carrier's trdepth (one float32 division).  A transparent instance (kmax == 0, or a carrier
// trdepth that is not finite) gets whd = 0 and keeps the material's trdepth: the box clip of the free flight misses it without a draw
inline vpt_volgrid_record vpt_volgrid_make_color_record(const vpt_volume_instance& vi, const vpt_volume& vol, const vpt_material& mat, int brick_offset,
    const vpt_volgrid_chroma& ch) {
  vpt_volgrid_record r   = vpt_volgrid_make_record(vi, vol, mat, brick_offset);
  const float        eff = ch.kmax > 0.0f ? r.trdepth / ch.kmax : 0.0f;
  if (vpt_volgrid_trdepth_ok(eff)) r.trdepth = eff;
  else r.whd[0] = r.whd[1] = r.whd[2] = 0;
  return r;
}
inline vpt_volgrid_chroma_row vpt_volgrid_make_chroma_row(const vpt_volgrid_chroma& ch, const vpt_volgrid_record& color_rec) {
  return {{ch.a[0], ch.a[1], ch.a[2]}, ch.kmax, color_rec.trdepth, {color_rec.whd[0], color_rec.whd[1], color_rec.whd[2]}};
}

// The event at a carrier collision with path weight w (history-aware probabilities, Kutz et al. 2017) - THIS IS ITS OPERATION ORDER:
//   s = max(max(w0 a0, w1 a1), w2 a2)     n = max(max(w0 (1 - a0), w1 (1 - a1)), w2 (1 - a2))
//   not (s + n > 0): END (weights all zero, or a sum that is not a number; `>` drops a NaN product, the path's own finite check ends those)
//   P = s / (s + n)
//   n == 0, or u < P: SCATTER, w_c = w_c * (a_c / P)       else: PASS, w_c = w_c * ((1 - a_c) / (1 - P))
// With n == 0 (equal channels among them) P is s / s = 1 and a_c / 1 = a_c: the same formula, and u is not read - the caller draws none
// (vpt_volgrid_event_draws).  P rounds to 1 only where u < P always holds, so 1 - P is never 0 on the PASS side.
enum { VPT_VOLGRID_PASS = 0, VPT_VOLGRID_SCATTER = 1, VPT_VOLGRID_END = 2 };
VPT_VOLGRID_HD void vpt_volgrid_event_sn(const float a[3], const float w[3], float& s, float& n) {
  const float s0 = w[0] * a[0], s1 = w[1] * a[1], s2 = w[2] * a[2];
  const float n0 = w[0] * (1.0f - a[0]), n1 = w[1] * (1.0f - a[1]), n2 = w[2] * (1.0f - a[2]);
  s = s0 > s1 ? s0 : s1, s = s > s2 ? s : s2;
  n = n0 > n1 ? n0 : n1, n = n > n2 ? n : n2;
}
// whether the event reads a random number
VPT_VOLGRID_HD bool vpt_volgrid_event_draws(const float a[3], const float w[3]) {
  float s, n;
  vpt_volgrid_event_sn(a, w, s, n);
  return s + n > 0.0f && n != 0.0f;
}
// the event; out (may alias w) receives the weight after it, unchanged on END; prob (nullable) receives P
VPT_VOLGRID_HD int vpt_volgrid_event(const float a[3], const float w[3], float u, float out[3], float* prob) {
  float s, n;
  vpt_volgrid_event_sn(a, w, s, n);
  if (prob) *prob = 0.0f;
  if (!(s + n > 0.0f)) {
    out[0] = w[0], out[1] = w[1], out[2] = w[2];
    return VPT_VOLGRID_END;
  }
  const float P = s / (s + n);
  if (prob) *prob = P;
  if (n == 0.0f || u < P) {
    out[0] = w[0] * (a[0] / P), out[1] = w[1] * (a[1] / P), out[2] = w[2] * (a[2] / P);
    return VPT_VOLGRID_SCATTER;
  }
  const float q = 1.0f - P;
  out[0] = w[0] * ((1.0f - a[0]) / q), out[1] = w[1] * ((1.0f - a[1]) / q), out[2] = w[2] * ((1.0f - a[2]) / q);
  return VPT_VOLGRID_PASS;
}

// ---- next-event estimation (include/vpt.h: vpt_scene_set_volgrid_nee) -----------------------------------------------------
// One tentative collision of a ratio-tracked shadow flight: `real` = min(sigma / m, 1), the probability that a delta-tracking flight would
// have taken it for real, is the share of the flight's weight that stops here.  One subtraction, one product; real == 1 gives exactly 0
VPT_VOLGRID_HD float vpt_volgrid_ratio_step(float T, float real) { return T * (1.0f - real); }

// ---- the first-collision pass (include/vpt.h: vpt_render_volgrid_aov_device): the collision cell and the density's gradient in it ----------
// The eight nodes of the cell eval_volume reads at node coordinates (s, t, r), each through clean(), in the order v000 v100 v010 v001 v011
// v101 v110 v111 of the trilerp above, and the fractions (u, v, w) inside it: one fetch for the whole gradient
VPT_VOLGRID_HD void vpt_volgrid_cell(const float* vox, int W, int H, int D, float s, float t, float r, float node[8], float uvw[3]) {
  int i = (int)s, j = (int)t, k = (int)r;
  i = i > 0 ? (i < W - 1 ? i : W - 1) : 0, j = j > 0 ? (j < H - 1 ? j : H - 1) : 0, k = k > 0 ? (k < D - 1 ? k : D - 1) : 0;
  const int ii = i + 1 < W - 1 ? i + 1 : W - 1, jj = j + 1 < H - 1 ? j + 1 : H - 1, kk = k + 1 < D - 1 ? k + 1 : D - 1;
  uvw[0] = s - i, uvw[1] = t - j, uvw[2] = r - k;
  const int WH = W * H, r0 = j * W + k * WH, r1 = jj * W + k * WH, r2 = j * W + kk * WH, r3 = jj * W + kk * WH;
  node[0] = vpt_volgrid_clean(vox[i + r0]), node[1] = vpt_volgrid_clean(vox[ii + r0]);
  node[2] = vpt_volgrid_clean(vox[i + r1]), node[3] = vpt_volgrid_clean(vox[i + r2]);
  node[4] = vpt_volgrid_clean(vox[i + r3]), node[5] = vpt_volgrid_clean(vox[ii + r2]);
  node[6] = vpt_volgrid_clean(vox[ii + r1]), node[7] = vpt_volgrid_clean(vox[ii + r3]);
}
// The analytic derivative of the trilerp of those eight nodes inside the cell, per unit of node coordinate: along x the four edge
// differences weighted bilinearly in (v, w), and so on - THIS IS THE TERM ORDER.  A cell on the last node plane of an axis (ii == i) has
// a zero difference along it.
VPT_VOLGRID_HD void vpt_volgrid_cell_gradient(const float n[8], const float uvw[3], float grad[3]) {
  const float u = uvw[0], v = uvw[1], w = uvw[2];
  grad[0] = ((n[1] - n[0]) * (1 - v) * (1 - w) + (n[6] - n[2]) * v * (1 - w)) + ((n[5] - n[3]) * (1 - v) * w + (n[7] - n[4]) * v * w);
  grad[1] = ((n[2] - n[0]) * (1 - u) * (1 - w) + (n[6] - n[1]) * u * (1 - w)) + ((n[4] - n[3]) * (1 - u) * w + (n[7] - n[5]) * u * w);
  grad[2] = ((n[3] - n[0]) * (1 - u) * (1 - v) + (n[5] - n[1]) * u * (1 - v)) + ((n[4] - n[2]) * (1 - u) * v + (n[7] - n[6]) * u * v);
}
// The world gradient of a grid instance's voxel value from the cell gradient: per axis times (whd - 1) / bbox (node coordinates per unit
// of the box), then the transpose of the frame's rotation (local = frame * world), summed from the left
VPT_VOLGRID_HD void vpt_volgrid_world_gradient(const vpt_volgrid_record& rec, const float cell_grad[3], float grad[3]) {
  float gl[3];
  for (int k = 0; k < 3; k++) gl[k] = cell_grad[k] * ((float)(rec.whd[k] - 1) / rec.bbox[k]);
  const float* f = rec.frame;
  grad[0] = (gl[0] * f[0] + gl[1] * f[1]) + gl[2] * f[2];
  grad[1] = (gl[0] * f[3] + gl[1] * f[4]) + gl[2] * f[5];
  grad[2] = (gl[0] * f[6] + gl[1] * f[7]) + gl[2] * f[8];
}
// n = -normalize(grad); a gradient of length 0, or one that is not finite (its length included), gives n = 0
VPT_VOLGRID_HD void vpt_volgrid_normal_of(const float grad[3], float n[3]) {
  const float len = sqrtf((grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2]);
  const bool  ok  = len > 0.0f && len <= 3.402823466e+38f;   // NaN: not ok
  for (int k = 0; k < 3; k++) n[k] = ok ? -(grad[k] / len) : 0.0f;
}
// The pass's normal of grid instance `rec` at a world point and the world gradient behind it (nullable): false, n = 0 and gradient 0
// outside the box.  The eight voxels of the cell are fetched once
VPT_VOLGRID_HD bool vpt_volgrid_normal(const vpt_volgrid_record& rec, const float* voxels, float px, float py, float pz, float n[3], float* grad_out) {
  float node[3], grad[3] = {0.0f, 0.0f, 0.0f};
  const bool inside = vpt_volgrid_locate(rec, px, py, pz, node);
  if (inside) {
    float cell[8], uvw[3], cg[3];
    vpt_volgrid_cell(voxels + rec.voxel_offset, rec.whd[0], rec.whd[1], rec.whd[2], node[0], node[1], node[2], cell, uvw);
    vpt_volgrid_cell_gradient(cell, uvw, cg);
    vpt_volgrid_world_gradient(rec, cg, grad);
  }
  vpt_volgrid_normal_of(grad, n);
  if (grad_out) grad_out[0] = grad[0], grad_out[1] = grad[1], grad_out[2] = grad[2];
  return inside;
}
