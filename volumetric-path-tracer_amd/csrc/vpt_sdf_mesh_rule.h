// vpt_sdf_mesh_rule.h — the rule of vpt_mesh_sdf / vpt_scene_mesh_volume (include/vpt.h), written once: which cells and grid edges of a
// signed-distance voxel grid carry the surface, the vertex and the normal of an active cell, and the order of a quad's corners (naive
// surface nets, quads out).  Compiled by the kernels (csrc/vpt_sdf_mesh.hip) and by the host mirror (host/vpt_sdf_mesh.cpp), both with
// -ffp-contract=off: float32 throughout, nothing fused, every sum in the order written here, the quotients and the square root IEEE
// operations - so both give the same bits, and THIS FILE IS THE CONTRACT'S OPERATION ORDER.
//
// Ids and order (a vertex's id is the rank of its cell among the active cells in voxel index order, a quad's place the rank of its
// grid edge by owner voxel, then axis) are integer facts of the flags below: each side counts them in its own way.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "vpt.h"

#if defined(__HIPCC__)
#define VPT_SDF_MESH_HD __host__ __device__ inline
#define VPT_SDF_MESH_UNROLL _Pragma("unroll")   // the corner array stays in registers only if its indices are constants
#else
#define VPT_SDF_MESH_HD inline
#define VPT_SDF_MESH_UNROLL
#endif

struct vpt_sdf_mesh_f3 {
  float x, y, z;
};

// what one voxel owns, one byte: its cell (the eight corners (x + dx, y + dy, z + dz), where x < W - 1, y < H - 1, z < D - 1) and its three
// grid edges (to x + 1, y + 1, z + 1)
constexpr unsigned VPT_SDF_MESH_ACTIVE = 1;   // between 1 and 7 corners of the cell are inside: the cell has a vertex
constexpr unsigned VPT_SDF_MESH_QUAD   = 2;   // << axis: the edge along `axis` changes sign and has four cells around it: it emits a quad
constexpr unsigned VPT_SDF_MESH_FLIP   = 16;  // << axis: the edge's UPPER end is inside (the quad's last three corners are reversed)

// a NaN voxel is outside
VPT_SDF_MESH_HD bool vpt_sdf_mesh_inside(float v, float iso) { return v < iso; }

// the corners of a cell are c[dx + 2 * dy + 4 * dz]; bit k of the mask: corner k is inside
VPT_SDF_MESH_HD unsigned vpt_sdf_mesh_mask(const float c[8], float iso) {
  unsigned mask = 0;
  VPT_SDF_MESH_UNROLL
  for (int k = 0; k < 8; k++) mask |= (vpt_sdf_mesh_inside(c[k], iso) ? 1u : 0u) << k;
  return mask;
}
VPT_SDF_MESH_HD bool vpt_sdf_mesh_active(unsigned mask) { return mask != 0 && mask != 255; }

// the quad bits of the edge from voxel X (value v0, position p[3] in a grid of dim[3]) along `axis` to the voxel of value v1, which exists.
// (a, b, c) a cyclic permutation of (x, y, z): the four cells X - e_b - e_c, X - e_c, X, X - e_b exist when 1 <= X_b <= dim_b - 2 and the
// same for c.  An edge on the border of the grid emits nothing.
VPT_SDF_MESH_HD unsigned vpt_sdf_mesh_edge_bits(int axis, const int p[3], const int dim[3], float v0, float v1, float iso) {
  const int  b = (axis + 1) % 3, c = (axis + 2) % 3;
  const bool in0 = vpt_sdf_mesh_inside(v0, iso), in1 = vpt_sdf_mesh_inside(v1, iso);
  if (in0 == in1 || p[b] < 1 || p[b] > dim[b] - 2 || p[c] < 1 || p[c] > dim[c] - 2) return 0;
  return (VPT_SDF_MESH_QUAD << axis) | (in1 ? VPT_SDF_MESH_FLIP << axis : 0u);
}

// where the edge from the lower corner (value va) to the upper one (vb) crosses iso, as a parameter in [0, 1]; 0.5f for anything else
// (infinite ends, an overflowing difference)
VPT_SDF_MESH_HD float vpt_sdf_mesh_crossing(float va, float vb, float iso) {
  const float t = (iso - va) / (vb - va);
  return (t >= 0.0f && t <= 1.0f) ? t : 0.5f;
}

// The vertex of an active cell in unit-cell coordinates: the mean of the crossing points of its edges.  The twelve edges in order: the four
// x-edges at (dy, dz) = (0,0), (1,0), (0,1), (1,1), the four y-edges at (dz, dx) in the same order, the four z-edges at (dx, dy).  A
// crossing point is t along the edge's axis and the edge's 0 / 1 offsets on the two others; each coordinate is summed from 0 in edge order
// and divided by (float)count.
VPT_SDF_MESH_HD vpt_sdf_mesh_f3 vpt_sdf_mesh_cell_vertex(const float c[8], float iso) {
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  int   count = 0;
  VPT_SDF_MESH_UNROLL
  for (int e = 0; e < 12; e++) {
    const int axis = e >> 2, p = e & 1, q = (e >> 1) & 1;   // p, q: the offsets on the next and the next-but-one axis, cyclically
    // strides of the three axes in c[]: 1, 2, 4
    const int sa = 1 << axis, sb = 1 << ((axis + 1) % 3), sc = 1 << ((axis + 2) % 3);
    const int lower = p * sb + q * sc;
    const float va = c[lower], vb = c[lower + sa];
    if (vpt_sdf_mesh_inside(va, iso) == vpt_sdf_mesh_inside(vb, iso)) continue;
    const float t = vpt_sdf_mesh_crossing(va, vb, iso);
    const float fp = (float)p, fq = (float)q;
    if (axis == 0) sx = sx + t, sy = sy + fp, sz = sz + fq;
    else if (axis == 1) sy = sy + t, sz = sz + fp, sx = sx + fq;
    else sz = sz + t, sx = sx + fp, sy = sy + fq;
    count++;
  }
  const float n = (float)count;   // >= 3 in an active cell
  return {sx / n, sy / n, sz / n};
}

// the position along one axis of the vertex of cell i (its index in the grid the descriptor's origin belongs to): add, multiply, add
VPT_SDF_MESH_HD float vpt_sdf_mesh_position(float origin, float step, int i, float u) { return origin + ((float)i + u) * step; }

// The normal: the gradient of the cell's trilinear interpolant at u, each component divided by its step, then the reference's normalize
// (yocto_math.h: l = sqrt(x * x + y * y + z * z) summed from the left, v / l if l != 0, else v).  A component that comes out NaN (voxels
// that are NaN or infinite) is written as +0: the sign and payload of a NaN are the one thing the two sides' hardware does not agree on.
VPT_SDF_MESH_HD vpt_sdf_mesh_f3 vpt_sdf_mesh_normal(const float c[8], vpt_sdf_mesh_f3 u, const float step[3]) {
  const float ax = 1.0f - u.x, ay = 1.0f - u.y, az = 1.0f - u.z;
  // d/dx: the four x-edges' differences, blended along y, then along z; the others alike
  const float gx = ((c[1] - c[0]) * ay + (c[3] - c[2]) * u.y) * az + ((c[5] - c[4]) * ay + (c[7] - c[6]) * u.y) * u.z;
  const float gy = ((c[2] - c[0]) * ax + (c[3] - c[1]) * u.x) * az + ((c[6] - c[4]) * ax + (c[7] - c[5]) * u.x) * u.z;
  const float gz = ((c[4] - c[0]) * ax + (c[5] - c[1]) * u.x) * ay + ((c[6] - c[2]) * ax + (c[7] - c[3]) * u.x) * u.y;
  float nx = gx / step[0], ny = gy / step[1], nz = gz / step[2];
  const float l = sqrtf((nx * nx + ny * ny) + nz * nz);
  if (l != 0) nx = nx / l, ny = ny / l, nz = nz / l;
  return {nx == nx ? nx : 0.0f, ny == ny ? ny : 0.0f, nz == nz ? nz : 0.0f};
}

// The corners of the quad of the edge from voxel X along `axis`, as offsets to X's index: the cells X - e_b - e_c, X - e_c, X, X - e_b in
// that order when X is inside; when X + e_a is inside the first is kept and the other three are reversed.  stride[3]: the index strides of
// the three axes (1, W, W * H).
VPT_SDF_MESH_HD void vpt_sdf_mesh_quad_cells(int axis, bool flip, const long long stride[3], long long out[4]) {
  const long long sb = stride[(axis + 1) % 3], sc = stride[(axis + 2) % 3];
  out[0] = -sb - sc, out[1] = flip ? -sb : -sc, out[2] = 0, out[3] = flip ? -sc : -sb;
}

// ---- what both sides refuse, in the same words ------------------------------------------------------------------------------------
// null, or what is wrong with the descriptor
inline const char* vpt_sdf_mesh_desc_fault(const vpt_sdf_mesh_desc& d) {
  long long n = 1;
  for (int k = 0; k < 3; k++) {
    if (d.whd[k] < 1) return "whd must be >= 1 on every axis";
    n *= d.whd[k];
    if (n >= (1ll << 31)) return "whd has 2^31 voxels or more";
  }
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(d.origin[k]) || !std::isfinite(d.step[k])) return "origin or step is not finite";
  if (!std::isfinite(d.iso)) return "iso is not finite";
  for (int k = 0; k < 3; k++)
    if (!(d.step[k] > 0)) return "step must be > 0 on every axis";
  return nullptr;
}
// null, or what is wrong with the region of a grid of whd: a box of at least no voxels inside the grid
inline const char* vpt_sdf_mesh_region_fault(const vpt_sdf_mesh_region& r, const int32_t whd[3]) {
  for (int k = 0; k < 3; k++)
    if (r.lo[k] < 0 || r.whd[k] < 0 || (long long)r.lo[k] + r.whd[k] > whd[k]) return "the region leaves the grid";
  return nullptr;
}
