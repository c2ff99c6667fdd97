// vpt_filter_rule.h — the rule of vpt_scene_filter_volumes (include/vpt.h), written once: the remap of a voxel, one pass of the separable
// blur at a node, and the fractal value noise at a sample point.  Compiled by the filter kernels (csrc/vpt_filter.hip) and by the host
// mirror (host/vpt_filter.cpp), both with -ffp-contract=off: float32 throughout, nothing fused, every sum in the order written here, the
// quotient an IEEE operation - so both give the same bits, and THIS FILE IS THE CONTRACT'S OPERATION ORDER.  No libm function but
// floorf, which is exact on both sides; the noise is integer arithmetic up to the lattice values.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "vpt.h"

#if defined(__HIPCC__)
#define VPT_FILTER_HD __host__ __device__ inline
#else
#define VPT_FILTER_HD inline
#endif

// one op as both sides read it: VPT_FILTER_RECORD_BYTES, made on the host by vpt_filter_make_record
struct alignas(16) vpt_filter_record {
  int32_t  type, count;   // count: BLUR the radius, NOISE the octaves
  uint32_t seed;
  int32_t  unused;
  float    p[8];          // REMAP {divisor, scale, offset, lo, hi}; BLUR w[0..R]; NOISE {gain, frequency[3], persistence}
};
static_assert(sizeof(vpt_filter_record) == VPT_FILTER_RECORD_BYTES, "include/vpt.h states the size of an op record");

// the sample point of voxel i along one axis: the sculpt's rule (csrc/vpt_sculpt_rule.h)
VPT_FILTER_HD float vpt_filter_sample(float origin, float step, int i) { return origin + (float)i * step; }

// A result that is a NaN is stored as THE quiet NaN 0x7fc00000: which NaN an operation returns (the sign of Inf - Inf, whose payload
// survives a sum of two) is the processor's choice and differs between the two sides; that it is one is the arithmetic's.  On the bits,
// so that no compiler may take the two NaNs for the same value.
VPT_FILTER_HD float vpt_filter_one_nan(float s) {
  uint32_t bits;
  memcpy(&bits, &s, 4);
  bits = (bits & 0x7fffffffu) > 0x7f800000u ? 0x7fc00000u : bits;
  memcpy(&s, &bits, 4);
  return s;
}

// ---- REMAP ---------------------------------------------------------------------------------------------------------------------------
VPT_FILTER_HD float vpt_filter_remap(const float* p, float v) {
  float t = v / p[0];
  t       = t * p[1];
  t       = t + p[2];
  t       = t > p[3] ? t : p[3];   // selects: a NaN becomes lo
  t       = t < p[4] ? t : p[4];
  return t;
}

// ---- BLUR: one pass at node `at` of `line`, the values along the pass's axis (line[at - R .. at + R] are read: the caller has clamped) ----
template <int R>
VPT_FILTER_HD float vpt_filter_blur_taps(const float* w, const float* line, int at) {
  float s = w[0] * line[at];
#if defined(__HIPCC__)
#pragma unroll   // the kernel's `line` is a register array: every index a constant
#endif
  for (int i = 1; i <= R; i++) s = s + w[i] * (line[at - i] + line[at + i]);
  return vpt_filter_one_nan(s);
}
VPT_FILTER_HD int vpt_filter_clamp(int i, int n) { return i > 0 ? (i < n - 1 ? i : n - 1) : 0; }   // to [0, n - 1]

// ---- NOISE -----------------------------------------------------------------------------------------------------------------------------
// the hash of a lattice point: multiplies by odd constants, xors and shifts of 32-bit words
VPT_FILTER_HD uint32_t vpt_filter_hash(int32_t ix, int32_t iy, int32_t iz, uint32_t seed) {
  uint32_t h = ((uint32_t)ix * 0x8da6b343u) ^ ((uint32_t)iy * 0xd8163841u) ^ ((uint32_t)iz * 0xcb1ab31fu) ^ (seed * 0x9e3779b9u);
  h ^= h >> 16;
  h *= 0x7feb352du;
  h ^= h >> 15;
  h *= 0x846ca68bu;
  h ^= h >> 16;
  return h;
}
// a lattice value in [0, 1): 24 bits of the hash, both the conversion and the product exact
VPT_FILTER_HD float vpt_filter_lattice(int32_t ix, int32_t iy, int32_t iz, uint32_t seed) {
  return (float)(vpt_filter_hash(ix, iy, iz, seed) >> 8) * 5.9604644775390625e-08f;   // 2^-24
}
VPT_FILTER_HD float vpt_filter_fade(float f) { return (f * f) * (3.0f - 2.0f * f); }
// lattice value noise at (x, y, z), |x|, |y|, |z| < 2^22 + 1 (validation): the eight values of the cell in the term order of
// vpt_volgrid_trilerp (csrc/vpt_volgrid_rule.h)
VPT_FILTER_HD float vpt_filter_vnoise(float x, float y, float z, uint32_t seed) {
  const float   cx = floorf(x), cy = floorf(y), cz = floorf(z);
  const int32_t i = (int32_t)cx, j = (int32_t)cy, k = (int32_t)cz;
  const float   u = vpt_filter_fade(x - cx), v = vpt_filter_fade(y - cy), w = vpt_filter_fade(z - cz);
  const float   v000 = vpt_filter_lattice(i, j, k, seed), v100 = vpt_filter_lattice(i + 1, j, k, seed);
  const float   v010 = vpt_filter_lattice(i, j + 1, k, seed), v001 = vpt_filter_lattice(i, j, k + 1, seed);
  const float   v011 = vpt_filter_lattice(i, j + 1, k + 1, seed), v101 = vpt_filter_lattice(i + 1, j, k + 1, seed);
  const float   v110 = vpt_filter_lattice(i + 1, j + 1, k, seed), v111 = vpt_filter_lattice(i + 1, j + 1, k + 1, seed);
  return v000 * (1 - u) * (1 - v) * (1 - w) + v100 * u * (1 - v) * (1 - w) + v010 * (1 - u) * v * (1 - w) +
         v001 * (1 - u) * (1 - v) * w + v011 * (1 - u) * v * w + v101 * u * (1 - v) * w + v110 * u * v * (1 - w) +
         v111 * u * v * w;
}
VPT_FILTER_HD float vpt_filter_fbm(float qx, float qy, float qz, float persistence, int octaves, uint32_t seed) {
  float sum = 0.0f, a = 1.0f;
  for (int o = 0; o < octaves; o++) {
    sum = sum + a * vpt_filter_vnoise(qx, qy, qz, seed + (uint32_t)o);
    qx = qx * 2.0f, qy = qy * 2.0f, qz = qz * 2.0f;
    a = a * persistence;
  }
  return sum;
}
// p = {gain, frequency[3], persistence} at the sample point (sx, sy, sz)
VPT_FILTER_HD float vpt_filter_noise(const vpt_filter_record& r, float sx, float sy, float sz, float v) {
  return vpt_filter_one_nan(v + r.p[0] * (vpt_filter_fbm(sx * r.p[1], sy * r.p[2], sz * r.p[3], r.p[4], r.count, r.seed) - 0.5f));
}

// one pointwise op (REMAP, NOISE) applied to a voxel's value v at its sample point
VPT_FILTER_HD float vpt_filter_pointwise(const vpt_filter_record& r, float sx, float sy, float sz, float v) {
  return r.type == VPT_FILTER_REMAP ? vpt_filter_remap(r.p, v) : vpt_filter_noise(r, sx, sy, sz, v);
}

inline vpt_filter_record vpt_filter_make_record(const vpt_filter_op& op) {
  vpt_filter_record r = {};
  r.type = op.type, r.count = op.count, r.seed = op.seed;
  for (int k = 0; k < 8; k++) r.p[k] = op.p[k];
  return r;
}

// ---- what both sides refuse, in the same words ------------------------------------------------------------------------------------
inline bool vpt_filter_finite(const float* p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(p[i])) return false;
  return true;
}
// null, or what is wrong with op `op`
inline const char* vpt_filter_op_fault(const vpt_filter_op& op) {
  if (op.type < VPT_FILTER_REMAP || op.type > VPT_FILTER_NOISE) return "type is not one of 0..2";
  if (op.type == VPT_FILTER_BLUR) {
    if (op.count < 1 || op.count > VPT_FILTER_MAX_RADIUS) return "the radius is not one of 1..4";
    if (!vpt_filter_finite(op.p, (size_t)op.count + 1)) return "a weight is not finite";
    return nullptr;
  }
  if (!vpt_filter_finite(op.p, 5)) return "a value is not finite";
  if (op.type == VPT_FILTER_REMAP) {
    if (op.p[0] == 0) return "divisor is 0";
    if (!(op.p[3] <= op.p[4])) return "lo is above hi";
  } else if (op.count < 1 || op.count > VPT_FILTER_MAX_OCTAVES) {
    return "octaves is not one of 1..8";
  }
  return nullptr;
}
constexpr long long VPT_FILTER_MAX_VOXELS = 1ll << 30;   // of one entry's region
// null, or what is wrong with entry `e` for a volume of `whd` in an edit whose ops (each valid) are `ops`; *unsupported: the size guard refused it
inline const char* vpt_filter_entry_fault(const vpt_filter_entry& e, const int32_t whd[3], const vpt_filter_op* ops, int num_ops, bool* unsupported) {
  *unsupported = false;
  for (int k = 0; k < 3; k++)
    if (e.region_lo[k] < 0 || e.region_whd[k] < 0 || (long long)e.region_lo[k] + e.region_whd[k] > whd[k]) return "the region leaves the grid";
  if (e.first_op < 0 || e.num_ops < 0 || (long long)e.first_op + e.num_ops > num_ops) return "the op range leaves the edit's list";
  if (!vpt_filter_finite(e.origin, 3) || !vpt_filter_finite(e.step, 3)) return "origin or step is not finite";
  const long long n = (long long)e.region_whd[0] * e.region_whd[1] * e.region_whd[2];   // inside a grid of fewer than 2^31 voxels
  if (n > VPT_FILTER_MAX_VOXELS) return *unsupported = true, "more than 2^30 voxels in the region: split it";
  if (n == 0) return nullptr;
  // a NOISE op's lattice coordinates stay below 2^22 in magnitude: the sample is monotonic along an axis, so the region's two ends bound it
  for (int s = e.first_op; s < e.first_op + e.num_ops; s++) {
    const vpt_filter_op& op = ops[s];
    if (op.type != VPT_FILTER_NOISE) continue;
    const float last = (float)(1 << (op.count - 1));
    for (int k = 0; k < 3; k++) {
      const float a = vpt_filter_sample(e.origin[k], e.step[k], e.region_lo[k]) * op.p[1 + k] * last;
      const float b = vpt_filter_sample(e.origin[k], e.step[k], e.region_lo[k] + e.region_whd[k] - 1) * op.p[1 + k] * last;
      if (!(std::fabs(a) < 4194304.0f && std::fabs(b) < 4194304.0f)) return "a noise op's coordinates can reach 2^22 at its last octave";
    }
  }
  return nullptr;
}
