// vpt_bake_rule.h — the rule of vpt_bake_sdf (include/vpt.h), written once: the closest point of a triangle, the squared distance,
// the order among candidates and the signed value.  Compiled by the bake kernel (csrc/vpt_bake.hip) and by the host mirror
// (host/vpt_bake.cpp), both with -ffp-contract=off: float32 throughout, nothing fused, every sum in the order written here, the three
// quotients and the square root IEEE operations - so both give the same bits, and THIS FILE IS THE CONTRACT'S OPERATION ORDER.
//
// Closest point: the seven-region test of Ericson, Real-Time Collision Detection, section 5.1.5, regions in the book's order (vertex A,
// vertex B, edge AB, vertex C, edge AC, edge BC, face) with the book's comparisons (<= 0, >= 0).  The region names the feature whose
// pseudonormal (Baerentzen & Aanaes, "Signed distance computation using the angle weighted pseudonormal", 2005) gives the sign.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define VPT_BAKE_HD __host__ __device__ inline
#else
#define VPT_BAKE_HD inline
#endif

// one kept triangle as both sides read it: 32 words
struct alignas(16) vpt_bake_record {
  float   a[3], b[3], c[3];
  float   normals[21];   // vpt_bake_feature_normals: face, edge ab, edge bc, edge ca, vertex a, vertex b, vertex c
  int32_t index;         // the triangle's index in the caller's array
};

// the feature a closest point lies on, in the order of the normals
enum { VPT_BAKE_FACE = 0, VPT_BAKE_EDGE_AB = 1, VPT_BAKE_EDGE_BC = 2, VPT_BAKE_EDGE_CA = 3, VPT_BAKE_VERTEX_A = 4, VPT_BAKE_VERTEX_B = 5, VPT_BAKE_VERTEX_C = 6 };

struct vpt_bake_f3 {
  float x, y, z;
};

VPT_BAKE_HD float vpt_bake_dot(vpt_bake_f3 u, vpt_bake_f3 v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
VPT_BAKE_HD vpt_bake_f3 vpt_bake_sub(vpt_bake_f3 u, vpt_bake_f3 v) { return {u.x - v.x, u.y - v.y, u.z - v.z}; }
// u + v * t
VPT_BAKE_HD vpt_bake_f3 vpt_bake_along(vpt_bake_f3 u, vpt_bake_f3 v, float t) { return {u.x + v.x * t, u.y + v.y * t, u.z + v.z * t}; }

// the sample point of voxel i along one axis
VPT_BAKE_HD float vpt_bake_sample(float origin, float step, int i) { return origin + (float)i * step; }

// (b - a) x (c - a); a triangle for which this is exactly {0, 0, 0} is dropped
VPT_BAKE_HD vpt_bake_f3 vpt_bake_cross(vpt_bake_f3 a, vpt_bake_f3 b, vpt_bake_f3 c) {
  vpt_bake_f3 u = vpt_bake_sub(b, a), v = vpt_bake_sub(c, a);
  return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}

// the point of triangle (a, b, c) closest to p; *feature: where it lies
VPT_BAKE_HD vpt_bake_f3 vpt_bake_closest(vpt_bake_f3 p, vpt_bake_f3 a, vpt_bake_f3 b, vpt_bake_f3 c, int* feature) {
  vpt_bake_f3 ab = vpt_bake_sub(b, a), ac = vpt_bake_sub(c, a), ap = vpt_bake_sub(p, a);
  float d1 = vpt_bake_dot(ab, ap), d2 = vpt_bake_dot(ac, ap);
  if (d1 <= 0.0f && d2 <= 0.0f) return *feature = VPT_BAKE_VERTEX_A, a;
  vpt_bake_f3 bp = vpt_bake_sub(p, b);
  float d3 = vpt_bake_dot(ab, bp), d4 = vpt_bake_dot(ac, bp);
  if (d3 >= 0.0f && d4 <= d3) return *feature = VPT_BAKE_VERTEX_B, b;
  float vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
    float v = d1 / (d1 - d3);
    return *feature = VPT_BAKE_EDGE_AB, vpt_bake_along(a, ab, v);
  }
  vpt_bake_f3 cp = vpt_bake_sub(p, c);
  float d5 = vpt_bake_dot(ab, cp), d6 = vpt_bake_dot(ac, cp);
  if (d6 >= 0.0f && d5 <= d6) return *feature = VPT_BAKE_VERTEX_C, c;
  float vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
    float w = d2 / (d2 - d6);
    return *feature = VPT_BAKE_EDGE_CA, vpt_bake_along(a, ac, w);
  }
  float va = d3 * d6 - d5 * d4;
  if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {
    float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    return *feature = VPT_BAKE_EDGE_BC, vpt_bake_along(b, vpt_bake_sub(c, b), w);
  }
  float denom = 1.0f / ((va + vb) + vc);
  float v = vb * denom, w = vc * denom;
  *feature = VPT_BAKE_FACE;
  return {(a.x + ab.x * v) + ac.x * w, (a.y + ab.y * v) + ac.y * w, (a.z + ab.z * v) + ac.z * w};
}

VPT_BAKE_HD vpt_bake_f3 vpt_bake_corner(const float* v) { return {v[0], v[1], v[2]}; }

// squared distance from p to a record's triangle; *side: dot(p - c, n) with n the normal of the feature the closest point c lies on,
// of which only the sign is read.  On an edge or a vertex d2 is |p - c|^2.  On the face it is the square of the height over the
// plane, dot(p - a, unit face normal), which is also the side: there c comes from three areas that cancel (vb / (va + vb + vc)), and
// on a narrow triangle it is off, in the plane, by some 1e-4 of the longest edge - which |p - c| turns into an error of the same
// size for a point close to the face, while the height does not know c.
VPT_BAKE_HD float vpt_bake_measure(vpt_bake_f3 p, const vpt_bake_record& r, float* side) {
  int         feature;
  vpt_bake_f3 a = vpt_bake_corner(r.a);
  vpt_bake_f3 c = vpt_bake_closest(p, a, vpt_bake_corner(r.b), vpt_bake_corner(r.c), &feature);
  if (feature == VPT_BAKE_FACE) {
    float h = vpt_bake_dot(vpt_bake_sub(p, a), vpt_bake_corner(r.normals));
    return *side = h, h * h;
  }
  vpt_bake_f3 q = vpt_bake_sub(p, c);
  *side = vpt_bake_dot(q, vpt_bake_corner(r.normals + 3 * feature));
  return vpt_bake_dot(q, q);
}
VPT_BAKE_HD float vpt_bake_distance2(vpt_bake_f3 p, const vpt_bake_record& r) {
  float side;
  return vpt_bake_measure(p, r, &side);
}

// the winner so far: the lexicographic minimum of (d2, index).  A NaN d2 never wins: both comparisons are false.
struct vpt_bake_best {
  float   d2;
  int32_t index;   // the caller's triangle index
  int32_t slot;    // where its record lies
};
VPT_BAKE_HD vpt_bake_best vpt_bake_none() { return {INFINITY, INT32_MAX, -1}; }
VPT_BAKE_HD void vpt_bake_offer(vpt_bake_best& best, float d2, int32_t index, int32_t slot) {
  if (d2 < best.d2 || (d2 == best.d2 && index < best.index)) best.d2 = d2, best.index = index, best.slot = slot;
}

// the value of a voxel for which no candidate won (every d2 was NaN)
VPT_BAKE_HD float vpt_bake_no_winner() { return INFINITY; }
// the voxel's value from the winning record: sign by the pseudonormal of the feature the closest point lies on
VPT_BAKE_HD float vpt_bake_value(vpt_bake_f3 p, const vpt_bake_record& r) {
  float side;
  float d2 = vpt_bake_measure(p, r, &side);
  float s  = side < 0.0f ? -1.0f : 1.0f;
  return s * sqrtf(d2);
}

// the record of triangle `index` of a mesh from its row of vpt_bake_feature_normals' table
inline vpt_bake_record vpt_bake_make_record(const float* positions, const int32_t* triangles, const float* normals, int32_t index) {
  vpt_bake_record r;
  const int32_t*  tri = triangles + 3 * (size_t)index;
  for (int k = 0; k < 3; k++) r.a[k] = positions[3 * (size_t)tri[0] + k], r.b[k] = positions[3 * (size_t)tri[1] + k], r.c[k] = positions[3 * (size_t)tri[2] + k];
  for (int k = 0; k < 21; k++) r.normals[k] = normals[21 * (size_t)index + k];
  r.index = index;
  return r;
}
