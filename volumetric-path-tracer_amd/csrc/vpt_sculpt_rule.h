// vpt_sculpt_rule.h — the rule of vpt_scene_sculpt_volumes (include/vpt.h), written once: the sample point of a voxel, the distance of
// an analytic brush and the combination with the resident value.  Compiled by the sculpt kernel (csrc/vpt_sculpt.hip) and by the host
// mirror (host/vpt_sculpt.cpp), both with -ffp-contract=off: float32 throughout, nothing fused, every sum in the order written here, the
// quotients and the square roots IEEE operations - so both give the same bits, and THIS FILE IS THE CONTRACT'S OPERATION ORDER.
//
// The six distances are the reference's sd_* (yocto_sdfs.h:43-80) as the scene loader binds them (yocto_sceneio.cpp:3684-3730), in the
// reference's term order, with the reference's abs / min / max: the ternaries of yocto_math.h:1354-1356, written out below.  K2's forms
// of the box distances (csrc/vpt_scene.hip.h: the hardware's |x|, v_min, v_max) are NOT used: they agree with these only up to the sign
// of intermediate zeros, and this file has to compile for the host.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "vpt.h"

#if defined(__HIPCC__)
#define VPT_SCULPT_HD __host__ __device__ inline
#else
#define VPT_SCULPT_HD inline
#endif

// one stamp as both sides read it: VPT_SCULPT_RECORD_BYTES, made on the host by vpt_sculpt_make_record
struct alignas(16) vpt_sculpt_record {
  float   frame[12];   // the brush's frame: x, y, z, o
  float   q[4];        // BBOX {thickness, w, h, d}; BOX {whd * 0.5f, 0}; CAPPED_CONE {height, r1, r2, 0}; SPHERE {radius}; TORUS {r1, r2}
  int32_t tag;         // type | op << 8
  float   blend;
  int32_t unused[2];
};
static_assert(sizeof(vpt_sculpt_record) == VPT_SCULPT_RECORD_BYTES, "include/vpt.h states the size of a stamp record");

struct vpt_sculpt_f3 {
  float x, y, z;
};

// abs, min, max of yocto_math.h:1354-1356
VPT_SCULPT_HD float vpt_sculpt_abs(float a) { return a < 0 ? -a : a; }
VPT_SCULPT_HD float vpt_sculpt_min(float a, float b) { return (a < b) ? a : b; }
VPT_SCULPT_HD float vpt_sculpt_max(float a, float b) { return (a > b) ? a : b; }
// length(vec2f), length(vec3f): sqrt(dot(a, a)), the dot products summed from the left
VPT_SCULPT_HD float vpt_sculpt_length2(float x, float y) { return sqrtf(x * x + y * y); }
VPT_SCULPT_HD float vpt_sculpt_length3(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

// the sample point of voxel i along one axis: vpt_bake_sample's rule (csrc/vpt_bake_rule.h)
VPT_SCULPT_HD float vpt_sculpt_sample(float origin, float step, int i) { return origin + (float)i * step; }

// transform_point(frame, p) = frame.x * p.x + frame.y * p.y + frame.z * p.z + frame.o (yocto_math.h), summed from the left
VPT_SCULPT_HD vpt_sculpt_f3 vpt_sculpt_to_local(const float* f, vpt_sculpt_f3 p) {
  return {((f[0] * p.x + f[3] * p.y) + f[6] * p.z) + f[9], ((f[1] * p.x + f[4] * p.y) + f[7] * p.z) + f[10],
      ((f[2] * p.x + f[5] * p.y) + f[8] * p.z) + f[11]};
}

// sd_box(p, b), yocto_sdfs.h:45-49
VPT_SCULPT_HD float vpt_sculpt_sd_box(vpt_sculpt_f3 p, float bx, float by, float bz) {
  const float dx = vpt_sculpt_abs(p.x) - bx, dy = vpt_sculpt_abs(p.y) - by, dz = vpt_sculpt_abs(p.z) - bz;
  return vpt_sculpt_min(vpt_sculpt_max(dx, vpt_sculpt_max(dy, dz)), 0.0f) +
         vpt_sculpt_length3(vpt_sculpt_max(dx, 0.0f), vpt_sculpt_max(dy, 0.0f), vpt_sculpt_max(dz, 0.0f));
}
// one of the three terms of sd_bbox: length(max({a, b, c}, 0)) + min(max(a, max(b, c)), 0)
VPT_SCULPT_HD float vpt_sculpt_bbox_term(float a, float b, float c) {
  return vpt_sculpt_length3(vpt_sculpt_max(a, 0.0f), vpt_sculpt_max(b, 0.0f), vpt_sculpt_max(c, 0.0f)) +
         vpt_sculpt_min(vpt_sculpt_max(a, vpt_sculpt_max(b, c)), 0.0f);
}
// sd_bbox(p, b, e), yocto_sdfs.h:51-63
VPT_SCULPT_HD float vpt_sculpt_sd_bbox(vpt_sculpt_f3 p, float bx, float by, float bz, float e) {
  const float px = vpt_sculpt_abs(p.x) - bx, py = vpt_sculpt_abs(p.y) - by, pz = vpt_sculpt_abs(p.z) - bz;
  const float qx = vpt_sculpt_abs(px + e) - e, qy = vpt_sculpt_abs(py + e) - e, qz = vpt_sculpt_abs(pz + e) - e;
  return vpt_sculpt_min(vpt_sculpt_min(vpt_sculpt_bbox_term(px, qy, qz), vpt_sculpt_bbox_term(qx, py, qz)), vpt_sculpt_bbox_term(qx, qy, pz));
}
// sd_torus(p, r1, r2), yocto_sdfs.h:65-69
VPT_SCULPT_HD float vpt_sculpt_sd_torus(vpt_sculpt_f3 p, float r1, float r2) {
  return vpt_sculpt_length2(vpt_sculpt_length2(p.x, p.z) - r1, p.y) - r2;
}
// sd_capped_cone(p, h, r1, r2), yocto_sdfs.h:71-80
VPT_SCULPT_HD float vpt_sculpt_sd_capped_cone(vpt_sculpt_f3 p, float h, float r1, float r2) {
  const float qx = vpt_sculpt_length2(p.x, p.z), qy = p.y;
  const float k1x = r2, k1y = h;
  const float k2x = r2 - r1, k2y = 2.0f * h;
  const float cax = qx - vpt_sculpt_min(qx, (qy < 0.0f) ? r1 : r2), cay = vpt_sculpt_abs(qy) - h;
  const float t   = vpt_sculpt_min(vpt_sculpt_max(((k1x - qx) * k2x + (k1y - qy) * k2y) / (k2x * k2x + k2y * k2y), 0.0f), 1.0f);
  const float cbx = (qx - k1x) + k2x * t, cby = (qy - k1y) + k2y * t;
  const float s   = (cbx < 0.0f && cay < 0.0f) ? -1.0f : 1.0f;
  return s * sqrtf(vpt_sculpt_min(cax * cax + cay * cay, cbx * cbx + cby * cby));
}

// sdf_data::f of the reference (the lambdas of yocto_sceneio.cpp:3684-3730) at a point of the brush's local frame
VPT_SCULPT_HD float vpt_sculpt_brush_local(const vpt_sculpt_record& r, vpt_sculpt_f3 p) {
  switch (r.tag & 255) {
    case VPT_SDF_BBOX: return vpt_sculpt_sd_bbox(p, r.q[1], r.q[2], r.q[3], r.q[0]);
    case VPT_SDF_BOX: return vpt_sculpt_sd_box({p.x - r.q[0], p.y - r.q[1], p.z - r.q[2]}, r.q[0], r.q[1], r.q[2]);   // sd_box(p - whd * 0.5f, whd * 0.5f)
    case VPT_SDF_CAPPED_CONE: return vpt_sculpt_sd_capped_cone(p, r.q[0], r.q[1], r.q[2]);
    case VPT_SDF_PLANE: return p.y;
    case VPT_SDF_SPHERE: return vpt_sculpt_length3(p.x, p.y, p.z) - r.q[0];
    default: return vpt_sculpt_sd_torus(p, r.q[0], r.q[1]);   // VPT_SDF_TORUS: validation leaves no other type
  }
}
// sdf.f(transform_point(sdf.frame, p)), yocto_sdfs.cpp:21, at a point of the grid's voxel space
VPT_SCULPT_HD float vpt_sculpt_brush(const vpt_sculpt_record& r, vpt_sculpt_f3 p) { return vpt_sculpt_brush_local(r, vpt_sculpt_to_local(r.frame, p)); }

// the polynomial smooth minimum of x and y over the width k > 0
VPT_SCULPT_HD float vpt_sculpt_smin(float x, float y, float k) {
  const float m  = (x < y) ? x : y;
  const float d  = x - y;
  const float ad = d < 0 ? -d : d;
  const float t  = k - ad;
  const float h  = (t > 0 ? t : 0) / k;
  return m - ((h * h) * k) * 0.25f;
}
// a: the resident value, b: the brush distance, k = blend >= 0.  With k == 0 the ops are the selects of the reference's op_union,
// op_subtraction(brush, resident) and op_intersection (yocto_sdfs.h:82-95), never fminf / fmaxf: a NaN resident value is replaced by
// UNION and INTERSECT and kept, with its bits, by SUBTRACT.
VPT_SCULPT_HD float vpt_sculpt_combine(int op, float k, float a, float b) {
  if (op == VPT_SCULPT_REPLACE) return b;
  if (k > 0) {
    if (op == VPT_SCULPT_UNION) return vpt_sculpt_smin(a, b, k);
    if (op == VPT_SCULPT_SUBTRACT) return -vpt_sculpt_smin(b, -a, k);
    return -vpt_sculpt_smin(-a, -b, k);
  }
  if (op == VPT_SCULPT_UNION) return (a < b) ? a : b;
  if (op == VPT_SCULPT_SUBTRACT) return (-b > a) ? -b : a;
  return (a > b) ? a : b;
}
// one stamp applied to a voxel's value v at its sample point p
VPT_SCULPT_HD float vpt_sculpt_stamp_value(const vpt_sculpt_record& r, vpt_sculpt_f3 p, float v) {
  return vpt_sculpt_combine(r.tag >> 8, r.blend, v, vpt_sculpt_brush(r, p));
}

// the record of a stamp (material is not part of it).  BOX folds whd * 0.5f here, by the float multiplication the reference's lambda does.
inline vpt_sculpt_record vpt_sculpt_make_record(const vpt_sculpt_stamp& s) {
  vpt_sculpt_record r = {};
  const float*      f = (const float*)&s.brush.frame;
  for (int k = 0; k < 12; k++) r.frame[k] = f[k];
  if (s.brush.type == VPT_SDF_BOX)
    for (int k = 0; k < 3; k++) r.q[k] = s.brush.whd[k] * 0.5f;
  else
    for (int k = 0; k < 4; k++) r.q[k] = s.brush.p[k];
  r.tag = s.brush.type | (s.op << 8), r.blend = s.blend;
  return r;
}

// ---- what both sides refuse, in the same words ------------------------------------------------------------------------------------
inline bool vpt_sculpt_finite(const float* p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(p[i])) return false;
  return true;
}
// null, or what is wrong with stamp `s`
inline const char* vpt_sculpt_stamp_fault(const vpt_sculpt_stamp& s) {
  if (s.brush.type < 0 || s.brush.type > VPT_SDF_TORUS) return "the brush's type is not one of 0..5";
  if (s.op < VPT_SCULPT_REPLACE || s.op > VPT_SCULPT_INTERSECT) return "op is not one of 0..3";
  if (!vpt_sculpt_finite((const float*)&s.brush.frame, 12) || !vpt_sculpt_finite(s.brush.whd, 3) || !vpt_sculpt_finite(s.brush.p, 4) || !std::isfinite(s.blend))
    return "a value is not finite";
  if (!(s.blend >= 0)) return "blend is negative";
  return nullptr;
}
// the most work one entry may ask of one launch: region voxels x stamps
constexpr long long VPT_SCULPT_MAX_WORK = 1ll << 36;
// null, or what is wrong with entry `e` for a volume of `whd` in an edit of `num_stamps` stamps; *unsupported: the work guard refused it
inline const char* vpt_sculpt_entry_fault(const vpt_sculpt_entry& e, const int32_t whd[3], int num_stamps, bool* unsupported) {
  *unsupported = false;
  for (int k = 0; k < 3; k++)
    if (e.region_lo[k] < 0 || e.region_whd[k] < 0 || (long long)e.region_lo[k] + e.region_whd[k] > whd[k]) return "the region leaves the grid";
  if (e.first_stamp < 0 || e.num_stamps < 0 || (long long)e.first_stamp + e.num_stamps > num_stamps) return "the stamp range leaves the edit's list";
  if (!vpt_sculpt_finite(e.origin, 3) || !vpt_sculpt_finite(e.step, 3)) return "origin or step is not finite";
  const long long n = (long long)e.region_whd[0] * e.region_whd[1] * e.region_whd[2];   // inside a grid of fewer than 2^31 voxels
  if (n > 0 && e.num_stamps > 0 && n > VPT_SCULPT_MAX_WORK / e.num_stamps) return *unsupported = true, "more than 2^36 brush evaluations in one launch: split the stroke";
  return nullptr;
}
