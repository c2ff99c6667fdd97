// vpt_record_bounds.hip.h — the bounds of the primitive in one leaf record (vpt_device.h), with the select-form min / max of the
// reference (yocto_math.h:1355-1356): shared by the refit and the rebuild (vpt_scene_update.hip), which read records that exist, and
// by vpt_scene_update_shapes (vpt_shape_update.hip), which makes the record first - one function, so the boxes have the same bits.
#pragma once
#include "vpt_device.h"

struct box3 { float lo[3], hi[3]; };
__device__ inline float sel_min(float a, float b) { return (a < b) ? a : b; }   // yocto_math.h:1355-1356: not fminf
__device__ inline float sel_max(float a, float b) { return (a > b) ? a : b; }
// the bounds of the primitive in one leaf record (vpt_device.h): quad_bounds over the four corners (a triangle repeats its last
// corner: min(p2, p2) == p2, the bits of triangle_bounds), point_bounds, line_bounds
__device__ inline box3 record_bounds(const float4* r) {
  float4 p0 = r[0], p1 = r[1], p2 = r[2], p3 = r[3];
  const int kind = __float_as_int(p3.w);
  box3 b;
  if (kind == VPT_LEAF_POINT) {
    const float rad = p1.x;
    const float a[3] = {p0.x - rad, p0.y - rad, p0.z - rad}, c[3] = {p0.x + rad, p0.y + rad, p0.z + rad};
    for (int k = 0; k < 3; k++) b.lo[k] = sel_min(a[k], c[k]), b.hi[k] = sel_max(a[k], c[k]);
  } else if (kind == VPT_LEAF_LINE) {
    const float r0 = p2.x, r1 = p2.y;
    const float a0[3] = {p0.x - r0, p0.y - r0, p0.z - r0}, a1[3] = {p1.x - r1, p1.y - r1, p1.z - r1};
    const float c0[3] = {p0.x + r0, p0.y + r0, p0.z + r0}, c1[3] = {p1.x + r1, p1.y + r1, p1.z + r1};
    for (int k = 0; k < 3; k++) b.lo[k] = sel_min(a0[k], a1[k]), b.hi[k] = sel_max(c0[k], c1[k]);
  } else {
    const float q0[3] = {p0.x, p0.y, p0.z}, q1[3] = {p1.x, p1.y, p1.z}, q2[3] = {p2.x, p2.y, p2.z}, q3[3] = {p3.x, p3.y, p3.z};
    for (int k = 0; k < 3; k++)
      b.lo[k] = sel_min(q0[k], sel_min(q1[k], sel_min(q2[k], q3[k]))), b.hi[k] = sel_max(q0[k], sel_max(q1[k], sel_max(q2[k], q3[k])));
  }
  return b;
}
