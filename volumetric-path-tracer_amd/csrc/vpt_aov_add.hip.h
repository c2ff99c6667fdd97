// vpt_aov_add.hip.h — how a first-hit pass updates a sum plane (vpt_aov_kernel.hip.h: the mesh pass; vpt_sdf_aov_kernel.hip.h: the
// sphere-traced one): one rule for both, so that a plane of either has the bits of `image` under the matching shader.
#pragma once
#include "vpt_math.hip.h"

// one sample's value into a sum plane; a value that is not finite counts as zeros (K1's finish, cpp:1087-1089), decided per plane
VPT_DEV void aov_add(float4* __restrict__ plane, int slot, f3 v, float alpha) {
  f4 rad = mk4(v.x, v.y, v.z, alpha);
  if (!(isfinite(rad.x) && isfinite(rad.y) && isfinite(rad.z) && isfinite(rad.w))) rad = mk4(0, 0, 0, 0);
  const float4 a = plane[slot];
  plane[slot] = make_float4(a.x + rad.x, a.y + rad.y, a.z + rad.z, a.w + rad.w);
}
