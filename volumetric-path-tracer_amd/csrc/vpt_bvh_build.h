// vpt_bvh_build.h — the core of the device BVH build (vpt_bvh_build.hip): boxes that are on the device in, nodes and primitive
// order that stay on the device out.  vpt_build_bvh (include/vpt.h) wraps it with its copies from and to the host;
// vpt_scene_rebuild_bvh (vpt_bvh_rebuild.hip) runs it on boxes made from the resident tables.
#pragma once
#include <cstddef>

#include "vpt_device_buffer.h"

// The build's working buffers.  reserve(n) sizes them for a build of up to n boxes; builds of fewer boxes reuse them, so a call
// that builds several BVHs reserves once, for the largest.
struct bvh_build_scratch {
  // quality VPT_BVH_SAH adds the bins of the SAH search (1344 B per five boxes); a build at VPT_BVH_MIDDLE never allocates them
  int reserve(int max_boxes, int quality = VPT_BVH_MIDDLE);
  // the result of the last bvh_build_core: `count` nodes in the reference's order, the primitive order (n entries)
  const vpt_bvh_node* nodes() const { return out.get<vpt_bvh_node>(); }
  const int*          primitives() const { return prims.get<int>(); }

  int           reserved = -1, sah_reserved = -1;
  size_t        scan_bytes = 0;
  device_buffer ctr, boxes, prims, node_of, flag, tscan, partner, counter, tnodes, keys, out, scan_temp;
  device_buffer sah_bins, sah_info, sah_slot;   // the SAH search: bins and borders per splitting node of a level, the slot of every node
};

// build_bvh(bvh, bboxes, highquality = quality) over n boxes on the current device, null stream.  Box i is the six floats
// {min.xyz, max.xyz} at d_boxes + stride * i (stride in floats, >= 6).  n == 0 gives the reference's root of an empty build.
// *count = the number of nodes; *launches (may be null) is increased by the kernels launched.  The host waits for every level
// (one counter read back per level), so the result is complete when the call returns.  quality: VPT_BVH_MIDDLE (split_middle) or
// VPT_BVH_SAH (split_sah: include/vpt.h, vpt_build_bvh_quality); another value is VPT_ERR_INVALID_ARG.
int bvh_build_core(bvh_build_scratch& s, const float* d_boxes, int stride, int n, int* count, int* launches = nullptr, int quality = VPT_BVH_MIDDLE);
