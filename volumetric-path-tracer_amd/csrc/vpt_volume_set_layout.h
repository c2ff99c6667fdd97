// vpt_volume_set_layout.h — the integer half of vpt_scene_update_volume_set (include/vpt.h): the new volume list with its
// offsets, the renumbering of the three lists and the segment table of the gather that fills the new voxel pool.  Plain C++ over no
// HIP header and with no device call, so that it can be read and debugged on a machine without a device.
#pragma once
#include <cstdint>
#include <vector>

#include "vpt.h"

// where one run of the new pool comes from
enum { VOL_SEG_OLD_POOL = 0, VOL_SEG_STAGING = 1, VOL_SEG_CONSTANT = 2, VOL_SEG_BAKE = 3 };
// `length` voxels from `dst` on: copied from the old pool or from the edit's staging buffer at `src`, set to the bits in `src`
// (CONSTANT), or left for the bake kernel that follows the gather.  32 bytes, as the device reads it.
struct vol_segment {
  long long dst, length;
  int       kind, pad;
  long long src;
};

struct volume_set_plan {
  bool                    moves_pool = false;   // a volume is added or removed: the pool is laid out anew
  std::vector<vpt_volume> volumes;              // the new list; moves_pool: offsets are the running sum of W*H*D
  long long               num_voxels = 0;       // of the pool after the edit
  // old id -> new id, -1: removed
  std::vector<int> new_volume, new_vol_instance, new_sdf;
  // moves_pool: the runs of the new pool in order of dst, none empty, touching end to start from 0 to num_voxels
  std::vector<vol_segment> segments;
  std::vector<long long>   added_offset;        // per entry of edit.add_volumes: where its grid starts in the new pool
};

// The plan of `e` over the lists as they are (old_volumes with the offsets of the resident pool of old_num_voxels).  The edit is the
// caller's checked one: ids in range and not repeated, whd >= 0 with products below 2^31, the total below 2^62, sources known,
// copy_of in range, offsets inside the payload.
void volume_set_plan_make(const std::vector<vpt_volume>& old_volumes, long long old_num_voxels, int num_old_vol_instances, int num_old_sdfs,
    const vpt_volume_set_edit& e, volume_set_plan& out);

// whd >= 0 with a product below 2^31, factor by factor: every partial product stays below 2^62, so nothing overflows on the way
bool volume_whd_ok(const int32_t whd[3]);
inline long long volume_voxels(const int32_t whd[3]) { return (long long)whd[0] * whd[1] * whd[2]; }   // of a whd that is ok
