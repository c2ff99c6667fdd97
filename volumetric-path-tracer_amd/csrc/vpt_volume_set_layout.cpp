// vpt_volume_set_layout.cpp — the new lists, the renumbering and the gather's segments of vpt_scene_update_volume_set (vpt_volume_set_layout.h)
#include "vpt_volume_set_layout.h"

#include <cstring>

bool volume_whd_ok(const int32_t v[3]) {
  if (v[0] < 0 || v[1] < 0 || v[2] < 0) return false;
  if (v[0] == 0 || v[1] == 0 || v[2] == 0) return true;
  long long n = 1;
  for (int k = 0; k < 3; k++) {
    n *= v[k];
    if (n >= (1ll << 31)) return false;
  }
  return true;
}

namespace {

// erase: the survivors of `count` entries in order, ids closing up
std::vector<int> renumber(int count, const int32_t* remove_ids, int num_remove) {
  std::vector<int> map((size_t)count, 0);
  for (int i = 0; i < num_remove; i++) map[(size_t)remove_ids[i]] = -1;
  int next = 0;
  for (int& m : map) m = m < 0 ? -1 : next++;
  return map;
}

}  // namespace

void volume_set_plan_make(const std::vector<vpt_volume>& old_volumes, long long old_num_voxels, int num_old_vol_instances, int num_old_sdfs,
    const vpt_volume_set_edit& e, volume_set_plan& out) {
  out = {};
  out.new_volume       = renumber((int)old_volumes.size(), e.remove_volume_ids, e.num_remove_volumes);
  out.new_vol_instance = renumber(num_old_vol_instances, e.remove_vol_instance_ids, e.num_remove_vol_instances);
  out.new_sdf          = renumber(num_old_sdfs, e.remove_sdf_ids, e.num_remove_sdfs);
  out.moves_pool       = e.num_remove_volumes > 0 || e.num_add_volumes > 0;
  if (!out.moves_pool) {
    out.volumes = old_volumes, out.num_voxels = old_num_voxels;
    return;
  }
  long long at = 0;
  auto run = [&](long long length, int kind, long long src) {
    if (length > 0) out.segments.push_back({at, length, kind, 0, src});
    at += length;
  };
  for (size_t i = 0; i < old_volumes.size(); i++) {
    if (out.new_volume[i] < 0) continue;
    vpt_volume v = old_volumes[i];
    const long long was = v.offset;
    v.offset = at;
    out.volumes.push_back(v);
    run(volume_voxels(v.whd), VOL_SEG_OLD_POOL, was);
  }
  for (int i = 0; i < e.num_add_volumes; i++) {
    const vpt_volume_new& n = e.add_volumes[i];
    vpt_volume v = {{n.whd[0], n.whd[1], n.whd[2]}, n.res, at};
    out.volumes.push_back(v);
    out.added_offset.push_back(at);
    const long long length = volume_voxels(n.whd);
    if (n.source == VPT_VOLUME_FROM_HOST) run(length, VOL_SEG_STAGING, n.offset);
    else if (n.source == VPT_VOLUME_FROM_BAKE) run(length, VOL_SEG_BAKE, 0);
    else if (n.source == VPT_VOLUME_FILL) {
      uint32_t bits;
      memcpy(&bits, &n.fill, 4);
      run(length, VOL_SEG_CONSTANT, (long long)bits);
    } else run(length, VOL_SEG_OLD_POOL, old_volumes[(size_t)n.copy_of].offset);
  }
  out.num_voxels = at;
}
