// vpt_volume_update.h — editing the volumes, grid instances and SDFs of a resident scene (include/vpt.h: vpt_scene_update_volumes;
// DESIGN.md §17): what a vpt_scene keeps for it and the calls vpt_capi.hip forwards to.  Kernel and host logic: vpt_volume_update.hip.
#pragma once
#include <vector>

#include "vpt_device_buffer.h"
#include "vpt_light_update.h"

struct volume_updater {
  long long num_voxels = 0;   // voxels of the pool the device holds now (set at creation; a volume that changes whd gets room at the end)
  // host copies of DScene::volumes and DScene::vol_instances, read back on the first edit of a handle (the SDFs' is light_updater's:
  // the light list is decided from it)
  bool ready = false;
  std::vector<vpt_volume>          volumes;
  std::vector<vpt_volume_instance> vol_instances;
};

// Validates `edit` and prepares its bakes (nothing a scene owns is written before both have passed), then writes voxels, the three
// small tables and every SDF record, and - when the SDF lights change - rebuilds the light tables through light_update_apply.  A
// voxel pool that grows is allocated anew and takes its predecessor's place in `tables`.  u's counters (vpt_scene_update_stats)
// describe this call.  Stream 0 of `device`; the device has finished when the call returns.
int volume_update_apply(DScene& d, const host_mirrors& h, long long num_shape_nodes, scene_updater& u, light_updater& lu, volume_updater& vu,
    std::vector<device_buffer>& tables, const vpt_volume_edit& edit, int device, int* light_features, bool* rebuilt);
