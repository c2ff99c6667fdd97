// vpt_bake.h — the two halves of vpt_bake_sdf (vpt_bake.hip) for a caller that bakes into voxels already on the device
// (vpt_scene_update_volumes, vpt_volume_update.hip): the host preparation with its uploads, and the launch.
#pragma once
#include "vpt_device_buffer.h"

// what a bake kernel reads besides the grid: made by bake_prepare on the current device, good for any number of launches
struct bake_job {
  device_buffer nodes, records;   // the tree (none in the brute form) and the triangle records in its slot order
  int   num_nodes = 0, num_records = 0;
  float reach = 0;
  bool  brute = false;
  vpt_bake_stats stats = {};      // dropped_triangles, bvh_nodes, bvh_depth
  long long bytes = 0;            // sent to the device: nodes and records
};
// The box of voxels a launch writes and how: lo <= voxel < hi per axis, inside the grid; mode VPT_VOXELS_REPLACE / VPT_VOXELS_UNION
// (include/vpt.h: UNION selects (a < b) ? a : b against the value the destination holds).
struct bake_region { int lo[3], hi[3], mode; };

// vpt_bake_sdf's host preparation for `desc` (which has passed vpt_bake_validate) under the name `entry`: feature normals, the tree through vpt_build_bvh
// on `device` (VPT_BAKE_BRUTE=1: none), the depth check (VPT_ERR_UNSUPPORTED), the records; nodes and records sent to `device`,
// which is the current device afterwards.  Writes nothing a scene owns.
int bake_prepare(int device, const vpt_bake_desc* desc, const char* entry, bake_job& job);
// One bake kernel on stream 0 over `desc`'s grid into d_voxels (the grid's first voxel, x + y*W + z*W*H).  region null: every
// voxel, plainly written (vpt_bake_sdf); else the instance that runs only the bricks touching the region and writes only the lanes
// inside it.  Asynchronous; *launched (nullable) counts the launch (an empty region launches nothing).
int bake_launch(const bake_job& job, const vpt_bake_desc* desc, float* d_voxels, const bake_region* region, int* launched);
