// vpt_bake.hip — vpt_bake_sdf (include/vpt.h): a triangle mesh baked into a signed-distance voxel grid, one lane per voxel.
// The arithmetic of a voxel is csrc/vpt_bake_rule.h, which the host mirror (host/vpt_bake.cpp) compiles too; this unit adds what
// makes it fast and cannot change a bit of it: a nearest-triangle walk of the project's own BVH (vpt_build_bvh over the boxes of
// the kept triangles, through the public entry: the node array is needed on the host anyway, for the depth check) instead of a
// loop over every triangle.  Because the winner is the minimum of (d2, caller's index), any visiting order that reaches every
// triangle whose d2 can equal the minimum gives the same voxel; what the walk may skip is decided by `reach`.
//
// Launch shape: one wave per block, a wave takes a 4 x 4 x 4 brick of voxels (lane = x + 4 y + 16 z inside it), so that the
// lanes of a wave walk nearly the same nodes.  The per-lane stack lies in LDS as [entry][lane]: entry e of lane l is word
// 64 e + l, so the 64 lanes of a push or pop touch the 64 banks once each.  BAKE_STACK entries of 4 bytes: 12 KB per wave.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vpt_bake.h"
#include "vpt_bake_prep.h"
#include "vpt_bake_rule.h"
#include "vpt_device_buffer.h"
#include "vpt_error.h"

namespace {

constexpr int BAKE_STACK = 48;   // far children a lane can have pending: one per internal node on its path, so a tree of depth <= 48

struct bake_grid {
  int   w, h, d;
  float origin[3], step[3];
};

// squared distance from p to a node's box, 0 inside
__device__ __forceinline__ float box_distance2(vpt_bake_f3 p, float4 q0, float4 q1) {
  float dx = fmaxf(fmaxf(q0.x - p.x, p.x - q0.w), 0.0f);
  float dy = fmaxf(fmaxf(q0.y - p.y, p.y - q1.x), 0.0f);
  float dz = fmaxf(fmaxf(q0.z - p.z, p.z - q1.y), 0.0f);
  return (dx * dx + dy * dy) + dz * dz;
}

// nodes == nullptr: the brute form, every record in turn.  records: in BVH slot order (leaf primitives start .. start + num - 1),
// or in the caller's order in the brute form.
// REGION (vpt_scene_update_volumes: the destination is a volume's place in a resident voxel pool): the grid holds the bricks that
// touch the box r.lo .. r.hi, a lane outside the box does nothing, and in UNION mode the voxel is selected against the resident
// value.  A voxel's arithmetic does not know its brick: the same bits as the whole-grid instance.
template <bool REGION>
__global__ __launch_bounds__(64) void bake_kernel(bake_grid g, bake_region r, const float4* __restrict__ nodes, int num_nodes,
    const vpt_bake_record* __restrict__ records, int num_records, float reach, float* __restrict__ voxels) {
  __shared__ int stack[BAKE_STACK * 64];
  const int lane = threadIdx.x;
  const int first_x = REGION ? r.lo[0] >> 2 : 0, first_y = REGION ? r.lo[1] >> 2 : 0, first_z = REGION ? r.lo[2] >> 2 : 0;
  const int bricks_x = (((REGION ? r.hi[0] : g.w) + 3) >> 2) - first_x, bricks_y = (((REGION ? r.hi[1] : g.h) + 3) >> 2) - first_y;
  const int brick = blockIdx.x;
  const int x = ((first_x + brick % bricks_x) << 2) + (lane & 3);
  const int y = ((first_y + (brick / bricks_x) % bricks_y) << 2) + ((lane >> 2) & 3);
  const int z = ((first_z + brick / (bricks_x * bricks_y)) << 2) + (lane >> 4);
  const bool inside = REGION ? x >= r.lo[0] && x < r.hi[0] && y >= r.lo[1] && y < r.hi[1] && z >= r.lo[2] && z < r.hi[2] : x < g.w && y < g.h && z < g.d;
  if (inside) {   // lanes outside the grid (the region) stay in the wave and do nothing
    const vpt_bake_f3 p = {vpt_bake_sample(g.origin[0], g.step[0], x), vpt_bake_sample(g.origin[1], g.step[1], y),
        vpt_bake_sample(g.origin[2], g.step[2], z)};
    vpt_bake_best best = vpt_bake_none();
    if (!nodes) {
      for (int slot = 0; slot < num_records; slot++) vpt_bake_offer(best, vpt_bake_distance2(p, records[slot]), records[slot].index, slot);
    } else {
      int   node = 0, sp = 0;
      float limit = INFINITY;   // sqrt(best.d2) + reach: a node whose box is farther than this holds no winner
      for (int visit = 0; visit < num_nodes; visit++) {   // a node is visited at most once
        const float4 q0 = nodes[2 * node], q1 = nodes[2 * node + 1];
        // a node whose bound EQUALS the best distance is entered: it may hold the same distance under a smaller index
        if (!(sqrtf(box_distance2(p, q0, q1)) > limit)) {
          const int start = __float_as_int(q1.z), packed = __float_as_int(q1.w);
          if ((packed >> 24) & 0xff) {   // internal: the nearer child next, the other one later
            const float dl = box_distance2(p, nodes[2 * start], nodes[2 * start + 1]);
            const float dr = box_distance2(p, nodes[2 * start + 2], nodes[2 * start + 3]);
            const int   near = dr < dl ? start + 1 : start, far = dr < dl ? start : start + 1;
            if (sp < BAKE_STACK) stack[64 * sp++ + lane] = far;   // always true: the host refuses a tree deeper than the stack
            node = near;
            continue;
          }
          const int num = packed & 0xffff;
          for (int k = 0; k < num; k++) vpt_bake_offer(best, vpt_bake_distance2(p, records[start + k]), records[start + k].index, start + k);
          limit = sqrtf(best.d2) + reach;
        }
        if (sp == 0) break;
        node = stack[64 * --sp + lane];
      }
    }
    const size_t at = (size_t)x + (size_t)y * g.w + (size_t)z * g.w * g.h;
    float v = best.slot < 0 ? vpt_bake_no_winner() : vpt_bake_value(p, records[best.slot]);
    if (REGION && r.mode == VPT_VOXELS_UNION) {   // op_union, yocto_sdfs.h:82: the select, not fminf
      const float a = voxels[at];
      v = (a < v) ? a : v;
    }
    voxels[at] = v;
  }
}

// edges from the root to the deepest leaf; -1 for an array that is no tree of `count` nodes
int tree_depth(const std::vector<vpt_bvh_node>& nodes, int count) {
  std::vector<std::pair<int, int>> todo = {{0, 0}};
  int depth = 0, visited = 0;
  while (!todo.empty()) {
    auto [id, level] = todo.back();
    todo.pop_back();
    if (id < 0 || id >= count || ++visited > count) return -1;
    if (level > depth) depth = level;
    if (!nodes[id].internal) continue;
    todo.push_back({nodes[id].start, level + 1}), todo.push_back({nodes[id].start + 1, level + 1});
  }
  return depth;
}

}  // namespace

int bake_prepare(int device, const vpt_bake_desc* desc, const char* entry, bake_job& job) {
  job.stats = vpt_bake_stats{}, job.bytes = 0;
  vpt_bake_stats* stats = &job.stats;
  const int nt = desc->num_triangles;
  std::vector<float>   normals(21 * (size_t)nt);
  std::vector<int32_t> keep(nt);
  if (int rc = vpt_bake_normals(desc, normals.data(), keep.data(), entry)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return vpt_set_error(VPT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
  REQUIRE(device >= 0 && device < ndev, "%s: device %d out of range (%d devices)", entry, device, ndev);
  std::vector<int32_t> kept;   // the caller's indices of the kept triangles, ascending
  for (int t = 0; t < nt; t++)
    if (keep[t]) kept.push_back(t);
  const int nk = (int)kept.size();
  const char* env   = getenv("VPT_BAKE_BRUTE");
  const bool  brute = env && strcmp(env, "1") == 0;

  // M: the largest magnitude among the coordinates the kernel computes with (kept corners, first and last sample point per axis)
  double M = 0;
  auto   corner = [&](int t, int c) { return desc->positions + 3 * (size_t)desc->triangles[3 * (size_t)t + c]; };
  for (int t : kept)
    for (int c = 0; c < 3; c++)
      for (int k = 0; k < 3; k++) M = std::fmax(M, std::fabs((double)corner(t, c)[k]));
  for (int k = 0; k < 3; k++) {
    M = std::fmax(M, std::fabs((double)vpt_bake_sample(desc->origin[k], desc->step[k], 0)));
    M = std::fmax(M, std::fabs((double)vpt_bake_sample(desc->origin[k], desc->step[k], desc->whd[k] - 1)));
  }
  // the computed distance of a triangle is not below the computed distance of a box around it by more than 2^-14 M
  const double reach_d = std::ldexp(M, -14);
  const float  reach   = reach_d < 3.0e38 ? std::nextafterf((float)reach_d, INFINITY) : INFINITY;

  std::vector<vpt_bvh_node> nodes;
  std::vector<int32_t>      order(nk);   // slot -> position in `kept`
  int num_nodes = 0, depth = 0;
  if (brute) {
    for (int i = 0; i < nk; i++) order[i] = i;
  } else {
    std::vector<float> boxes(6 * (size_t)nk);
    for (int i = 0; i < nk; i++)
      for (int k = 0; k < 3; k++) {
        float a = corner(kept[i], 0)[k], b = corner(kept[i], 1)[k], c = corner(kept[i], 2)[k];
        boxes[6 * (size_t)i + k]     = std::fmin(a, std::fmin(b, c));
        boxes[6 * (size_t)i + 3 + k] = std::fmax(a, std::fmax(b, c));
      }
    nodes.resize(2 * (size_t)nk);
    if (int rc = vpt_build_bvh(device, boxes.data(), nk, nodes.data(), (int)nodes.size(), &num_nodes, order.data())) return rc;
    depth = tree_depth(nodes, num_nodes);
    if (depth < 0) return vpt_set_error(VPT_ERR_HIP, "%s: the BVH build returned no tree", entry);
    for (int i = 0; i < num_nodes; i++)
      if (!nodes[i].internal && (nodes[i].start < 0 || nodes[i].num < 0 || nodes[i].start + nodes[i].num > nk))
        return vpt_set_error(VPT_ERR_HIP, "%s: the BVH build returned a leaf outside the primitive array", entry);
    stats->dropped_triangles = nt - nk, stats->bvh_nodes = num_nodes, stats->bvh_depth = depth;
    if (depth > BAKE_STACK)
      return vpt_set_error(VPT_ERR_UNSUPPORTED, "%s: BVH depth %d needs a %d-entry traversal stack; the LDS stack holds %d", entry, depth, depth, BAKE_STACK);
  }
  stats->dropped_triangles = nt - nk;
  std::vector<vpt_bake_record> records(nk);
  for (int slot = 0; slot < nk; slot++) {
    REQUIRE(order[slot] >= 0 && order[slot] < nk, "%s: the BVH build returned primitive %d of %d", entry, order[slot], nk);
    records[slot] = vpt_bake_make_record(desc->positions, desc->triangles, normals.data(), kept[order[slot]]);
  }

  HIP_TRY(hipSetDevice(device));
  if (job.nodes.allocate((size_t)num_nodes * sizeof(vpt_bvh_node)) || job.records.allocate((size_t)nk * sizeof(vpt_bake_record))) return VPT_ERR_HIP;
  if (num_nodes) HIP_TRY(hipMemcpy(job.nodes.get(), nodes.data(), (size_t)num_nodes * sizeof(vpt_bvh_node), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(job.records.get(), records.data(), (size_t)nk * sizeof(vpt_bake_record), hipMemcpyHostToDevice));
  job.num_nodes = num_nodes, job.num_records = nk, job.reach = reach, job.brute = brute;
  job.bytes = (long long)((size_t)num_nodes * sizeof(vpt_bvh_node) + (size_t)nk * sizeof(vpt_bake_record));
  return VPT_OK;
}

int bake_launch(const bake_job& job, const vpt_bake_desc* desc, float* d_voxels, const bake_region* region, int* launched) {
  bake_grid g;
  g.w = desc->whd[0], g.h = desc->whd[1], g.d = desc->whd[2];
  for (int k = 0; k < 3; k++) g.origin[k] = desc->origin[k], g.step[k] = desc->step[k];
  bake_region r = {{0, 0, 0}, {g.w, g.h, g.d}, VPT_VOXELS_REPLACE};
  if (region) r = *region;
  long long bricks = 1;   // every brick holds a voxel of the grid: fewer than 2^31
  for (int k = 0; k < 3; k++) {
    if (r.hi[k] <= r.lo[k]) return VPT_OK;   // an empty region
    bricks *= ((r.hi[k] + 3) >> 2) - (r.lo[k] >> 2);
  }
  const float4* nodes = job.brute ? nullptr : job.nodes.get<float4>();
  if (region) hipLaunchKernelGGL(bake_kernel<true>, dim3((unsigned)bricks), dim3(64), 0, 0, g, r, nodes, job.num_nodes, job.records.get<vpt_bake_record>(), job.num_records, job.reach, d_voxels);
  else hipLaunchKernelGGL(bake_kernel<false>, dim3((unsigned)bricks), dim3(64), 0, 0, g, r, nodes, job.num_nodes, job.records.get<vpt_bake_record>(), job.num_records, job.reach, d_voxels);
  HIP_TRY(hipGetLastError());
  if (launched) ++*launched;
  return VPT_OK;
}

extern "C" int vpt_bake_sdf(int device, const vpt_bake_desc* desc, float* voxels, vpt_bake_stats* stats) {
  const char* entry = "vpt_bake_sdf";
  if (stats) *stats = vpt_bake_stats{};
  if (int rc = vpt_bake_validate(desc, entry)) return rc;
  REQUIRE(voxels, "%s: null voxels", entry);
  bake_job job;
  const int rc = bake_prepare(device, desc, entry, job);
  if (stats) *stats = job.stats;   // of a tree that is too deep as well
  if (rc) return rc;
  const size_t  nvox = (size_t)desc->whd[0] * desc->whd[1] * desc->whd[2];
  device_buffer d_voxels;
  if (d_voxels.allocate(nvox * sizeof(float))) return VPT_ERR_HIP;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(hipEventCreate(&e0));
  if (hipError_t e = hipEventCreate(&e1); e != hipSuccess) {
    (void)hipEventDestroy(e0);
    return vpt_set_error(VPT_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(e));
  }
  float      ms = 0;
  hipError_t err = hipEventRecord(e0, 0);
  int        launch_rc = VPT_OK;   // bake_launch has recorded HIP's own message
  if (err == hipSuccess) launch_rc = bake_launch(job, desc, d_voxels.get<float>(), nullptr, nullptr);
  if (err == hipSuccess && launch_rc == VPT_OK) err = hipEventRecord(e1, 0);
  if (err == hipSuccess && launch_rc == VPT_OK) err = hipEventSynchronize(e1);
  if (err == hipSuccess && launch_rc == VPT_OK) err = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0), (void)hipEventDestroy(e1);
  if (launch_rc != VPT_OK) return launch_rc;
  if (err != hipSuccess) return vpt_set_error(VPT_ERR_HIP, "%s: bake kernel: %s", entry, hipGetErrorString(err));
  if (stats) stats->launches = 1, stats->device_ms = ms;
  HIP_TRY(hipMemcpy(voxels, d_voxels.get(), nvox * sizeof(float), hipMemcpyDeviceToHost));
  return VPT_OK;
}
