// vpt_sdf_mesh.hip — vpt_mesh_sdf and vpt_scene_mesh_volume (include/vpt.h): the iso surface of a signed-distance voxel grid
// as a quad mesh.  The arithmetic and the flags are csrc/vpt_sdf_mesh_rule.h's, which the host mirror (host/vpt_sdf_mesh.cpp) compiles too:
// this unit is built with -ffp-contract=off like it.  Here: four passes over the voxels in index order, one lane per voxel in 1-D blocks,
// so that block order is the rule's order and a rank is (scanned count of the blocks before) + (waves before in the block) + (lanes
// before in the wave) - no atomics, nothing depends on which block arrives first.
//   1. classify   one byte per voxel (its cell's active bit, its three edges' quad bits) and {cells, quads} per block
//   2. scan       rocPRIM's exclusive scan of the block counts; its last entry, the totals, is the one read-back that sizes the outputs
//   3. vertices   the id of every active cell into a per-voxel array, its position and normal into the outputs
//   4. quads      an int4 of the four neighbouring cells' ids per quad bit: a launch of its own, it reads ids other blocks wrote
// Scratch: 5 bytes per voxel (flags, ids) and 32 bytes per block.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "vpt_device_buffer.h"
#include "vpt_error.h"
#include "vpt_resident.h"
#include "vpt_sdf_mesh_rule.h"

namespace {

constexpr int MESH_BLOCK = 256, MESH_WAVES = MESH_BLOCK / 64;

// the grid a launch works on: a box of voxels (all of them, or a region) inside an array of rows of w and slices of w * h voxels
struct mesh_grid {
  int   w, h;
  int   lo[3], dim[3];
  float origin[3], step[3], iso;
};
struct mesh_counts {
  long long cells, quads;
};
struct mesh_counts_plus {
  __host__ __device__ mesh_counts operator()(const mesh_counts& a, const mesh_counts& b) const { return {a.cells + b.cells, a.quads + b.quads}; }
};

// voxel (x, y, z) of the box: 64-bit from the first voxel of the array (a volume's place in a pool of any size)
__device__ __forceinline__ size_t voxel_at(const mesh_grid& g, int x, int y, int z) {
  return (size_t)(g.lo[0] + x) + (size_t)(g.lo[1] + y) * (size_t)g.w + (size_t)(g.lo[2] + z) * (size_t)g.w * (size_t)g.h;
}
__device__ __forceinline__ void split_index(const mesh_grid& g, unsigned idx, int p[3]) {
  p[0] = (int)(idx % (unsigned)g.dim[0]), p[1] = (int)((idx / (unsigned)g.dim[0]) % (unsigned)g.dim[1]),
  p[2] = (int)(idx / ((unsigned)g.dim[0] * (unsigned)g.dim[1]));
}
// the eight corners of cell p, which exists
__device__ __forceinline__ void load_cell(const float* __restrict__ voxels, const mesh_grid& g, const int p[3], float c[8]) {
#pragma unroll
  for (int k = 0; k < 8; k++) c[k] = voxels[voxel_at(g, p[0] + (k & 1), p[1] + ((k >> 1) & 1), p[2] + (k >> 2))];
}
__device__ __forceinline__ unsigned lanes_below(unsigned long long ballot) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// Pass 1.  A lane owns voxel idx of the box: its cell and its three edges.  The corners are read with their coordinates clamped to the
// box, so every load is in bounds and no lane branches on where it lies; what a clamped corner stands in for is never looked at (a cell
// on the upper border does not exist, an edge that leaves the box neither).  Along x a wave's eight loads are consecutive, and a voxel that
// eight lanes read comes out of L1 / L2 for seven of them: staging the block's corners in LDS first was measured and is slower.
__global__ __launch_bounds__(MESH_BLOCK) void mesh_classify_kernel(const float* __restrict__ voxels, mesh_grid g, unsigned n, unsigned char* __restrict__ flags,
    mesh_counts* __restrict__ counts) {
  __shared__ unsigned wave_counts[MESH_WAVES][2];
  const unsigned idx  = blockIdx.x * MESH_BLOCK + threadIdx.x;   // the last block's lanes stay below 2^32
  unsigned bits = 0;
  if (idx < n) {
    int p[3];
    split_index(g, idx, p);
    const bool has[3] = {p[0] + 1 < g.dim[0], p[1] + 1 < g.dim[1], p[2] + 1 < g.dim[2]};
    float c[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int x = min(p[0] + (k & 1), g.dim[0] - 1), y = min(p[1] + ((k >> 1) & 1), g.dim[1] - 1), z = min(p[2] + (k >> 2), g.dim[2] - 1);
      c[k] = voxels[voxel_at(g, x, y, z)];
    }
    if (has[0] && has[1] && has[2] && vpt_sdf_mesh_active(vpt_sdf_mesh_mask(c, g.iso))) bits |= VPT_SDF_MESH_ACTIVE;
#pragma unroll
    for (int a = 0; a < 3; a++)
      if (has[a]) bits |= vpt_sdf_mesh_edge_bits(a, p, g.dim, c[0], c[1 << a], g.iso);
    flags[idx] = (unsigned char)bits;
  }
  const unsigned long long cell = __builtin_amdgcn_ballot_w64(bits & VPT_SDF_MESH_ACTIVE);
  const unsigned quads = __popcll(__builtin_amdgcn_ballot_w64(bits & (VPT_SDF_MESH_QUAD << 0))) + __popcll(__builtin_amdgcn_ballot_w64(bits & (VPT_SDF_MESH_QUAD << 1))) +
                         __popcll(__builtin_amdgcn_ballot_w64(bits & (VPT_SDF_MESH_QUAD << 2)));
  if ((threadIdx.x & 63) == 0) wave_counts[threadIdx.x >> 6][0] = __popcll(cell), wave_counts[threadIdx.x >> 6][1] = quads;
  __syncthreads();
  if (threadIdx.x == 0) {
    mesh_counts sum = {0, 0};
    for (int wv = 0; wv < MESH_WAVES; wv++) sum.cells += wave_counts[wv][0], sum.quads += wave_counts[wv][1];
    counts[blockIdx.x] = sum;
  }
}

// the entries of the block's waves before this lane's wave, of `mine` set by every wave's first lane (one barrier)
__device__ __forceinline__ unsigned waves_before(unsigned (&per_wave)[MESH_WAVES], unsigned mine) {
  if ((threadIdx.x & 63) == 0) per_wave[threadIdx.x >> 6] = mine;
  __syncthreads();
  unsigned before = 0;
  for (unsigned wv = 0; wv < (threadIdx.x >> 6); wv++) before += per_wave[wv];
  return before;
}

// Pass 3.  positions / normals: float3 per vertex, either may be null (then only the ids are made).
__global__ __launch_bounds__(MESH_BLOCK) void mesh_vertices_kernel(const float* __restrict__ voxels, mesh_grid g, unsigned n, const unsigned char* __restrict__ flags,
    const mesh_counts* __restrict__ bases, int* __restrict__ ids, float* __restrict__ positions, float* __restrict__ normals) {
  __shared__ unsigned per_wave[MESH_WAVES];
  const unsigned idx    = blockIdx.x * MESH_BLOCK + threadIdx.x;
  const bool     active = idx < n && (flags[idx] & VPT_SDF_MESH_ACTIVE);
  const unsigned long long ballot = __builtin_amdgcn_ballot_w64(active);
  const unsigned before = waves_before(per_wave, (unsigned)__popcll(ballot));
  if (!active) return;
  const long long id = bases[blockIdx.x].cells + before + lanes_below(ballot);   // < 2^31: there are fewer voxels than that
  ids[idx] = (int)id;
  if (!positions && !normals) return;
  int p[3];
  split_index(g, idx, p);
  float c[8];
  load_cell(voxels, g, p, c);
  const vpt_sdf_mesh_f3 u = vpt_sdf_mesh_cell_vertex(c, g.iso);
  if (positions) {
    positions[3 * id + 0] = vpt_sdf_mesh_position(g.origin[0], g.step[0], g.lo[0] + p[0], u.x);
    positions[3 * id + 1] = vpt_sdf_mesh_position(g.origin[1], g.step[1], g.lo[1] + p[1], u.y);
    positions[3 * id + 2] = vpt_sdf_mesh_position(g.origin[2], g.step[2], g.lo[2] + p[2], u.z);
  }
  if (normals) {
    const vpt_sdf_mesh_f3 nrm = vpt_sdf_mesh_normal(c, u, g.step);
    normals[3 * id + 0] = nrm.x, normals[3 * id + 1] = nrm.y, normals[3 * id + 2] = nrm.z;
  }
}

// Pass 4.  A quad bit is set only where the four cells around the edge exist, and each of them holds both ends of the edge: all four are
// active and have their ids.
__global__ __launch_bounds__(MESH_BLOCK) void mesh_quads_kernel(mesh_grid g, unsigned n, const unsigned char* __restrict__ flags, const mesh_counts* __restrict__ bases,
    const int* __restrict__ ids, int4* __restrict__ quads) {
  __shared__ unsigned per_wave[MESH_WAVES];
  const unsigned idx  = blockIdx.x * MESH_BLOCK + threadIdx.x;
  const unsigned bits = idx < n ? flags[idx] : 0u;
  const unsigned long long b0 = __builtin_amdgcn_ballot_w64(bits & (VPT_SDF_MESH_QUAD << 0)), b1 = __builtin_amdgcn_ballot_w64(bits & (VPT_SDF_MESH_QUAD << 1)),
                           b2 = __builtin_amdgcn_ballot_w64(bits & (VPT_SDF_MESH_QUAD << 2));
  const unsigned before = waves_before(per_wave, (unsigned)(__popcll(b0) + __popcll(b1) + __popcll(b2)));
  if (!(bits & (7 * VPT_SDF_MESH_QUAD))) return;
  long long at = bases[blockIdx.x].quads + before + lanes_below(b0) + lanes_below(b1) + lanes_below(b2);   // < 2^31: the host has checked the total
  const long long stride[3] = {1, g.dim[0], (long long)g.dim[0] * g.dim[1]};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (!(bits & (VPT_SDF_MESH_QUAD << a))) continue;
    long long cell[4];
    vpt_sdf_mesh_quad_cells(a, (bits & (VPT_SDF_MESH_FLIP << a)) != 0, stride, cell);
    quads[at++] = make_int4(ids[(long long)idx + cell[0]], ids[(long long)idx + cell[1]], ids[(long long)idx + cell[2]], ids[(long long)idx + cell[3]]);
  }
}

struct event_pair {   // destroyed on every path
  hipEvent_t a = nullptr, b = nullptr;
  ~event_pair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  int create() {
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    return VPT_OK;
  }
  int elapsed(float& ms) const {
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, a, b));
    ms += t;
    return VPT_OK;
  }
};

struct mesh_outputs {
  float*   positions;
  float*   normals;
  int32_t  vertex_capacity;
  int32_t* quads;
  int32_t  quad_capacity;
};

bool no_cells(const mesh_grid& g) { return g.dim[0] < 2 || g.dim[1] < 2 || g.dim[2] < 2; }

// The four passes over the box `g` of the device array `voxels`, on the current device's stream 0, which is idle.  The caller has validated.
int mesh_run(const char* entry, const float* voxels, const mesh_grid& g, const mesh_outputs& out, vpt_sdf_mesh_stats* stats) {
  *stats = vpt_sdf_mesh_stats{};
  if (no_cells(g)) return VPT_OK;
  const long long n      = (long long)g.dim[0] * g.dim[1] * g.dim[2];
  const unsigned  blocks = (unsigned)((n + MESH_BLOCK - 1) / MESH_BLOCK);
  device_buffer flags, counts, bases, scan_temp;
  if (flags.allocate((size_t)n) || counts.allocate(((size_t)blocks + 1) * sizeof(mesh_counts)) || bases.allocate(((size_t)blocks + 1) * sizeof(mesh_counts))) return VPT_ERR_HIP;
  size_t scan_bytes = 0;
  HIP_TRY(rocprim::exclusive_scan((void*)nullptr, scan_bytes, counts.get<mesh_counts>(), bases.get<mesh_counts>(), mesh_counts{0, 0}, (size_t)blocks + 1, mesh_counts_plus()));
  if (scan_temp.allocate(scan_bytes)) return VPT_ERR_HIP;
  event_pair count_time, emit_time;
  if (int rc = count_time.create()) return rc;
  if (int rc = emit_time.create()) return rc;
  // the entry after the last block's is zero: its place in the scan holds the totals
  HIP_TRY(hipMemsetAsync(counts.get<mesh_counts>() + blocks, 0, sizeof(mesh_counts), 0));
  HIP_TRY(hipEventRecord(count_time.a, 0));
  hipLaunchKernelGGL(mesh_classify_kernel, dim3(blocks), dim3(MESH_BLOCK), 0, 0, voxels, g, (unsigned)n, flags.get<unsigned char>(), counts.get<mesh_counts>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(rocprim::exclusive_scan(scan_temp.get(), scan_bytes, counts.get<mesh_counts>(), bases.get<mesh_counts>(), mesh_counts{0, 0}, (size_t)blocks + 1, mesh_counts_plus()));
  stats->launches = 2;
  HIP_TRY(hipEventRecord(count_time.b, 0));
  mesh_counts total = {0, 0};
  HIP_TRY(hipMemcpy(&total, bases.get<mesh_counts>() + blocks, sizeof(total), hipMemcpyDeviceToHost));   // waits for the scan
  if (int rc = count_time.elapsed(stats->device_ms)) return rc;
  if (total.quads > INT_MAX) return vpt_set_error(VPT_ERR_UNSUPPORTED, "%s: %lld quads: more than 2^31 - 1", entry, total.quads);
  stats->num_vertices = (int32_t)total.cells, stats->num_quads = (int32_t)total.quads;
  REQUIRE(!(out.positions || out.normals) || out.vertex_capacity >= stats->num_vertices, "vertex_capacity %d < %d vertices", out.vertex_capacity, stats->num_vertices);
  REQUIRE(!out.quads || out.quad_capacity >= stats->num_quads, "quad_capacity %d < %d quads", out.quad_capacity, stats->num_quads);
  if (!(out.positions || out.normals || out.quads) || total.cells == 0) return VPT_OK;

  const size_t nv = (size_t)total.cells, nq = (size_t)total.quads;
  device_buffer ids, positions, normals, quads;
  if (ids.allocate((size_t)n * sizeof(int))) return VPT_ERR_HIP;
  if (out.positions && positions.allocate(nv * 12)) return VPT_ERR_HIP;
  if (out.normals && normals.allocate(nv * 12)) return VPT_ERR_HIP;
  if (out.quads && quads.allocate(nq * sizeof(int4))) return VPT_ERR_HIP;
  HIP_TRY(hipEventRecord(emit_time.a, 0));
  hipLaunchKernelGGL(mesh_vertices_kernel, dim3(blocks), dim3(MESH_BLOCK), 0, 0, voxels, g, (unsigned)n, flags.get<const unsigned char>(), bases.get<const mesh_counts>(),
      ids.get<int>(), positions.get<float>(), normals.get<float>());
  HIP_TRY(hipGetLastError());
  stats->launches++;
  if (out.quads && nq) {
    hipLaunchKernelGGL(mesh_quads_kernel, dim3(blocks), dim3(MESH_BLOCK), 0, 0, g, (unsigned)n, flags.get<const unsigned char>(), bases.get<const mesh_counts>(),
        ids.get<const int>(), quads.get<int4>());
    HIP_TRY(hipGetLastError());
    stats->launches++;
  }
  HIP_TRY(hipEventRecord(emit_time.b, 0));
  HIP_TRY(hipEventSynchronize(emit_time.b));
  if (int rc = emit_time.elapsed(stats->device_ms)) return rc;
  if (out.positions) HIP_TRY(hipMemcpy(out.positions, positions.get(), nv * 12, hipMemcpyDeviceToHost));
  if (out.normals) HIP_TRY(hipMemcpy(out.normals, normals.get(), nv * 12, hipMemcpyDeviceToHost));
  if (out.quads && nq) HIP_TRY(hipMemcpy(out.quads, quads.get(), nq * sizeof(int4), hipMemcpyDeviceToHost));
  return VPT_OK;
}

int validate(const char* entry, const vpt_sdf_mesh_desc* desc, const mesh_outputs& out, const vpt_sdf_mesh_stats* stats) {
  REQUIRE(desc && stats, "%s: null argument", entry);
  if (const char* fault = vpt_sdf_mesh_desc_fault(*desc)) return vpt_set_error(VPT_ERR_INVALID_ARG, "%s: %s", entry, fault);
  REQUIRE(out.vertex_capacity >= 0 && out.quad_capacity >= 0, "%s: a capacity is negative", entry);
  return VPT_OK;
}

mesh_grid grid_of(const vpt_sdf_mesh_desc& d, const vpt_sdf_mesh_region* region) {
  mesh_grid g = {d.whd[0], d.whd[1], {0, 0, 0}, {d.whd[0], d.whd[1], d.whd[2]}, {d.origin[0], d.origin[1], d.origin[2]}, {d.step[0], d.step[1], d.step[2]}, d.iso};
  if (region)
    for (int k = 0; k < 3; k++) g.lo[k] = region->lo[k], g.dim[k] = region->whd[k];
  return g;
}

}  // namespace

extern "C" int vpt_mesh_sdf(int device, const vpt_sdf_mesh_desc* desc, const float* voxels, float* positions, float* normals, int32_t vertex_capacity, int32_t* quads,
    int32_t quad_capacity, vpt_sdf_mesh_stats* stats) {
  const char*        entry = "vpt_mesh_sdf";
  const mesh_outputs out   = {positions, normals, vertex_capacity, quads, quad_capacity};
  if (int rc = validate(entry, desc, out, stats)) return rc;
  REQUIRE(voxels, "%s: null voxels", entry);
  const mesh_grid g = grid_of(*desc, nullptr);
  *stats = vpt_sdf_mesh_stats{};
  if (no_cells(g)) return VPT_OK;   // nothing to mesh: no device is looked for
  // nor for a grid that lies on one side of iso: the voxels are at hand, and the look ends at the first voxel of the other side
  const size_t count = (size_t)g.dim[0] * g.dim[1] * g.dim[2];
  size_t       other = 1;
  while (other < count && vpt_sdf_mesh_inside(voxels[other], g.iso) == vpt_sdf_mesh_inside(voxels[0], g.iso)) other++;
  if (other == count) return VPT_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return vpt_set_error(VPT_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
  REQUIRE(device >= 0 && device < ndev, "%s: device %d out of range (%d devices)", entry, device, ndev);
  HIP_TRY(hipSetDevice(device));
  const size_t  bytes = (size_t)g.dim[0] * g.dim[1] * g.dim[2] * sizeof(float);
  device_buffer d_voxels;
  if (d_voxels.allocate(bytes)) return VPT_ERR_HIP;
  HIP_TRY(hipMemcpy(d_voxels.get(), voxels, bytes, hipMemcpyHostToDevice));
  return mesh_run(entry, d_voxels.get<const float>(), g, out, stats);
}

extern "C" int vpt_scene_mesh_volume(vpt_scene* scene, int volume, const vpt_sdf_mesh_desc* desc, const vpt_sdf_mesh_region* region, float* positions, float* normals,
    int32_t vertex_capacity, int32_t* quads, int32_t quad_capacity, vpt_sdf_mesh_stats* stats) {
  const char* entry = "vpt_scene_mesh_volume";
  REQUIRE(scene && stats, "%s: null argument", entry);
  const resident& r = resident_of(scene);
  REQUIRE(volume >= 0 && volume < r.d.num_volumes, "%s: volume %d out of range (%d)", entry, volume, r.d.num_volumes);
  const vpt_volume& v = r.m.volumes[(size_t)volume];
  vpt_sdf_mesh_desc own = {{v.whd[0], v.whd[1], v.whd[2]}, {0, 0, 0}, {1, 1, 1}, 0};
  if (desc) {
    REQUIRE(desc->whd[0] == v.whd[0] && desc->whd[1] == v.whd[1] && desc->whd[2] == v.whd[2], "%s: desc->whd is not the volume's (%d x %d x %d)", entry, v.whd[0], v.whd[1],
        v.whd[2]);
    own = *desc;
  } else {
    for (int k = 0; k < 3; k++) own.step[k] = v.res * (float)v.whd[k] / (float)(v.whd[k] > 1 ? v.whd[k] - 1 : 1);
  }
  const mesh_outputs out = {positions, normals, vertex_capacity, quads, quad_capacity};
  if (int rc = validate(entry, &own, out, stats)) return rc;
  if (region)
    if (const char* fault = vpt_sdf_mesh_region_fault(*region, own.whd)) return vpt_set_error(VPT_ERR_INVALID_ARG, "%s: %s", entry, fault);
  const mesh_grid g = grid_of(own, region);
  if (no_cells(g)) return *stats = vpt_sdf_mesh_stats{}, VPT_OK;
  HIP_TRY(hipSetDevice(r.device));
  HIP_TRY(hipDeviceSynchronize());   // launches on any stream may still write the voxels an edit has just handed over
  return mesh_run(entry, r.d.voxels + v.offset, g, out, stats);
}
