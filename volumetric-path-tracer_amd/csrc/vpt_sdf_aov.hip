// vpt_sdf_aov.hip — the first-hit pass of the implicit shaders (include/vpt.h: vpt_render_sdf_aov_device): the one
// instance of its kernel (vpt_sdf_aov_kernel.hip.h), the layout kernels of its planes, and their C-ABI.  Sees a scene through the
// `resident` part of its handle (vpt_resident.h): the tables, the device; nothing of the render side - no schedule, no stack.
#include <algorithm>

#include "vpt_adaptive.h"   // vpt_layout_dparams
#include "vpt_device_buffer.h"
#include "vpt_error.h"
#include "vpt_resident.h"
#include "vpt_sdf_aov.h"
#include "vpt_sdf_aov_kernel.hip.h"

namespace {

// the counterpart of vpt_resolve_ids_kernel for this pass's two id planes: [nranks][nslots] -> row-major, values as they are
__global__ void vpt_resolve_sdf_ids_kernel(DParams pr, const int2* ids_all, const float4* hit_all, int2* rows_ids, float4* rows_hit) {
  int g = blockIdx.x * blockDim.x + threadIdx.x;   // global slot over all ranks
  if (g >= pr.nslots * pr.nranks) return;
  DParams q = pr;
  q.rank    = g / pr.nslots;
  int px, py;
  if (!slot_to_pixel(q, g - q.rank * pr.nslots, px, py)) return;
  const long long idx = (long long)py * pr.width + px;
  rows_ids[idx] = ids_all[g];
  if (hit_all) rows_hit[idx] = hit_all[g];
}

// row-major host-order planes, hits and rng <-> this rank's tile-major slots (vpt_render_sdf_aov); null planes are skipped
__global__ void vpt_sdf_aov_permute_kernel(DParams pr, int to_tiles, sdf_aov_planes tiles, int* tiles_hits, ulonglong2* tiles_rng, sdf_aov_planes rows,
    int* rows_hits, ulonglong2* rows_rng) {
  int slot = blockIdx.x * blockDim.x + threadIdx.x;
  int px, py;
  if (slot >= pr.nslots || !slot_to_pixel(pr, slot, px, py)) return;
  const long long idx = (long long)py * pr.width + px;
  float4* const   t4[4] = {tiles.normal, tiles.albedo, tiles.depth, tiles.hit};
  float4* const   r4[4] = {rows.normal, rows.albedo, rows.depth, rows.hit};
  for (int k = 0; k < 4; k++) {
    if (!t4[k]) continue;
    if (to_tiles) t4[k][slot] = r4[k][idx];
    else r4[k][idx] = t4[k][slot];
  }
  if (tiles.ids) {
    if (to_tiles) tiles.ids[slot] = rows.ids[idx];
    else rows.ids[idx] = tiles.ids[slot];
  }
  if (to_tiles) tiles_hits[slot] = rows_hits[idx], tiles_rng[slot] = rows_rng[idx];
  else rows_hits[idx] = tiles_hits[slot], rows_rng[idx] = tiles_rng[slot];
}

// the conditions on the planes of the pass (include/vpt.h), device or host pointers alike
int check_planes(const vpt_sdf_aov_planes* p) {
  REQUIRE(p, "null planes");
  REQUIRE(p->normal || p->albedo || p->depth || p->ids || p->hit, "planes: every plane is null, nothing to render");
  REQUIRE(p->ids || !p->hit, "planes: hit is given without ids");
  const void* const        given[5] = {p->normal, p->albedo, p->depth, p->ids, p->hit};
  static const char* const name[5]  = {"normal", "albedo", "depth", "ids", "hit"};
  for (int a = 0; a < 5; a++)   // the kernel updates each plane on its own: two of them in one buffer would lose updates
    for (int b = a + 1; b < 5; b++) REQUIRE(!given[a] || given[a] != given[b], "planes: %s and %s share a buffer", name[a], name[b]);
  return VPT_OK;
}
int check_maxiter(const vpt_params* params) {   // the range vpt_kat accepts for a march
  REQUIRE(params->spheretrace_maxiter >= 0 && params->spheretrace_maxiter <= (1 << 20), "params: spheretrace_maxiter %d outside 0 .. %d",
      params->spheretrace_maxiter, 1 << 20);
  return VPT_OK;
}
sdf_aov_planes device_planes(const vpt_sdf_aov_planes& p) { return {(float4*)p.normal, (float4*)p.albedo, (float4*)p.depth, (int2*)p.ids, (float4*)p.hit}; }

}  // namespace

// the pack of a session's pick (vpt_sdf_aov.h)
int vpt_sdf_pick_device(const vpt_scene* s, const void* d_ids_rowmajor, const void* d_hit_rowmajor, long long pixel, void* d_out48, void* stream) {
  REQUIRE(s && d_ids_rowmajor && d_hit_rowmajor && d_out48 && pixel >= 0, "null argument");
  hipLaunchKernelGGL(vpt_sdf_pick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, resident_of(s).d, (const int2*)d_ids_rowmajor,
      (const float4*)d_hit_rowmajor, pixel, (int*)d_out48);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

extern "C" {

int vpt_render_sdf_aov_device(vpt_scene* s, const vpt_params* params, const vpt_layout* layout, int nsamples, const vpt_sdf_aov_planes* planes,
    void* d_hits, void* d_rng, void* stream) {
  if (int rc = check_planes(planes)) return rc;
  REQUIRE(params, "null params");
  REQUIRE(layout, "null layout");
  REQUIRE(d_hits, "null hits");
  REQUIRE(d_rng, "null rng");
  if (int rc = check_maxiter(params)) return rc;
  REQUIRE(nsamples >= 0, "nsamples %d is negative", nsamples);
  DParams pr;
  if (int rc = vpt_layout_dparams(layout, pr)) return rc;
  REQUIRE(s, "null scene");
  const resident& r = resident_of(s);
  REQUIRE(params->camera >= 0 && params->camera < r.d.num_cameras, "camera %d out of range", params->camera);
  if (nsamples == 0) return VPT_OK;
  pr.camera = params->camera, pr.spheretrace_maxiter = params->spheretrace_maxiter;
  pr.preview = params->samples == 1, pr.nsamples = nsamples;
  const size_t lds = (6 * (size_t)r.d.num_sdfs + 7 * (size_t)r.d.num_vol_instances) * sizeof(float4);   // the SDF records, as K2 keeps them
  if (lds > 64 * 1024)
    return vpt_set_error(VPT_ERR_UNSUPPORTED, "scene has too many SDFs for the LDS copy of their records (%d + %d)", r.d.num_sdfs, r.d.num_vol_instances);
  HIP_TRY(hipSetDevice(r.device));
  hipLaunchKernelGGL(vpt_sdf_aov_kernel, dim3((pr.nslots + VPT_BLOCK - 1) / VPT_BLOCK), dim3(VPT_BLOCK), lds, (hipStream_t)stream, r.d, pr,
      device_planes(*planes), (int*)d_hits, (ulonglong2*)d_rng);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

int vpt_resolve_sdf_ids_device(const vpt_layout* layout, const void* d_ids, const void* d_hit, void* d_ids_rowmajor, void* d_hit_rowmajor, void* stream) {
  REQUIRE(layout && d_ids && d_ids_rowmajor, "null argument");
  REQUIRE((d_hit != nullptr) == (d_hit_rowmajor != nullptr), "d_hit and d_hit_rowmajor must be null together");
  DParams pr;
  if (int rc = vpt_layout_dparams(layout, pr)) return rc;
  const long long total = (long long)pr.nslots * pr.nranks;
  REQUIRE(total < (1LL << 31), "image too large");
  hipLaunchKernelGGL(vpt_resolve_sdf_ids_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pr, (const int2*)d_ids,
      (const float4*)d_hit, (int2*)d_ids_rowmajor, (float4*)d_hit_rowmajor);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

int vpt_render_sdf_aov(vpt_scene* s, const vpt_params* params, int nsamples, int width, int height, const vpt_sdf_aov_planes* planes, int32_t* hits,
    uint64_t* rng, int* samples_io) {
  if (int rc = check_planes(planes)) return rc;
  REQUIRE(params, "null params");
  REQUIRE(hits, "null hits");
  REQUIRE(rng, "null rng");
  REQUIRE(samples_io, "null samples_io");
  REQUIRE(width >= 1 && height >= 1 && width < 32768 && height < 32768, "bad image size: width %d, height %d", width, height);
  REQUIRE(nsamples >= 0, "nsamples %d is negative", nsamples);
  if (int rc = check_maxiter(params)) return rc;
  REQUIRE(s, "null scene");
  const resident& r = resident_of(s);
  REQUIRE(params->camera >= 0 && params->camera < r.d.num_cameras, "camera %d out of range", params->camera);
  const int todo = std::min(nsamples, params->samples - *samples_io);   // no-op once reached, as vpt_render
  if (todo <= 0) return VPT_OK;
  HIP_TRY(hipSetDevice(r.device));
  const vpt_layout lay = {width, height, 8, 8, 0, 1};
  DParams          pr;
  if (int rc = vpt_layout_dparams(&lay, pr)) return rc;
  const size_t slots = (size_t)pr.nslots, n = (size_t)width * height;
  // per plane: bytes per entry, the host array, tile-major and row-major device copies
  struct part { size_t bytes; void* host; device_buffer tiles, rows; };
  part parts[7] = {{16, planes->normal}, {16, planes->albedo}, {16, planes->depth}, {8, planes->ids}, {16, planes->hit}, {4, hits}, {16, rng}};
  for (part& p : parts) {
    if (!p.host) continue;
    if (int rc = p.tiles.allocate(slots * p.bytes)) return rc;
    if (int rc = p.rows.allocate(n * p.bytes)) return rc;
    HIP_TRY(hipMemcpyAsync(p.rows.get(), p.host, n * p.bytes, hipMemcpyHostToDevice, nullptr));
  }
  const vpt_sdf_aov_planes tiles = {parts[0].tiles.get(), parts[1].tiles.get(), parts[2].tiles.get(), parts[3].tiles.get(), parts[4].tiles.get()};
  const vpt_sdf_aov_planes rows  = {parts[0].rows.get(), parts[1].rows.get(), parts[2].rows.get(), parts[3].rows.get(), parts[4].rows.get()};
  auto permute = [&](int to_tiles) {
    hipLaunchKernelGGL(vpt_sdf_aov_permute_kernel, dim3((pr.nslots + 255) / 256), dim3(256), 0, nullptr, pr, to_tiles, device_planes(tiles),
        parts[5].tiles.get<int>(), parts[6].tiles.get<ulonglong2>(), device_planes(rows), parts[5].rows.get<int>(), parts[6].rows.get<ulonglong2>());
  };
  permute(1);
  HIP_TRY(hipGetLastError());
  if (int rc = vpt_render_sdf_aov_device(s, params, &lay, todo, &tiles, parts[5].tiles.get(), parts[6].tiles.get(), nullptr)) return rc;
  permute(0);
  HIP_TRY(hipGetLastError());
  for (part& p : parts)
    if (p.host) HIP_TRY(hipMemcpyAsync(p.host, p.rows.get(), n * p.bytes, hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  *samples_io += todo;
  return VPT_OK;
}

}  // extern "C"
