// vpt_sdf_aov.hip — the first-hit pass of the implicit shaders (include/vpt.h: vpt_render_sdf_aov_device): the one
// instance of its kernel (vpt_sdf_aov_kernel.hip.h), the pack of a session's pick, and their C-ABI; the layout copies of its planes
// are vpt_layout.hip's.  Sees a scene through the
// `resident` part of its handle (vpt_resident.h): the tables, the device; nothing of the render side - no schedule, no stack.
#include <algorithm>

#include "vpt_error.h"
#include "vpt_layout.h"
#include "vpt_resident.h"
#include "vpt_sdf_aov.h"
#include "vpt_sdf_aov_kernel.hip.h"

namespace {

// the conditions on the planes of the pass (include/vpt.h), device or host pointers alike
int check_given(const vpt_sdf_aov_planes* p) {
  REQUIRE(p, "null planes");
  const void* const        given[5] = {p->normal, p->albedo, p->depth, p->ids, p->hit};
  static const char* const name[5]  = {"normal", "albedo", "depth", "ids", "hit"};
  return check_plane_set(name, given, 5, 3, 4);
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
  if (int rc = check_given(planes)) return rc;
  REQUIRE(params, "null params");
  REQUIRE(layout, "null layout");
  REQUIRE(d_hits, "null hits");
  REQUIRE(d_rng, "null rng");
  if (int rc = check_maxiter(params)) return rc;
  REQUIRE(nsamples >= 0, "nsamples %d is negative", nsamples);
  DParams pr;
  if (int rc = make_dparams(params, layout, nsamples, pr)) return rc;
  REQUIRE(s, "null scene");
  const resident& r = resident_of(s);
  REQUIRE(params->camera >= 0 && params->camera < r.d.num_cameras, "camera %d out of range", params->camera);
  if (nsamples == 0) return VPT_OK;
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
  const layout_plane planes[2] = {{(void*)d_ids, d_ids_rowmajor, 8}, {(void*)d_hit, d_hit_rowmajor, 16}};
  return layout_copy(layout, LAYOUT_ALL_TILES_TO_ROWS, planes, d_hit ? 2 : 1, (hipStream_t)stream);
}

int vpt_render_sdf_aov(vpt_scene* s, const vpt_params* params, int nsamples, int width, int height, const vpt_sdf_aov_planes* planes, int32_t* hits,
    uint64_t* rng, int* samples_io) {
  if (int rc = check_given(planes)) return rc;
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
  const vpt_layout lay      = {width, height, 8, 8, 0, 1};
  const host_plane parts[7] = {{planes->normal, 16}, {planes->albedo, 16}, {planes->depth, 16}, {planes->ids, 8}, {planes->hit, 16}, {hits, 4},
      {rng, 16}};
  if (int rc = layout_round_trip(lay, parts, 7, nullptr, [&](const vpt_layout* l, void* const* t) {
        const vpt_sdf_aov_planes tiles = {t[0], t[1], t[2], t[3], t[4]};
        return vpt_render_sdf_aov_device(s, params, l, todo, &tiles, t[5], t[6], nullptr);
      }))
    return rc;
  *samples_io += todo;
  return VPT_OK;
}

}  // extern "C"
