// vpt_volgrid_aov.hip — the first-collision pass of the volgrid shader (include/vpt.h: vpt_render_volgrid_aov_device): the
// three instances of its kernel (vpt_volgrid_aov_kernel.hip.h), the pack of a session's pick, and their C-ABI; the layout copies of its
// planes are vpt_layout.hip's.  It takes K3's tables from the scene handle as a volgrid launch does (volgrid_prepare, volgrid_arguments):
// the refusals of a render are its refusals, and a stale table is rebuilt first.
#include <algorithm>

#include "vpt_scene_handle.h"
#include "vpt_volgrid_aov.h"
#include "vpt_volgrid_aov_kernel.hip.h"

template __global__ void vpt_volgrid_aov_kernel<VA_OPACITY>(DScene, DParams, volgrid_args, volgrid_aov_planes, int* __restrict__, ulonglong2* __restrict__);
template __global__ void vpt_volgrid_aov_kernel<VA_IDS>(DScene, DParams, volgrid_args, volgrid_aov_planes, int* __restrict__, ulonglong2* __restrict__);
template __global__ void vpt_volgrid_aov_kernel<VA_ALL>(DScene, DParams, volgrid_args, volgrid_aov_planes, int* __restrict__, ulonglong2* __restrict__);

namespace {

// the conditions on the planes of the pass (include/vpt.h), device or host pointers alike
int check_given(const vpt_volgrid_aov_planes* p) {
  REQUIRE(p, "null planes");
  const void* const        given[6] = {p->opacity, p->albedo, p->depth, p->normal, p->ids, p->hit};
  static const char* const name[6]  = {"opacity", "albedo", "depth", "normal", "ids", "hit"};
  return check_plane_set(name, given, 6, 4, 5);
}
volgrid_aov_planes device_planes(const vpt_volgrid_aov_planes& p) {
  return {(float4*)p.opacity, (float4*)p.albedo, (float4*)p.depth, (float4*)p.normal, (int2*)p.ids, (float4*)p.hit};
}

}  // namespace

// the pack of a session's pick (vpt_volgrid_aov.h)
int vpt_volgrid_pick_device(const vpt_scene* s, const void* d_ids_rowmajor, const void* d_hit_rowmajor, long long pixel, void* d_out48, void* stream) {
  REQUIRE(s && d_ids_rowmajor && d_hit_rowmajor && d_out48 && pixel >= 0, "null argument");
  REQUIRE(s->volgrid.built_edits == s->edit_generation, "volgrid pick: the tables are older than the scene (no pass has run since its last edit)");
  hipLaunchKernelGGL(vpt_volgrid_pick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, s->d, volgrid_arguments(s), (const int2*)d_ids_rowmajor,
      (const float4*)d_hit_rowmajor, pixel, (int*)d_out48);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

extern "C" {

int vpt_render_volgrid_aov_device(vpt_scene* s, const vpt_params* params, const vpt_layout* layout, int nsamples, const vpt_volgrid_aov_planes* planes,
    void* d_hits, void* d_rng, void* stream) {
  if (int rc = check_given(planes)) return rc;
  REQUIRE(params, "null params");
  REQUIRE(layout, "null layout");
  REQUIRE(d_hits, "null hits");
  REQUIRE(d_rng, "null rng");
  REQUIRE(nsamples >= 0, "nsamples %d is negative", nsamples);
  DParams pr;
  if (int rc = make_dparams(params, layout, nsamples, pr)) return rc;
  REQUIRE(s, "null scene");
  if (int rc = check_camera(s, params)) return rc;
  if (nsamples == 0) return VPT_OK;
  HIP_TRY(hipSetDevice(s->device));
  if (int rc = volgrid_prepare(s, (hipStream_t)stream)) return rc;   // a medium without a usable trdepth: refused as a render refuses it
  const volgrid_args va  = volgrid_arguments(s);
  const size_t       lds = (size_t)va.num_instances * sizeof(vpt_volgrid_record);   // (volgrid_prepare has checked that they fit)
  const int want = (planes->opacity ? VA_OPACITY : 0) | (planes->albedo ? VA_ALBEDO : 0) | (planes->depth ? VA_DEPTH : 0) |
                   (planes->normal ? VA_NORMAL : 0) | (planes->ids ? VA_IDS : 0);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((pr.nslots + VPT_BLOCK - 1) / VPT_BLOCK)), dim3(VPT_BLOCK), lds, (hipStream_t)stream, s->d, pr, va,
        device_planes(*planes), (int*)d_hits, (ulonglong2*)d_rng);
  };
  // the smallest instance that covers the request
  if (want == VA_OPACITY) launch(vpt_volgrid_aov_kernel<VA_OPACITY>);
  else if (want == VA_IDS) launch(vpt_volgrid_aov_kernel<VA_IDS>);
  else launch(vpt_volgrid_aov_kernel<VA_ALL>);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

// (the plane-list kernel of vpt_layout.hip serves ids / hit of this pass unchanged: both are int32 x2 and float4 per slot)
int vpt_resolve_volgrid_ids_device(const vpt_layout* layout, const void* d_ids, const void* d_hit, void* d_ids_rowmajor, void* d_hit_rowmajor, void* stream) {
  return vpt_resolve_sdf_ids_device(layout, d_ids, d_hit, d_ids_rowmajor, d_hit_rowmajor, stream);
}

int vpt_render_volgrid_aov(vpt_scene* s, const vpt_params* params, int nsamples, int width, int height, const vpt_volgrid_aov_planes* planes,
    int32_t* hits, uint64_t* rng, int* samples_io) {
  if (int rc = check_given(planes)) return rc;
  REQUIRE(params, "null params");
  REQUIRE(hits, "null hits");
  REQUIRE(rng, "null rng");
  REQUIRE(samples_io, "null samples_io");
  REQUIRE(width >= 1 && height >= 1 && width < 32768 && height < 32768, "bad image size: width %d, height %d", width, height);
  REQUIRE(nsamples >= 0, "nsamples %d is negative", nsamples);
  REQUIRE(s, "null scene");
  if (int rc = check_camera(s, params)) return rc;
  const int todo = std::min(nsamples, params->samples - *samples_io);   // no-op once reached, as vpt_render
  if (todo <= 0) return VPT_OK;
  HIP_TRY(hipSetDevice(s->device));
  const vpt_layout lay      = {width, height, 8, 8, 0, 1};
  const host_plane parts[8] = {{planes->opacity, 16}, {planes->albedo, 16}, {planes->depth, 16}, {planes->normal, 16}, {planes->ids, 8},
      {planes->hit, 16}, {hits, 4}, {rng, 16}};
  if (int rc = layout_round_trip(lay, parts, 8, nullptr, [&](const vpt_layout* l, void* const* t) {
        const vpt_volgrid_aov_planes tiles = {t[0], t[1], t[2], t[3], t[4], t[5]};
        return vpt_render_volgrid_aov_device(s, params, l, todo, &tiles, t[6], t[7], nullptr);
      }))
    return rc;
  *samples_io += todo;
  return vpt_check_watchdog(s);   // a flight that ran into VPT_VOLGRID_MAX_STEPS: reported as a render reports it
}

}  // extern "C"
