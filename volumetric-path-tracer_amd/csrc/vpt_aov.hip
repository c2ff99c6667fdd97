// vpt_aov.hip — the first-hit pass of the mesh shaders (include/vpt.h: vpt_render_aov_device): the instances of its
// kernel (vpt_aov_kernel.hip.h) for scenes of faces - those for scenes with points or lines are vpt_k1_curves.hip's - and its C-ABI;
// the layout copies of its planes are vpt_layout.hip's.  The twin of vpt_sdf_aov.hip, but over the BVHs: it takes the traversal setup
// of the scene handle's render side (vpt_scene_handle.h).
#include <algorithm>

#include "vpt_aov_kernel.hip.h"
#include "vpt_scene_handle.h"

VPT_AOV_DEFINE(true, false)
VPT_AOV_DEFINE(false, false)
extern VPT_AOV_DEFINE(true, true)
extern VPT_AOV_DEFINE(false, true)

// the conditions on the planes of the pass (include/vpt.h), device or host pointers alike
static int check_given(const vpt_aov_planes* p) {
  REQUIRE(p, "null planes");
  const void* const        given[6] = {p->normal, p->albedo, p->texcoord, p->depth, p->ids, p->uvt};
  static const char* const name[6]  = {"normal", "albedo", "texcoord", "depth", "ids", "uvt"};
  return check_plane_set(name, given, 6, 4, 5);
}
static aov_planes device_planes(const vpt_aov_planes& p) {
  return {(float4*)p.normal, (float4*)p.albedo, (float4*)p.texcoord, (float4*)p.depth, (int2*)p.ids, (float*)p.uvt};
}

extern "C" {

int vpt_render_aov_device(vpt_scene* s, const vpt_params* params, const vpt_layout* layout, int nsamples, const vpt_aov_planes* planes,
    void* d_hits, void* d_rng, void* stream) {
  if (int rc = check_given(planes)) return rc;
  REQUIRE(s && params && layout && d_hits && d_rng, "null argument");
  if (int rc = check_camera(s, params)) return rc;
  REQUIRE(nsamples >= 0, "negative sample count");
  if (nsamples == 0) return VPT_OK;
  DParams pr;
  if (int rc = make_dparams(params, layout, nsamples, pr)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  traversal_launch t;
  if (int rc = traversal_setup(s, pr.nslots, t)) return rc;
  auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, t.grid, dim3(VPT_BLOCK), t.lds, (hipStream_t)stream, s->d, pr, device_planes(*planes), (int*)d_hits, (ulonglong2*)d_rng, t.stack); };
  with_flags([&](auto spill, auto curves) { launch(vpt_aov_kernel<spill, curves>); }, t.stack.spill, s->curves);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

int vpt_resolve_ids_device(const vpt_layout* layout, const void* d_ids, const void* d_uvt, void* d_ids_rowmajor, void* d_uvt_rowmajor, void* stream) {
  REQUIRE(layout && d_ids && d_ids_rowmajor, "null argument");
  REQUIRE((d_uvt != nullptr) == (d_uvt_rowmajor != nullptr), "d_uvt and d_uvt_rowmajor must be null together");
  const layout_plane planes[2] = {{(void*)d_ids, d_ids_rowmajor, 8}, {(void*)d_uvt, d_uvt_rowmajor, 12}};
  return layout_copy(layout, LAYOUT_ALL_TILES_TO_ROWS, planes, d_uvt ? 2 : 1, (hipStream_t)stream);
}

int vpt_render_aov(vpt_scene* s, const vpt_params* params, int nsamples, int width, int height, const vpt_aov_planes* planes, int32_t* hits,
    uint64_t* rng, int* samples_io) {
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
  const host_plane parts[8] = {{planes->normal, 16}, {planes->albedo, 16}, {planes->texcoord, 16}, {planes->depth, 16}, {planes->ids, 8},
      {planes->uvt, 12}, {hits, 4}, {rng, 16}};
  if (int rc = layout_round_trip(lay, parts, 8, nullptr, [&](const vpt_layout* l, void* const* t) {
        const vpt_aov_planes tiles = {t[0], t[1], t[2], t[3], t[4], t[5]};
        return vpt_render_aov_device(s, params, l, todo, &tiles, t[6], t[7], nullptr);
      }))
    return rc;
  *samples_io += todo;
  return VPT_OK;
}

}  // extern "C"
