// vpt_probes.hip — the probes and self-tests of the C-ABI (include/vpt.h, include/vpt_kat.h): vpt_intersect, the known-answer-test
// entry points with their id checks and record strides, vpt_spheretrace, vpt_eval_lobes and the two self-tests.  Host code only: the
// kernels are vpt_kernels.hip's (vpt_intersect on scenes with points or lines: vpt_k1_curves.hip's), so a change to an id check
// recompiles none of them.
#include <algorithm>
#include <cstring>
#include <vector>

#include "vpt_kat.h"
#include "vpt_scene_handle.h"

extern "C" {

int vpt_selftest_reciprocal(int device, unsigned long long* mismatches, unsigned long long* fallbacks) {
  REQUIRE(mismatches && fallbacks, "null argument");
  HIP_TRY(hipSetDevice(device));
  device_buffer d;
  if (int rc = d.allocate(16)) return rc;
  HIP_TRY(hipMemset(d.get(), 0, 16));
  hipLaunchKernelGGL(vpt_reciprocal_selftest_kernel, dim3(4096), dim3(256), 0, 0, d.get<unsigned long long>());
  unsigned long long h[2] = {0, 0};
  int rc = hipMemcpy(h, d.get(), 16, hipMemcpyDeviceToHost) == hipSuccess ? VPT_OK : vpt_set_error(VPT_ERR_HIP, "reciprocal self-test failed to run");
  *mismatches = h[0], *fallbacks = h[1];
  return rc;
}

int vpt_intersect(vpt_scene* s, int n, const float* rays, int instance, int32_t* ids, float* uvt) {
  REQUIRE(s && rays && ids && uvt && n >= 0, "bad argument");
  REQUIRE(instance >= -1 && instance < s->d.num_instances, "instance %d out of range", instance);
  REQUIRE(instance < 0 || s->h.slot_of[(size_t)instance] >= 0, "instance %d is not in the scene BVH", instance);
  if (n == 0) return VPT_OK;
  HIP_TRY(hipSetDevice(s->device));
  device_buffer d_rays, d_ids, d_uvt;
  if (d_rays.allocate((size_t)n * 24) || d_ids.allocate((size_t)n * 8) || d_uvt.allocate((size_t)n * 12) ||
      hipMemcpy(d_rays.get(), rays, (size_t)n * 24, hipMemcpyHostToDevice) != hipSuccess)
    return vpt_set_error(VPT_ERR_HIP, "vpt_intersect: device buffers");
  traversal_launch t;
  if (int rc = traversal_setup(s, n, t)) return rc;
  auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, t.grid, dim3(VPT_BLOCK), t.lds, 0, s->d, n, d_rays.get<const float>(), instance, d_ids.get<int>(), d_uvt.get<float>(), t.stack); };
  // points or lines: the leaf tests of the VPT_FEAT_CURVES instances, a kernel of its own; else COMPACT on a scene of triangles: through
  // the short leaf records, as its path tracers go
  if (s->curves) with_flags([&](auto spill) { launch(vpt_intersect_curves_kernel<spill>); }, t.stack.spill);
  else with_flags([&](auto spill, auto compact) { launch(vpt_intersect_kernel<spill, compact>); }, t.stack.spill, s->d.tri_prims != nullptr);
  bool ok = hipMemcpy(ids, d_ids.get(), (size_t)n * 8, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(uvt, d_uvt.get(), (size_t)n * 12, hipMemcpyDeviceToHost) == hipSuccess;
  return ok ? VPT_OK : vpt_set_error(VPT_ERR_HIP, "vpt_intersect failed to run");
}

// ---- known-answer-test entry points (include/vpt_kat.h) ------------------------------------------------------------
static const int k_kat_strides[VPT_KAT_OP_COUNT][2] = {{19, 22}, {15, 10}, {4, 4}, {5, 6}, {7, 5}, {7, 24}, {3, 3}, {7, 3}, {6, 1},
    {6, 1}, {4, 3}, {6, 3}, {7, 4}, {4, 1}, {4, 1}};

int vpt_kat_strides(int op, int* in_stride, int* out_stride) {
  REQUIRE(op >= 0 && op < VPT_KAT_OP_COUNT && in_stride && out_stride, "unknown KAT op %d", op);
  *in_stride = k_kat_strides[op][0], *out_stride = k_kat_strides[op][1];
  return VPT_OK;
}

int vpt_kat(vpt_scene* s, int op, int iparam, int n, const float* in, float* out) {
  REQUIRE(s && n >= 0 && (n == 0 || (in && out)), "bad argument");
  REQUIRE(op >= 0 && op < VPT_KAT_OP_COUNT, "unknown KAT op %d", op);
  // vpt_kat_kernel's traverse and eval_surface_point are the instances without VPT_FEAT_CURVES: they would read point and line leaf
  // records as quads
  if (s->curves && (op == VPT_KAT_INTERSECT || op == VPT_KAT_SURFACE))
    return vpt_set_error(VPT_ERR_UNSUPPORTED, "KAT op %d on a scene with points or lines: vpt_intersect and the AOV pass (vpt_render_aov) are the ways in", op);
  if (n == 0) return VPT_OK;
  const int si = k_kat_strides[op][0], so = k_kat_strides[op][1];
  const DScene& D = s->d;
  // every id a record carries is checked here, so that no batch can index outside the scene's tables
  std::vector<int> aux((size_t)n, 0);
  auto id_ok = [](float v, int count) { return v >= 0 && v < (float)count && v == (float)(int)v; };
  for (int i = 0; i < n; i++) {
    const float* a = in + (size_t)i * si;
    bool ok = true;
    switch (op) {
      case VPT_KAT_LOBES: ok = id_ok(a[0], VPT_MAT_GLTFPBR + 1); break;
      case VPT_KAT_TEXTURE: ok = id_ok(a[0], D.num_textures); break;
      case VPT_KAT_CAMERA: ok = id_ok(a[0], D.num_cameras); break;
      case VPT_KAT_INTERSECT: ok = a[6] == -1.0f || (id_ok(a[6], D.num_instances) && s->h.slot_of[(size_t)a[6]] >= 0); break;
      case VPT_KAT_SURFACE:
        ok = id_ok(a[0], D.num_instances) && id_ok(a[1], s->h.shape_elems[(size_t)s->h.inst_shape[(size_t)a[0]]]);
        if (ok) aux[(size_t)i] = s->h.prim_slot[(size_t)s->h.shape_elem_offset[(size_t)s->h.inst_shape[(size_t)a[0]]] + (size_t)a[1]];
        break;
      case VPT_KAT_SAMPLE_LIGHTS:
      case VPT_KAT_LIGHTS_PDF:
      case VPT_KAT_LIGHTS_PDF_K2: ok = D.num_lights > 0; break;
      case VPT_KAT_SDF_NORMAL: ok = a[0] == 0.0f ? id_ok(a[1], D.num_vol_instances) : (a[0] == 1.0f && id_ok(a[1], D.num_sdfs)); break;
      case VPT_KAT_SPHERETRACE: ok = a[6] == -1.0f || id_ok(a[6], D.num_sdfs); break;
      case VPT_KAT_VOLUME: ok = id_ok(a[0], D.num_volumes); break;
      case VPT_KAT_SDF_FUNCTION: ok = id_ok(a[0], D.num_sdfs); break;
      default: break;
    }
    REQUIRE(ok, "KAT op %d record %d: id out of range", op, i);
  }
  REQUIRE((op != VPT_KAT_LIGHTS_PDF && op != VPT_KAT_LIGHTS_PDF_K2 && op != VPT_KAT_SPHERETRACE) || (iparam >= 0 && iparam <= (1 << 20)),
      "KAT op %d: iteration limit %d out of range", op, iparam);
  HIP_TRY(hipSetDevice(s->device));
  device_buffer d_in, d_out, d_aux;
  if (d_in.allocate((size_t)n * si * 4) || d_out.allocate((size_t)n * so * 4) || d_aux.allocate((size_t)n * 4) ||
      hipMemcpy(d_in.get(), in, (size_t)n * si * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_aux.get(), aux.data(), (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess)
    return vpt_set_error(VPT_ERR_HIP, "vpt_kat: device buffers");
  traversal_launch t;
  if (int rc = traversal_setup(s, n, t)) return rc;
  const size_t lds = std::max(t.lds, (size_t)s->stack_cap * VPT_BLOCK * sizeof(int));   // the ops of K2's code path walk with the refs-only stack
  with_flags([&](auto spill) { hipLaunchKernelGGL(vpt_kat_kernel<spill>, t.grid, dim3(VPT_BLOCK), lds, 0, s->d, op, iparam, n, si, so, d_in.get<const float>(), d_aux.get<const int>(), d_out.get<float>(), t.stack, s->stack_cap); }, t.stack.spill);
  bool ok = hipGetLastError() == hipSuccess && hipMemcpy(out, d_out.get(), (size_t)n * so * 4, hipMemcpyDeviceToHost) == hipSuccess;
  return ok ? VPT_OK : vpt_set_error(VPT_ERR_HIP, "vpt_kat failed to run");
}

int vpt_spheretrace(vpt_scene* s, int n, const float* rays, int sdf, int maxiter, int32_t* ids, float* t) {
  REQUIRE(s && n >= 0 && (n == 0 || (rays && ids && t)), "bad argument");
  std::vector<float> in((size_t)n * 7), out((size_t)n * 4);
  for (int i = 0; i < n; i++) {
    memcpy(&in[(size_t)i * 7], rays + (size_t)i * 6, 24);
    in[(size_t)i * 7 + 6] = (float)(sdf < 0 ? -1 : sdf);
  }
  if (int rc = vpt_kat(s, VPT_KAT_SPHERETRACE, maxiter, n, in.data(), out.data())) return rc;
  for (int i = 0; i < n; i++) {
    ids[3 * (size_t)i] = (int)out[4 * (size_t)i], ids[3 * (size_t)i + 1] = (int)out[4 * (size_t)i + 2], ids[3 * (size_t)i + 2] = (int)out[4 * (size_t)i + 3];
    t[i] = out[4 * (size_t)i + 1];
  }
  return VPT_OK;
}

int vpt_eval_lobes(vpt_scene* s, int n, const float* in19, float* out22) { return vpt_kat(s, VPT_KAT_LOBES, 0, n, in19, out22); }

int vpt_selftest_light_cdf(vpt_scene* s, int light, int n, unsigned long long* mismatches, int* indexed) {
  REQUIRE(s && mismatches && indexed && n > 0, "bad argument");
  REQUIRE(light >= 0 && light < s->d.num_lights, "light %d out of range", light);
  HIP_TRY(hipSetDevice(s->device));
  DCdfIndex ix;
  HIP_TRY(hipMemcpy(&ix, s->d.light_index + light, sizeof(ix), hipMemcpyDeviceToHost));
  *indexed = ix.levels > 0 ? (ix.guide_buckets > 0 ? 2 : 1) : 0, *mismatches = 0;
  if (!ix.levels) return VPT_OK;   // short CDFs use the reference's binary search itself
  device_buffer d;
  if (int rc = d.allocate(8)) return rc;
  HIP_TRY(hipMemset(d.get(), 0, 8));
  hipLaunchKernelGGL(vpt_light_cdf_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, s->d, light, n, d.get<unsigned long long>());
  return hipMemcpy(mismatches, d.get(), 8, hipMemcpyDeviceToHost) == hipSuccess ? VPT_OK : vpt_set_error(VPT_ERR_HIP, "light CDF self-test failed to run");
}

}  // extern "C"
