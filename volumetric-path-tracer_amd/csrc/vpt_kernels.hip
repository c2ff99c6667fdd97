// vpt_kernels.hip — the kernels outside K1 and K2 (declared in vpt_launch.h): vpt_intersect, the known-answer-test kernel and the
// self-tests, the light setup of vpt_scene_create, the launch schedule's cost average, and the elementwise state kernels.
#include "vpt_kat_kernels.hip.h"
#include "vpt_srgb.hip.h"

// vpt_kat (vpt_kat_kernels.hip.h)
template __global__ void vpt_kat_kernel<true>(DScene, int, int, int, int, int, const float*, const int*, float*, stack_cfg, int);
template __global__ void vpt_kat_kernel<false>(DScene, int, int, int, int, int, const float*, const int*, float*, stack_cfg, int);

// light_prims of the single-leaf mesh lights (vpt_device.h): one thread per (light, primitive of the leaf)
__global__ void vpt_light_setup_kernel(DScene sc, float4* out) {
  int l = blockIdx.x, k = threadIdx.x;
  if (l >= sc.num_lights || k >= 4) return;
  float4 r7 = sc.light_rec[8 * l + 7];
  if ((__float_as_int(r7.w) & 255) != VPT_LIGHT_SMALL_MESH || k >= ((__float_as_int(r7.w) >> 8) & 15)) return;
  const DInstance& inst = sc.instances[sc.lights[l].instance];
  const DShape&    sh   = sc.shapes[inst.shape];
  const float4*    leaf = sc.leaf_prims + 4 * ((long long)sh.leaf_offset + ((~sh.root_ref) >> 4) + k);
  f3 n = eval_element_normal(sc, inst, __float_as_int(leaf[0].w));
  for (int c = 0; c < 4; c++) out[20 * l + 5 * k + c] = leaf[c];
  out[20 * l + 5 * k + 4] = make_float4(n.x, n.y, n.z, __int_as_float(sh.is_triangles ? 1 : 0));
}

// medium records (vpt_device.h): one thread per material.  The kernels' own eval_material_at, compiled with their flags, without
// textures' or vertex colours' say (a scene where they have one renders with the instance that does not read the records): the
// bits a path copies at a hit on the material.  The texture ids are dropped, not followed: those of a material no mesh instance
// uses (an SDF's) are not range-checked (prep_check_material)
__global__ void vpt_medium_setup_kernel(DScene sc, float4* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sc.num_materials) return;
  vpt_material mat = sc.materials[i];
  mat.emission_tex = mat.color_tex = mat.roughness_tex = mat.scattering_tex = VPT_INVALID;
  const mpoint m = eval_material_at(sc, mat, mk2(0, 0), mk4(1, 1, 1, 1));
  out[3 * i]     = make_float4(m.density.x, m.density.y, m.density.z, m.scattering.x);
  out[3 * i + 1] = make_float4(m.scattering.y, m.scattering.z, m.emission.x, m.emission.y);
  out[3 * i + 2] = make_float4(m.emission.z, m.scanisotropy, 0, 0);
}

// search_light_cdf against the plain binary search on the same CDF: values at, just below and just above CDF
// entries, uniform ones, and the ends of the range; out[0] = mismatches
__global__ void vpt_light_cdf_selftest_kernel(DScene sc, int light_id, int n, unsigned long long* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  const vpt_light& light = sc.lights[light_id];
  const float*     cdf   = sc.light_cdf + light.cdf_offset;
  const int        len   = light.cdf_len;
  float back = cdf[len - 1];
  // the wave votes inside search_light_cdf: keep all lanes in, flag the surplus ones instead of returning
  bool     live = i < n;
  unsigned h    = (unsigned)i * 2654435761u + 12345u;
  h ^= h >> 15, h *= 2246822519u, h ^= h >> 13;
  float v = cdf[h % (unsigned)len];
  switch (i & 7) {
    case 0: break;
    case 1: v = __uint_as_float(__float_as_uint(v) - (v > 0 ? 1u : 0u)); break;
    case 2: v = __uint_as_float(__float_as_uint(v) + 1u); break;
    case 3: v = 0.0f; break;
    case 4: v = back; break;
    default: v = back * ((h >> 8) * (1.0f / 16777216.0f)); break;
  }
  float r = clampf(v, 0.0f, back - 0.00001f);
  int a = search_light_cdf(sc, light_id, r);
  int lo = 0, cnt = len;   // std::upper_bound, as sample_discrete
  while (cnt > 0) {
    int half = cnt >> 1;
    if (!(r < cdf[lo + half])) lo += half + 1, cnt -= half + 1;
    else cnt = half;
  }
  int b = lo < len ? lo : len - 1;
  if (live && a != b) atomicAdd(&out[0], 1ull);
}

// Launch schedule: a wave's duration varies by +-17 % from one launch to the next on the same tile (it depends on which waves shared its SIMD:
// profiles/r04_k2_lane_histogram.txt), and longest-first scheduling on such estimates ends well above its bound (K2: 225 ms against 203).  The order is
// therefore taken from a running average of the duration PER SAMPLE (weight = samples seen, capped), whose bit pattern - positive floats - is the sort key.
__global__ void vpt_cost_average_kernel(const unsigned* __restrict__ cost, float* __restrict__ avg, unsigned* __restrict__ key, int n, float nsamples, float weight) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float per_sample = (float)cost[i] / nsamples;
  float a = weight > 0 ? (avg[i] * weight + per_sample * nsamples) / (weight + nsamples) : per_sample;
  avg[i] = a;
  key[i] = __float_as_uint(a);
}

// vpt_intersect: one lane per ray through the production traversal (COMPACT: the leaf records of a scene of triangles, as the path tracers read them)
template <bool SPILL, bool COMPACT>
__global__ void vpt_intersect_kernel(DScene sc, int n, const float* rays, int instance,
    int* ids, float* uvt, stack_cfg stack) {
  extern __shared__ int lds_stack[];
  const lane_stack2<SPILL> stk = make_lane_stack<SPILL>(lds_stack, stack);
  int i = blockIdx.x * VPT_BLOCK + threadIdx.x;
  const bool live = i < n;   // the whole wave goes through the query (traverse(): the group forms need every lane); surplus lanes carry no ray
  if (!live) i = 0;
  hit_t h = traverse<COMPACT>(sc, live, mk3(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2]), mk3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]), instance, stk);
  if (!live) return;
  ids[2 * i] = h.hit ? h.instance : -1, ids[2 * i + 1] = h.hit ? h.element : -1;
  uvt[3 * i] = h.hit ? h.uv.x : 0, uvt[3 * i + 1] = h.hit ? h.uv.y : 0, uvt[3 * i + 2] = h.hit ? h.distance : 0;
}
template __global__ void vpt_intersect_kernel<true, true>(DScene, int, const float*, int, int*, float*, stack_cfg);
template __global__ void vpt_intersect_kernel<false, true>(DScene, int, const float*, int, int*, float*, stack_cfg);
template __global__ void vpt_intersect_kernel<true, false>(DScene, int, const float*, int, int*, float*, stack_cfg);
template __global__ void vpt_intersect_kernel<false, false>(DScene, int, const float*, int, int*, float*, stack_cfg);

// all 2^32 operands of rcp_newton (vpt_mesh_kernel.hip.h) against the IEEE quotient; out[0] = mismatches, out[1] = out of range
__global__ void vpt_reciprocal_selftest_kernel(unsigned long long* out) {
  unsigned long long bad = 0, skipped = 0;
  for (unsigned long long b = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; b < (1ull << 32); b += (unsigned long long)gridDim.x * blockDim.x) {
    float x = __uint_as_float((unsigned)b), a = __builtin_fabsf(x);
    if (!rcp_in_range(a, a)) { skipped++; continue; }
    if (__float_as_uint(rcp_newton(x)) != __float_as_uint(1.0f / x)) bad++;
  }
  if (bad) atomicAdd(&out[0], bad);
  if (skipped) atomicAdd(&out[1], skipped);
}

// ---- output resolve (the plain layout copies: vpt_layout.hip) ---------------------------------------------
// get_render (cpp:1105-1116) over the gathered buffers of all ranks: [nranks][nslots] -> row-major * 1/samples
__global__ void vpt_resolve_kernel(DParams pr, const float4* tiles_all, float scale, float4* rows_image) {
  int g = blockIdx.x * blockDim.x + threadIdx.x;   // global slot over all ranks
  if (g >= pr.nslots * pr.nranks) return;
  DParams q = pr;
  q.rank    = g / pr.nslots;
  int px, py;
  if (!slot_to_pixel(q, g - q.rank * pr.nslots, px, py)) return;
  float4 v = tiles_all[g];
  rows_image[(long long)py * pr.width + px] = make_float4(v.x * scale, v.y * scale, v.z * scale, v.w * scale);
}

// The output stage of a preview on the device: get_render (cpp:1105-1116) followed by rgb_to_srgb
// (yocto_color.h:228-231) and float_to_byte (:207-211), both in vpt_srgb.hip.h; alpha is quantised
// linearly, as save_image does.
__global__ void vpt_resolve_srgb8_kernel(DParams pr, const float4* tiles_all, float scale, uchar4* rows_rgba8) {
  int g = blockIdx.x * blockDim.x + threadIdx.x;   // global slot over all ranks
  if (g >= pr.nslots * pr.nranks) return;
  DParams q = pr;
  q.rank    = g / pr.nslots;
  int px, py;
  if (!slot_to_pixel(q, g - q.rank * pr.nslots, px, py)) return;
  float4 v = tiles_all[g];
  rows_rgba8[(long long)py * pr.width + px] =
      make_uchar4(srgb_quant(srgb_curve(v.x * scale)), srgb_quant(srgb_curve(v.y * scale)), srgb_quant(srgb_curve(v.z * scale)), srgb_quant(v.w * scale));
}
