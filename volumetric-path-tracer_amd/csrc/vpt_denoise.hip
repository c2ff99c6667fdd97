// vpt_denoise.hip — the guided à-trous filter behind denoise_render (include/vpt.h: vpt_denoise, vpt_denoise_device,
// vpt_half_variance_device).  The arithmetic is the rule include/vpt.h states, operation for operation and in its order
// (-ffp-contract=off; float32 / and sqrt are correctly rounded), so the host mirror (host/vpt_denoise.cpp) gives the same bits.
// Two forms of a pass, same bits:
//   plain  one lane per pixel, a wave = 64 pixels of one row, every tap a 16-byte load from global memory;
//   tiled  a workgroup stages a 64 x 8 pixel tile with its halo of 2 s pixels in LDS (colour and guides as float4, variance and
//          luminance as float: a wave reads 64 consecutive entries of one row, so no bank is asked twice) and takes the taps
//          from there; the luminance of a pixel is divided out once when it is staged, not once per tap.  Strides 1 and 2.
// VPT_DENOISE_PLAIN=1 (read per call) runs every pass in the plain form: the tests' A/B switch.
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "vpt_device_buffer.h"
#include "vpt_error.h"

namespace {
#define DN_DEV __device__ __forceinline__

constexpr int k_tile_w = 64, k_tile_h = 8, k_block = 256;   // tiled form: each lane owns rows ty and ty + 4 of its column
constexpr int k_max_tiled_stride = 2;

struct pass_args {
  const float4* c_in;
  const float*  v_in;
  const float4* normal;
  const float4* albedo;
  float4*       c_out;
  float*        v_out;   // null on the last pass: nobody reads its variance
  int           width, height;
  float         sigma_l, r_normal, r_albedo;   // r_*: 1 / sigma^2, divided out once per call
};

DN_DEV float lum(float4 c) { return ((c.x + c.y) + c.z) / 3.0f; }
DN_DEV float d2(float4 a, float4 b) {
  const float x = a.x - b.x, y = a.y - b.y, z = a.z - b.z, w = a.w - b.w;
  return ((x * x + y * y) + z * z) + w * w;
}
DN_DEV float kernel_h(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

struct tap_sums {
  float W = 0, V = 0, x = 0, y = 0, z = 0;
};
template <bool N, bool A>
DN_DEV void add_tap(tap_sums& s, const pass_args& a, float hh, float r, float lp, float4 np, float4 ap, float lq, float4 cq, float vq,
    float4 nq, float4 aq) {
  float x = fabsf(lp - lq) * r;
  if (N) x = x + d2(np, nq) * a.r_normal;
  if (A) x = x + d2(ap, aq) * a.r_albedo;
  const float u = fmaxf(1.0f - x / 4.0f, 0.0f);
  const float w = hh * ((u * u) * (u * u));
  s.W = s.W + w;
  s.x = s.x + w * cq.x, s.y = s.y + w * cq.y, s.z = s.z + w * cq.z;
  s.V = s.V + (w * w) * vq;
}
DN_DEV void store_pixel(const pass_args& a, size_t p, const tap_sums& s, float alpha) {
  a.c_out[p] = make_float4(s.x / s.W, s.y / s.W, s.z / s.W, alpha);
  if (a.v_out) a.v_out[p] = s.V / (s.W * s.W);
}

// ---- plain form -------------------------------------------------------------------------------------------------------------
template <bool N, bool A>
__global__ void __launch_bounds__(k_block) vpt_denoise_plain_kernel(pass_args a, int stride) {
  const int px = blockIdx.x * 64 + (threadIdx.x & 63), py = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (px >= a.width || py >= a.height) return;
  const size_t p  = (size_t)py * a.width + px;
  const float4 cp = a.c_in[p];
  const float4 np = N ? a.normal[p] : make_float4(0, 0, 0, 0), ap = A ? a.albedo[p] : make_float4(0, 0, 0, 0);
  const float  lp = lum(cp), r = 1.0f / (a.sigma_l * sqrtf(a.v_in[p]) + 1e-4f);
  tap_sums s;
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = py + stride * dy;
    if (qy < 0 || qy >= a.height) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = px + stride * dx;
      if (qx < 0 || qx >= a.width) continue;
      const size_t q  = (size_t)qy * a.width + qx;
      const float4 cq = a.c_in[q];
      add_tap<N, A>(s, a, kernel_h(dy) * kernel_h(dx), r, lp, np, ap, lum(cq), cq, a.v_in[q], N ? a.normal[q] : np, A ? a.albedo[q] : ap);
    }
  }
  store_pixel(a, p, s, cp.w);
}

// ---- tiled form -------------------------------------------------------------------------------------------------------------
template <int S, bool N, bool A>
__global__ void __launch_bounds__(k_block) vpt_denoise_tiled_kernel(pass_args a) {
  constexpr int P = k_tile_w + 4 * S, R = k_tile_h + 4 * S;   // the tile with its halo
  __shared__ float4 s_c[R * P];
  __shared__ float4 s_n[N ? R * P : 1];
  __shared__ float4 s_a[A ? R * P : 1];
  __shared__ float  s_v[R * P];
  __shared__ float  s_l[R * P];
  const int x0 = blockIdx.x * k_tile_w - 2 * S, y0 = blockIdx.y * k_tile_h - 2 * S;   // image position of entry (0, 0)
  for (int i = threadIdx.x; i < R * P; i += k_block) {
    const int    r = i / P, c = i - r * P, gx = x0 + c, gy = y0 + r;
    const bool   in = gx >= 0 && gx < a.width && gy >= 0 && gy < a.height;   // entries outside the image are never used as taps
    const size_t g  = in ? (size_t)gy * a.width + gx : 0;
    const float4 cq = in ? a.c_in[g] : make_float4(0, 0, 0, 0);
    s_c[i] = cq, s_l[i] = lum(cq), s_v[i] = in ? a.v_in[g] : 0.0f;
    if (N) s_n[i] = in ? a.normal[g] : make_float4(0, 0, 0, 0);
    if (A) s_a[i] = in ? a.albedo[g] : make_float4(0, 0, 0, 0);
  }
  __syncthreads();
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int px = blockIdx.x * k_tile_w + tx;
  if (px >= a.width) return;
#pragma unroll
  for (int half = 0; half < 2; half++) {
    const int row = ty + 4 * half, py = blockIdx.y * k_tile_h + row;
    if (py >= a.height) break;
    const int    i  = (row + 2 * S) * P + tx + 2 * S;
    const float4 cp = s_c[i];
    const float4 np = N ? s_n[i] : make_float4(0, 0, 0, 0), ap = A ? s_a[i] : make_float4(0, 0, 0, 0);
    const float  lp = s_l[i], r = 1.0f / (a.sigma_l * sqrtf(s_v[i]) + 1e-4f);
    tap_sums s;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
      const int qy = py + S * dy;
      if (qy < 0 || qy >= a.height) continue;
#pragma unroll
      for (int dx = -2; dx <= 2; dx++) {
        const int qx = px + S * dx;
        if (qx < 0 || qx >= a.width) continue;
        const int q = i + (S * dy) * P + S * dx;
        add_tap<N, A>(s, a, kernel_h(dy) * kernel_h(dx), r, lp, np, ap, s_l[q], s_c[q], s_v[q], N ? s_n[q] : np, A ? s_a[q] : ap);
      }
    }
    store_pixel(a, (size_t)py * a.width + px, s, cp.w);
  }
}

// ---- variance seeds ---------------------------------------------------------------------------------------------------------
// spatial seed: max(0, box3(lum^2) - box3(lum)^2) of the colour
__global__ void __launch_bounds__(k_block) vpt_denoise_seed_kernel(const float4* __restrict__ color, float* __restrict__ variance, int width,
    int height) {
  const int px = blockIdx.x * 64 + (threadIdx.x & 63), py = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (px >= width || py >= height) return;
  float sum = 0, sum2 = 0, count = 0;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++) {
    const int qy = py + dy;
    if (qy < 0 || qy >= height) continue;
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      const int qx = px + dx;
      if (qx < 0 || qx >= width) continue;
      const float l = lum(color[(size_t)qy * width + qx]);
      sum = sum + l, sum2 = sum2 + l * l, count = count + 1.0f;
    }
  }
  const float m = sum / count, m2 = sum2 / count;
  variance[(size_t)py * width + px] = fmaxf(0.0f, m2 - m * m);
}

// half variance: box3(g * g), g = (lum(S_a / a) - lum((S_n - S_a) / (n - a))) / 2
__global__ void __launch_bounds__(k_block) vpt_half_variance_kernel(const float4* __restrict__ sum_a, float fa, const float4* __restrict__ sum_n,
    float fb, float* __restrict__ variance, int width, int height) {
  const int px = blockIdx.x * 64 + (threadIdx.x & 63), py = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (px >= width || py >= height) return;
  float sum = 0, count = 0;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++) {
    const int qy = py + dy;
    if (qy < 0 || qy >= height) continue;
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      const int qx = px + dx;
      if (qx < 0 || qx >= width) continue;
      const float4 sa = sum_a[(size_t)qy * width + qx], sn = sum_n[(size_t)qy * width + qx];
      const float4 A  = make_float4(sa.x / fa, sa.y / fa, sa.z / fa, 0);
      const float4 B  = make_float4((sn.x - sa.x) / fb, (sn.y - sa.y) / fb, (sn.z - sa.z) / fb, 0);
      const float  g  = (lum(A) - lum(B)) / 2.0f;
      sum = sum + g * g, count = count + 1.0f;
    }
  }
  variance[(size_t)py * width + px] = sum / count;
}

template <bool N, bool A>
void launch_pass(const pass_args& a, int stride, bool tiled, hipStream_t st) {
  const dim3 plain_grid((a.width + 63) / 64, (a.height + 3) / 4), tile_grid((a.width + k_tile_w - 1) / k_tile_w, (a.height + k_tile_h - 1) / k_tile_h);
  if (tiled && stride == 1) hipLaunchKernelGGL((vpt_denoise_tiled_kernel<1, N, A>), tile_grid, dim3(k_block), 0, st, a);
  else if (tiled && stride == 2) hipLaunchKernelGGL((vpt_denoise_tiled_kernel<2, N, A>), tile_grid, dim3(k_block), 0, st, a);
  else hipLaunchKernelGGL((vpt_denoise_plain_kernel<N, A>), plain_grid, dim3(k_block), 0, st, a, stride);
}

constexpr long long k_max_pixels = 1LL << 28;   // 4 GiB of float4: far past any frame, and every index fits

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

int check_size(int width, int height) {
  REQUIRE(width >= 1 && height >= 1, "bad image size: width %d, height %d", width, height);
  REQUIRE((long long)width * height <= k_max_pixels, "image too large: width %d, height %d", width, height);
  return VPT_OK;
}
int check_params(const vpt_denoise_params* p) {
  REQUIRE(p, "null params");
  REQUIRE(p->iterations >= 1 && p->iterations <= 8, "iterations %d outside 1..8", p->iterations);
  REQUIRE(std::isfinite(p->sigma_luminance) && p->sigma_luminance > 0, "sigma_luminance must be finite and > 0");
  REQUIRE(std::isfinite(p->sigma_normal) && p->sigma_normal > 0, "sigma_normal must be finite and > 0");
  REQUIRE(std::isfinite(p->sigma_albedo) && p->sigma_albedo > 0, "sigma_albedo must be finite and > 0");
  return VPT_OK;
}
}  // namespace

extern "C" {

int64_t vpt_denoise_scratch_bytes(int width, int height) {
  if (check_size(width, height) != VPT_OK) return -1;
  return (int64_t)width * height * (2 * 16 + 2 * 4);   // two colour and two variance buffers
}

int vpt_denoise_device(const vpt_denoise_params* params, int width, int height, const void* d_color, const void* d_normal, const void* d_albedo,
    const void* d_variance, void* d_out, void* d_scratch, void* stream) {
  if (int rc = check_params(params)) return rc;
  if (int rc = check_size(width, height)) return rc;
  REQUIRE(d_color, "null color");
  REQUIRE(d_out, "null out");
  REQUIRE(d_scratch, "null scratch");
  const size_t n = (size_t)width * height, scratch_bytes = n * 40;
  const struct { const void* p; size_t bytes; const char* name; } inputs[] = {{d_color, n * 16, "color"}, {d_normal, n * 16, "normal"},
      {d_albedo, n * 16, "albedo"}, {d_variance, n * 4, "variance"}};
  for (auto& in : inputs) {
    REQUIRE(!overlap(d_out, n * 16, in.p, in.bytes), "out aliases %s", in.name);
    REQUIRE(!overlap(d_scratch, scratch_bytes, in.p, in.bytes), "scratch aliases %s", in.name);
  }
  REQUIRE(!overlap(d_out, n * 16, d_scratch, scratch_bytes), "out aliases scratch");
  const hipStream_t st = (hipStream_t)stream;
  float4* cbuf[2] = {(float4*)d_scratch, (float4*)d_scratch + n};
  float*  vbuf[2] = {(float*)(cbuf[1] + n), (float*)(cbuf[1] + n) + n};
  const dim3 grid((width + 63) / 64, (height + 3) / 4);
  if (!d_variance) {   // pass 0 writes vbuf[0], so the seed goes to vbuf[1]
    hipLaunchKernelGGL(vpt_denoise_seed_kernel, grid, dim3(k_block), 0, st, (const float4*)d_color, vbuf[1], width, height);
    HIP_TRY(hipGetLastError());
  }
  const char* env   = getenv("VPT_DENOISE_PLAIN");
  const bool  plain = env && atoi(env) != 0;
  pass_args a = {};
  a.normal = (const float4*)d_normal, a.albedo = (const float4*)d_albedo, a.width = width, a.height = height;
  a.sigma_l = params->sigma_luminance, a.r_normal = 1.0f / (params->sigma_normal * params->sigma_normal);
  a.r_albedo = 1.0f / (params->sigma_albedo * params->sigma_albedo);
  for (int k = 0; k < params->iterations; k++) {
    const bool last = k == params->iterations - 1;
    a.c_in  = k == 0 ? (const float4*)d_color : cbuf[(k - 1) & 1];
    a.v_in  = k == 0 ? (d_variance ? (const float*)d_variance : vbuf[1]) : vbuf[(k - 1) & 1];
    a.c_out = last ? (float4*)d_out : cbuf[k & 1];
    a.v_out = last ? nullptr : vbuf[k & 1];
    const int  stride = 1 << k;
    const bool tiled  = !plain && stride <= k_max_tiled_stride;
    if (d_normal && d_albedo) launch_pass<true, true>(a, stride, tiled, st);
    else if (d_normal) launch_pass<true, false>(a, stride, tiled, st);
    else if (d_albedo) launch_pass<false, true>(a, stride, tiled, st);
    else launch_pass<false, false>(a, stride, tiled, st);
    HIP_TRY(hipGetLastError());
  }
  return VPT_OK;
}

int vpt_half_variance_device(int width, int height, const void* d_sum_a, int a, const void* d_sum_n, int n, void* d_variance, void* stream) {
  if (int rc = check_size(width, height)) return rc;
  REQUIRE(d_sum_a, "null sum_a");
  REQUIRE(d_sum_n, "null sum_n");
  REQUIRE(d_variance, "null variance");
  REQUIRE(a > 0 && a < n, "sample counts must satisfy 0 < a < n (a %d, n %d)", a, n);
  const size_t px = (size_t)width * height;
  REQUIRE(!overlap(d_variance, px * 4, d_sum_a, px * 16), "variance aliases sum_a");
  REQUIRE(!overlap(d_variance, px * 4, d_sum_n, px * 16), "variance aliases sum_n");
  hipLaunchKernelGGL(vpt_half_variance_kernel, dim3((width + 63) / 64, (height + 3) / 4), dim3(k_block), 0, (hipStream_t)stream,
      (const float4*)d_sum_a, (float)a, (const float4*)d_sum_n, (float)(n - a), (float*)d_variance, width, height);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

int vpt_half_variance(int device, int width, int height, const float* sum_a, int a, const float* sum_n, int n, float* variance) {
  if (int rc = check_size(width, height)) return rc;
  REQUIRE(sum_a, "null sum_a");
  REQUIRE(sum_n, "null sum_n");
  REQUIRE(variance, "null variance");
  REQUIRE(a > 0 && a < n, "sample counts must satisfy 0 < a < n (a %d, n %d)", a, n);
  const int ndev = vpt_device_count();
  if (ndev <= 0 || device < 0) return vpt_set_error(VPT_ERR_NO_DEVICE, "no HIP device %d available (this library has no CPU fallback)", device);
  REQUIRE(device < ndev, "device %d out of range (%d devices)", device, ndev);
  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(device));
  const size_t  px = (size_t)width * height;
  device_buffer d_a, d_n, d_v;
  if (int rc = d_a.allocate(px * 16)) return rc;
  if (int rc = d_n.allocate(px * 16)) return rc;
  if (int rc = d_v.allocate(px * 4)) return rc;
  HIP_TRY(hipMemcpy(d_a.get(), sum_a, px * 16, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_n.get(), sum_n, px * 16, hipMemcpyHostToDevice));
  if (int rc = vpt_half_variance_device(width, height, d_a.get(), a, d_n.get(), n, d_v.get(), nullptr)) return rc;
  HIP_TRY(hipMemcpy(variance, d_v.get(), px * 4, hipMemcpyDeviceToHost));
  return VPT_OK;
}

int vpt_denoise(const vpt_denoise_params* params, int device, int width, int height, const float* color, const float* normal, const float* albedo,
    const float* variance, float* out) {
  if (int rc = check_params(params)) return rc;
  if (int rc = check_size(width, height)) return rc;
  REQUIRE(color, "null color");
  REQUIRE(out, "null out");
  const size_t n = (size_t)width * height;
  const struct { const void* p; size_t bytes; const char* name; } inputs[] = {{color, n * 16, "color"}, {normal, n * 16, "normal"},
      {albedo, n * 16, "albedo"}, {variance, n * 4, "variance"}};
  for (auto& in : inputs) REQUIRE(!overlap(out, n * 16, in.p, in.bytes), "out aliases %s", in.name);
  const int ndev = vpt_device_count();
  if (ndev <= 0 || device < 0) return vpt_set_error(VPT_ERR_NO_DEVICE, "no HIP device %d available (this library has no CPU fallback)", device);
  REQUIRE(device < ndev, "device %d out of range (%d devices)", device, ndev);
  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(device));
  device_buffer d_color, d_normal, d_albedo, d_variance, d_out, d_scratch;
  if (int rc = d_color.allocate(n * 16)) return rc;
  if (int rc = d_out.allocate(n * 16)) return rc;
  if (int rc = d_scratch.allocate(n * 40)) return rc;
  HIP_TRY(hipMemcpy(d_color.get(), color, n * 16, hipMemcpyHostToDevice));
  if (normal) {
    if (int rc = d_normal.allocate(n * 16)) return rc;
    HIP_TRY(hipMemcpy(d_normal.get(), normal, n * 16, hipMemcpyHostToDevice));
  }
  if (albedo) {
    if (int rc = d_albedo.allocate(n * 16)) return rc;
    HIP_TRY(hipMemcpy(d_albedo.get(), albedo, n * 16, hipMemcpyHostToDevice));
  }
  if (variance) {
    if (int rc = d_variance.allocate(n * 4)) return rc;
    HIP_TRY(hipMemcpy(d_variance.get(), variance, n * 4, hipMemcpyHostToDevice));
  }
  if (int rc = vpt_denoise_device(params, width, height, d_color.get(), d_normal.get(), d_albedo.get(), d_variance.get(), d_out.get(),
          d_scratch.get(), nullptr))
    return rc;
  HIP_TRY(hipMemcpy(out, d_out.get(), n * 16, hipMemcpyDeviceToHost));   // on the null stream: waits for the passes
  return VPT_OK;
}

}  // extern "C"
