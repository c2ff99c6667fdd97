// vpt_frame_stages.hip — the device stages a frame loop needs beside the render kernels (include/vpt.h): make_state on
// the device, the reference's tone mapping, the preview's replication, the pack of a mesh pick; their launchers and their C-ABI, and
// vpt_tonemap on host arrays.  The session that strings them together is csrc/vpt_session.hip.
// The arithmetic of the tone map is the rule include/vpt.h states, operation for operation (-ffp-contract=off; float32 / is correctly
// rounded), so without the sRGB curve the host mirror (host/vpt_display.cpp) gives the same bits; the curve is vpt_srgb.hip.h's.
#include "vpt_frame_stages.h"

#include <cmath>
#include <cstdint>

#include "vpt_device_buffer.h"
#include "vpt_error.h"
#include "vpt_kernels.hip.h"   // slot_to_pixel
#include "vpt_layout.h"
#include "vpt_rng_jump.h"
#include "vpt_srgb.hip.h"

namespace {

constexpr int       k_block      = 256;
constexpr long long k_max_pixels = 1LL << 28;   // as vpt_denoise: every index fits

// ---- make_state on the device -------------------------------------------------------------------------------------------------
// 64 consecutive slots are one 8x8 block of pixels (slot_to_pixel): lane q holds pixel (x0 + (q & 7), y0 + (q >> 3)), whose row-major
// index is idx0 + (q >> 3) * width + (q & 7).  The wave jumps the master stream to idx0 (scalar: at most 64 rounds of two 64-bit
// products, 30 for a frame below 2^30 pixels), a lane adds its own offset with one step of the LCG (A^k, c_k) from `tab`, a kernel argument.
struct jump_table {
  vpt_lcg_jump e[64];
};

__global__ void __launch_bounds__(k_block) vpt_state_init_kernel(DParams pr, jump_table tab, unsigned long long master_state,
    unsigned long long master_inc, float4* __restrict__ image, int* __restrict__ hits, ulonglong2* __restrict__ rngs) {
  const int slot = blockIdx.x * k_block + threadIdx.x;
  if (slot >= pr.nslots) return;   // nslots is a multiple of 64: whole waves leave
  const int first = __builtin_amdgcn_readfirstlane(slot & ~63);
  int       x0 = 0, y0 = 0, px, py;
  (void)slot_to_pixel(pr, first, x0, y0);   // a block outside the frame keeps (0, 0): none of its lanes owns a pixel
  const unsigned long long idx0 = (unsigned long long)y0 * (unsigned long long)pr.width + (unsigned long long)x0;
  const vpt_lcg_jump       j    = vpt_pcg32_jump(master_inc, idx0);
  const unsigned long long s0   = j.mul * master_state + j.add;
  if (!slot_to_pixel(pr, slot, px, py)) return;   // padding, or another rank's
  const vpt_lcg_jump k = tab.e[slot & 63];
  const vpt_pcg32    r = vpt_state_pixel_rng(k.mul * s0 + k.add);
  if (image) image[slot] = make_float4(0, 0, 0, 0);   // (null: the state of a first-hit pass, which has planes instead)
  hits[slot] = 0, rngs[slot] = make_ulonglong2(r.state, r.inc);
}

// the 24 bytes of a pick: {hit, instance, element} and {u, v, distance} of one pixel of the row-major id frame
__global__ void vpt_pick_kernel(const int2* __restrict__ ids, const float* __restrict__ uvt, long long pixel, int* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int2 id = ids[pixel];
  out[0] = id.x >= 0 ? 1 : 0, out[1] = id.x, out[2] = id.y;
  for (int c = 0; c < 3; c++) out[3 + c] = __float_as_int(uvt[3 * pixel + c]);
}

// ---- tonemap(vec4f, exposure, filmic, srgb), yocto_color.h:306-316 --------------------------------------------------------------
__device__ __forceinline__ float filmic_curve(float c) {   // tonemap_filmic without accurate_fit, :274-280
  const float h   = c * 0.6f;
  const float ldr = ((h * h) * 2.51f + h * 0.03f) / (((h * h) * 2.43f + h * 0.59f) + 0.14f);
  return (0 < ldr) ? ldr : 0.0f;
}
__global__ void __launch_bounds__(k_block) vpt_tonemap_kernel(const float4* __restrict__ linear, float4* __restrict__ display_f,
    uchar4* __restrict__ rgba8, long long n, float scale, int scaled, int filmic, int srgb) {
  const long long i = (long long)blockIdx.x * k_block + threadIdx.x;
  if (i >= n) return;
  float4 c = linear[i];
  if (scaled) c.x = c.x * scale, c.y = c.y * scale, c.z = c.z * scale;
  if (filmic) c.x = filmic_curve(c.x), c.y = filmic_curve(c.y), c.z = filmic_curve(c.z);
  if (srgb) c.x = srgb_curve(c.x), c.y = srgb_curve(c.y), c.z = srgb_curve(c.z);
  if (display_f) display_f[i] = c;
  if (rgba8) rgba8[i] = make_uchar4(srgb_quant(c.x), srgb_quant(c.y), srgb_quant(c.z), srgb_quant(c.w));
}

// ---- the preview replicated to full size, apps/ypathtrace/ypathtrace.cpp:164-169 -----------------------------------------------
__global__ void __launch_bounds__(k_block) vpt_upscale_kernel(const float4* __restrict__ preview, int pw, int ph, int pratio,
    float4* __restrict__ out, int width, int height) {
  const int i = blockIdx.x * 64 + (threadIdx.x & 63), j = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (i >= width || j >= height) return;
  const int pi = min(i / pratio, pw - 1), pj = min(j / pratio, ph - 1);
  out[(size_t)j * width + i] = preview[(size_t)pj * pw + pi];
}

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
int check_tonemap(const vpt_display_params* d, int width, int height, const void* linear, const void* display_f, const void* rgba8) {
  if (int rc = check_display(d)) return rc;
  if (int rc = check_size(width, height)) return rc;
  REQUIRE(linear, "null linear");
  REQUIRE(display_f || rgba8, "null display_f and rgba8: nothing to write");
  const size_t n = (size_t)width * height;
  REQUIRE(!overlap(display_f, n * 16, linear, n * 16), "display_f aliases linear");
  REQUIRE(!overlap(rgba8, n * 4, linear, n * 16), "rgba8 aliases linear");
  REQUIRE(!overlap(rgba8, n * 4, display_f, n * 16), "rgba8 aliases display_f");
  return VPT_OK;
}

}  // namespace

int check_display(const vpt_display_params* d) {
  REQUIRE(d, "null display params");
  REQUIRE(std::isfinite(d->exposure), "exposure must be finite");
  REQUIRE((d->filmic == 0 || d->filmic == 1) && (d->srgb == 0 || d->srgb == 1), "filmic and srgb must be 0 or 1");
  return VPT_OK;
}

int state_init(const vpt_layout* layout, void* d_image, void* d_hits, void* d_rng, void* stream) {
  DParams pr;
  if (int rc = vpt_layout_dparams(layout, pr)) return rc;
  jump_table      tab;
  const vpt_pcg32 master = vpt_pcg32_make(VPT_STATE_MASTER_SEED, 1);
  for (int q = 0; q < 64; q++) tab.e[q] = vpt_pcg32_jump(master.inc, (uint64_t)(q >> 3) * (uint64_t)pr.width + (uint64_t)(q & 7));
  hipLaunchKernelGGL(vpt_state_init_kernel, dim3((pr.nslots + k_block - 1) / k_block), dim3(k_block), 0, (hipStream_t)stream, pr, tab,
      (unsigned long long)master.state, (unsigned long long)master.inc, (float4*)d_image, (int*)d_hits, (ulonglong2*)d_rng);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

int vpt_pick_device(const vpt_scene*, const void* d_ids_rowmajor, const void* d_uvt_rowmajor, long long pixel, void* d_out24, void* stream) {
  hipLaunchKernelGGL(vpt_pick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const int2*)d_ids_rowmajor, (const float*)d_uvt_rowmajor, pixel,
      (int*)d_out24);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

extern "C" {

int vpt_state_init_device(const vpt_layout* layout, void* d_image, void* d_hits, void* d_rng, void* stream) {
  REQUIRE(layout && d_image && d_hits && d_rng, "null argument");
  return state_init(layout, d_image, d_hits, d_rng, stream);
}

int vpt_tonemap_device(const vpt_display_params* display, int width, int height, const void* d_linear, void* d_display_f, void* d_rgba8,
    void* stream) {
  if (int rc = check_tonemap(display, width, height, d_linear, d_display_f, d_rgba8)) return rc;
  const long long n = (long long)width * height;
  hipLaunchKernelGGL(vpt_tonemap_kernel, dim3((unsigned)((n + k_block - 1) / k_block)), dim3(k_block), 0, (hipStream_t)stream,
      (const float4*)d_linear, (float4*)d_display_f, (uchar4*)d_rgba8, n, exp2f(display->exposure), display->exposure != 0 ? 1 : 0,
      display->filmic, display->srgb);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

int vpt_upscale_device(int pratio, int pw, int ph, const void* d_preview, int width, int height, void* d_out, void* stream) {
  REQUIRE(pratio >= 1, "pratio %d must be >= 1", pratio);
  if (int rc = check_size(pw, ph)) return rc;
  if (int rc = check_size(width, height)) return rc;
  REQUIRE(d_preview, "null preview");
  REQUIRE(d_out, "null out");
  REQUIRE(!overlap(d_out, (size_t)width * height * 16, d_preview, (size_t)pw * ph * 16), "out aliases preview");
  hipLaunchKernelGGL(vpt_upscale_kernel, dim3((width + 63) / 64, (height + 3) / 4), dim3(k_block), 0, (hipStream_t)stream,
      (const float4*)d_preview, pw, ph, pratio, (float4*)d_out, width, height);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

int vpt_tonemap(const vpt_display_params* display, int device, int width, int height, const float* linear, float* display_f, uint8_t* rgba8) {
  if (int rc = check_tonemap(display, width, height, linear, display_f, rgba8)) return rc;
  const int ndev = vpt_device_count();
  if (ndev <= 0 || device < 0) return vpt_set_error(VPT_ERR_NO_DEVICE, "no HIP device %d available (this library has no CPU fallback)", device);
  REQUIRE(device < ndev, "device %d out of range (%d devices)", device, ndev);
  (void)hipGetLastError();
  HIP_TRY(hipSetDevice(device));
  const size_t  n = (size_t)width * height;
  device_buffer d_linear, d_display, d_bytes;
  if (int rc = d_linear.allocate(n * 16)) return rc;
  if (display_f)
    if (int rc = d_display.allocate(n * 16)) return rc;
  if (rgba8)
    if (int rc = d_bytes.allocate(n * 4)) return rc;
  HIP_TRY(hipMemcpy(d_linear.get(), linear, n * 16, hipMemcpyHostToDevice));
  if (int rc = vpt_tonemap_device(display, width, height, d_linear.get(), d_display.get(), d_bytes.get(), nullptr)) return rc;
  if (display_f) HIP_TRY(hipMemcpy(display_f, d_display.get(), n * 16, hipMemcpyDeviceToHost));   // on the null stream: waits for the kernel
  if (rgba8) HIP_TRY(hipMemcpy(rgba8, d_bytes.get(), n * 4, hipMemcpyDeviceToHost));
  return VPT_OK;
}

}  // extern "C"
