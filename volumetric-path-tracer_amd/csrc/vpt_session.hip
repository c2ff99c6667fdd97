// vpt_session.hip — progressive rendering on one GPU (include/vpt.h: vpt_session): the three device stages a frame
// loop needs beside the render kernels - make_state on the device, the reference's tone mapping, the preview's replication - and the
// session that strings them together with vpt_render_device, vpt_resolve_device and vpt_denoise_device over buffers that stay in HBM.
// The session is plain host code over the C-ABI: it sees a scene through its public calls only.
// The arithmetic of the tone map is the rule include/vpt.h states, operation for operation (-ffp-contract=off; float32 / is correctly
// rounded), so without the sRGB curve the host mirror (host/vpt_display.cpp) gives the same bits; the curve is vpt_srgb.hip.h's.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "vpt_device_buffer.h"
#include "vpt_error.h"
#include "vpt_kernels.hip.h"   // slot_to_pixel
#include "vpt_layout.h"
#include "vpt_rng_jump.h"
#include "vpt_sdf_aov.h"   // vpt_sdf_pick_device
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
int check_display(const vpt_display_params* d) {
  REQUIRE(d, "null display params");
  REQUIRE(std::isfinite(d->exposure), "exposure must be finite");
  REQUIRE((d->filmic == 0 || d->filmic == 1) && (d->srgb == 0 || d->srgb == 1), "filmic and srgb must be 0 or 1");
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

// vpt_state_init_device; d_image may be null here (hits and rng alone: the state a first-hit pass runs over)
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

}  // namespace

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

// ---- the session --------------------------------------------------------------------------------------------------------------
struct vpt_session {
  vpt_scene*         scene  = nullptr;
  int                device = 0;
  hipStream_t        st     = nullptr;
  vpt_session_params p      = {};
  int                width = 0, height = 0, pw = 0, ph = 0;   // the frame and its preview
  int                samples = 0;
  vpt_layout         lay = {}, play = {};
  device_buffer      s_image, s_hits, s_rng;            // the pathtrace_state, tile-major (the guides are rendered in it first)
  device_buffer      p_image, p_hits, p_rng, p_rows;    // the preview's state and its get_render
  device_buffer      image, display_f, rgba8;           // row-major: linear image, the two displays
  device_buffer      r_image, r_hits, r_rng;            // row-major staging of get_state, allocated when first asked for
  long long          r_pixels = 0;
  // denoise = 1
  device_buffer normal, albedo, variance, sum_a, sum_n, filtered, scratch;
  device_buffer g_albedo;   // tile-major sums of the albedo guide (the normal guide's are rendered in s_image)
  bool          denoise_allocated = false, has_albedo = false, filtered_valid = false;
  int           a = 0;   // samples behind sum_a (0: none)
  // adaptive mode (vpt_session_set_adaptive): the run lives from the first advance after a reset to the next reset
  bool              adaptive = false;
  vpt_adaptive      ad       = {};
  vpt_adaptive_run* run      = nullptr;
  device_buffer     a_se2, a_var, a_hits, a_mean, a_m2;   // row-major planes of the run's statistics
  long long         a_pixels = 0;
  // the id frame behind pick and get_ids: made on first use after a reset, kept until the next one (every edit resets)
  device_buffer            i_hits, i_rng, i_ids, i_uvt;   // the state and the planes of its one-sample pass, tile-major
  device_buffer            ids, uvt, pick;                // row-major; the 24 bytes of a pick
  long long                i_pixels = 0, i_slots = 0;     // what they were allocated for (0: nothing)
  bool                     ids_valid = false;
  std::vector<vpt_instance> instances;                    // the scene's instance table as of the id frame: a pick's shape and material
  // the id frame of an implicit session (pick_sdf, get_sdf_ids): the same life, the planes of vpt_render_sdf_aov_device
  device_buffer q_hits, q_rng, q_ids, q_hit;              // the state and the planes of its one-sample pass, tile-major
  device_buffer sdf_ids, sdf_hit, sdf_pick;               // row-major; the 48 bytes of a pick
  long long     q_pixels = 0, q_slots = 0;                // what they were allocated for (0: nothing)
  bool          sdf_ids_valid = false;
  // what the last call cost
  int     launches = 0;
  int64_t up = 0, down = 0;
};

namespace {

bool implicit_shader(int shader) { return shader == VPT_SHADER_IMPLICIT || shader == VPT_SHADER_IMPLICIT_NORMAL; }

// make_state's size rule (yocto_pathtrace.cpp:964-970)
void frame_size(int resolution, float aspect, int& width, int& height) {
  if (aspect >= 1) width = resolution, height = (int)std::round(resolution / aspect);
  else height = resolution, width = (int)std::round(resolution * aspect);
}

int check_session_params(const vpt_session_params* p) {
  REQUIRE(p, "null session params");
  if (p->render.shader < 0 || p->render.shader > VPT_SHADER_IMPLICIT_NORMAL) return vpt_set_error(VPT_ERR_UNKNOWN_SHADER, "sampler unknown");
  REQUIRE(p->render.resolution >= 1 && p->render.resolution < 32768, "resolution %d outside 1..32767", p->render.resolution);
  REQUIRE(p->render.samples >= 1, "samples %d must be >= 1", p->render.samples);
  REQUIRE(p->render.bounces >= 0, "negative bounce count");
  REQUIRE(p->pratio >= 1 && p->pratio <= 64, "pratio %d outside 1..64", p->pratio);
  REQUIRE(p->render.resolution / p->pratio >= 1, "pratio %d leaves no preview of resolution %d", p->pratio, p->render.resolution);
  if (int rc = check_display(&p->display)) return rc;
  REQUIRE(p->denoise == 0 || p->denoise == 1, "denoise must be 0 or 1");
  if (p->denoise) {
    const vpt_denoise_params& f = p->filter;
    REQUIRE(f.iterations >= 1 && f.iterations <= 8, "iterations %d outside 1..8", f.iterations);
    REQUIRE(std::isfinite(f.sigma_luminance) && f.sigma_luminance > 0, "sigma_luminance must be finite and > 0");
    REQUIRE(std::isfinite(f.sigma_normal) && f.sigma_normal > 0, "sigma_normal must be finite and > 0");
    REQUIRE(std::isfinite(f.sigma_albedo) && f.sigma_albedo > 0, "sigma_albedo must be finite and > 0");
    REQUIRE(p->guide_samples >= 1, "guide_samples %d must be >= 1", p->guide_samples);
  }
  return VPT_OK;
}

void begin_call(vpt_session* s) { s->launches = 0, s->up = 0, s->down = 0; }

void drop_run(vpt_session* s) {
  if (s->run) vpt_adaptive_run_destroy(s->run);
  s->run = nullptr;
}
// vpt_session_set_adaptive's conditions, against the per-pixel cap `samples`
int check_session_adaptive(const vpt_adaptive* a, int samples) {
  REQUIRE(std::isfinite(a->threshold) && a->threshold >= 0, "adaptive threshold must be finite and >= 0");
  REQUIRE(a->step >= 1, "adaptive step must be >= 1");
  REQUIRE(a->min_samples >= 1 && a->min_samples <= samples, "adaptive min_samples must be in 1 .. render.samples (%d)", samples);
  return VPT_OK;
}

int allocate(vpt_session* s, int width, int height, int pw, int ph, bool denoise) {
  s->width = s->height = 0, s->denoise_allocated = false, s->r_pixels = 0, s->i_pixels = s->i_slots = 0, s->q_pixels = s->q_slots = 0;   // a new frame: the lazily made buffers go with the old one
  const vpt_layout lay = {width, height, 8, 8, 0, 1}, play = {pw, ph, 8, 8, 0, 1};
  const long long  slots = vpt_layout_slots(&lay), pslots = vpt_layout_slots(&play);
  if (slots < 0 || pslots < 0) return VPT_ERR_INVALID_ARG;
  const size_t n = (size_t)width * height;
  using sized = std::pair<device_buffer*, size_t>;
  const sized frame[] = {{&s->s_image, (size_t)slots * 16}, {&s->s_hits, (size_t)slots * 4}, {&s->s_rng, (size_t)slots * 16},
      {&s->p_image, (size_t)pslots * 16}, {&s->p_hits, (size_t)pslots * 4}, {&s->p_rng, (size_t)pslots * 16}, {&s->p_rows, (size_t)pw * ph * 16},
      {&s->image, n * 16}, {&s->display_f, n * 16}, {&s->rgba8, n * 4}};
  for (auto& [b, bytes] : frame)
    if (int rc = b->allocate(bytes)) return rc;
  if (denoise) {
    const sized filter[] = {{&s->normal, n * 16}, {&s->albedo, n * 16}, {&s->variance, n * 4}, {&s->sum_a, n * 16}, {&s->sum_n, n * 16},
        {&s->filtered, n * 16}, {&s->scratch, (size_t)vpt_denoise_scratch_bytes(width, height)}, {&s->g_albedo, (size_t)slots * 16}};
    for (auto& [b, bytes] : filter)
      if (int rc = b->allocate(bytes)) return rc;
  } else {
    for (device_buffer* b : {&s->normal, &s->albedo, &s->variance, &s->sum_a, &s->sum_n, &s->filtered, &s->scratch, &s->g_albedo}) *b = device_buffer();
  }
  s->lay = lay, s->play = play, s->width = width, s->height = height, s->pw = pw, s->ph = ph, s->denoise_allocated = denoise;
  return VPT_OK;
}

// `image` (or the filtered image, where the display shows it) -> both displays
int tonemap_display(vpt_session* s) {
  const void* src = s->filtered_valid ? s->filtered.get() : s->image.get();
  s->launches++;
  return vpt_tonemap_device(&s->p.display, s->width, s->height, src, s->display_f.get(), s->rgba8.get(), s->st);
}

// one guide: `samples` passes of `shader` over a state initialised on the device (in the session's own state buffers), get_render
int render_guide(vpt_session* s, int shader, void* d_out) {
  vpt_params p = s->p.render;
  p.shader = shader, p.samples = s->p.guide_samples;
  if (int rc = vpt_state_init_device(&s->lay, s->s_image.get(), s->s_hits.get(), s->s_rng.get(), s->st)) return rc;
  if (int rc = vpt_render_device(s->scene, &p, &s->lay, p.samples, s->s_image.get(), s->s_hits.get(), s->s_rng.get(), s->st)) return rc;
  s->launches += 3;
  return vpt_resolve_device(&s->lay, s->s_image.get(), p.samples, d_out, s->st);
}

// both guides of the mesh shaders from one first-hit pass (include/vpt.h: vpt_render_aov_device): `normal` and `color` trace the same
// rays from the same streams, so one traversal per sample serves both; the bits are those of two calls of render_guide
int render_mesh_guides(vpt_session* s) {
  vpt_params p = s->p.render;
  p.samples    = s->p.guide_samples;
  if (int rc = vpt_state_init_device(&s->lay, s->s_image.get(), s->s_hits.get(), s->s_rng.get(), s->st)) return rc;   // zeroes s_image
  HIP_TRY(hipMemsetAsync(s->g_albedo.get(), 0, (size_t)vpt_layout_slots(&s->lay) * 16, s->st));
  const vpt_aov_planes planes = {s->s_image.get(), s->g_albedo.get(), nullptr, nullptr, nullptr, nullptr};
  if (int rc = vpt_render_aov_device(s->scene, &p, &s->lay, p.samples, &planes, s->s_hits.get(), s->s_rng.get(), s->st)) return rc;
  if (int rc = vpt_resolve_device(&s->lay, s->s_image.get(), p.samples, s->normal.get(), s->st)) return rc;
  s->launches += 4;
  return vpt_resolve_device(&s->lay, s->g_albedo.get(), p.samples, s->albedo.get(), s->st);
}

// the id frame (include/vpt.h: vpt_session_pick): one sample in the pixel-centre branch at full resolution over a state of its own
int ensure_ids(vpt_session* s) {
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  if (implicit_shader(s->p.render.shader))
    return vpt_set_error(VPT_ERR_UNSUPPORTED, "the session renders an implicit shader: its picture is not what the mesh BVH holds");
  if (s->ids_valid) return VPT_OK;
  HIP_TRY(hipSetDevice(s->device));
  const size_t n = (size_t)s->width * s->height, slots = (size_t)vpt_layout_slots(&s->lay);
  // the state and the planes hold one entry per tile-major SLOT: frames of equal pixel counts can differ in it (105 x 40 and 100 x 42)
  if (s->i_pixels != (long long)n || s->i_slots != (long long)slots) {
    s->i_pixels = s->i_slots = 0;
    using sized = std::pair<device_buffer*, size_t>;
    const sized frame[] = {{&s->i_hits, slots * 4}, {&s->i_rng, slots * 16}, {&s->i_ids, slots * 8}, {&s->i_uvt, slots * 12}, {&s->ids, n * 8},
        {&s->uvt, n * 12}, {&s->pick, 24}};
    for (auto& [b, bytes] : frame)
      if (int rc = b->allocate(bytes)) return rc;
    s->i_pixels = (long long)n, s->i_slots = (long long)slots;
  }
  vpt_params p = s->p.render;
  p.samples    = 1;
  if (int rc = state_init(&s->lay, nullptr, s->i_hits.get(), s->i_rng.get(), s->st)) return rc;
  const vpt_aov_planes planes = {nullptr, nullptr, nullptr, nullptr, s->i_ids.get(), s->i_uvt.get()};
  if (int rc = vpt_render_aov_device(s->scene, &p, &s->lay, 1, &planes, s->i_hits.get(), s->i_rng.get(), s->st)) return rc;
  if (int rc = vpt_resolve_ids_device(&s->lay, s->i_ids.get(), s->i_uvt.get(), s->ids.get(), s->uvt.get(), s->st)) return rc;
  s->launches += 3;
  // a pick's shape and material are those of the instance table as it stands now: read once per id frame
  int count = 0;
  if (int rc = vpt_scene_get_instances(s->scene, nullptr, 0, &count)) return rc;
  s->instances.resize((size_t)count);
  if (int rc = vpt_scene_get_instances(s->scene, s->instances.data(), count, nullptr)) return rc;
  s->down += (int64_t)count * (int64_t)sizeof(vpt_instance);
  s->ids_valid = true;
  return VPT_OK;
}

// the id frame of an implicit session (include/vpt.h: vpt_session_pick_sdf): one sample of the sphere-traced first-hit pass in the
// pixel-centre branch at full resolution over a state of its own
int ensure_sdf_ids(vpt_session* s) {
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  if (!implicit_shader(s->p.render.shader))
    return vpt_set_error(VPT_ERR_UNSUPPORTED, "the session renders a mesh shader: use vpt_session_pick / vpt_session_get_ids");
  if (s->sdf_ids_valid) return VPT_OK;
  HIP_TRY(hipSetDevice(s->device));
  const size_t n = (size_t)s->width * s->height, slots = (size_t)vpt_layout_slots(&s->lay);
  if (s->q_pixels != (long long)n || s->q_slots != (long long)slots) {   // one entry per tile-major SLOT, as ensure_ids
    s->q_pixels = s->q_slots = 0;
    using sized = std::pair<device_buffer*, size_t>;
    const sized frame[] = {{&s->q_hits, slots * 4}, {&s->q_rng, slots * 16}, {&s->q_ids, slots * 8}, {&s->q_hit, slots * 16}, {&s->sdf_ids, n * 8},
        {&s->sdf_hit, n * 16}, {&s->sdf_pick, sizeof(vpt_sdf_pick)}};
    for (auto& [b, bytes] : frame)
      if (int rc = b->allocate(bytes)) return rc;
    s->q_pixels = (long long)n, s->q_slots = (long long)slots;
  }
  vpt_params p = s->p.render;
  p.samples    = 1;
  if (int rc = state_init(&s->lay, nullptr, s->q_hits.get(), s->q_rng.get(), s->st)) return rc;
  const vpt_sdf_aov_planes planes = {nullptr, nullptr, nullptr, s->q_ids.get(), s->q_hit.get()};
  if (int rc = vpt_render_sdf_aov_device(s->scene, &p, &s->lay, 1, &planes, s->q_hits.get(), s->q_rng.get(), s->st)) return rc;
  if (int rc = vpt_resolve_sdf_ids_device(&s->lay, s->q_ids.get(), s->q_hit.get(), s->sdf_ids.get(), s->sdf_hit.get(), s->st)) return rc;
  s->launches += 3;
  s->sdf_ids_valid = true;
  return VPT_OK;
}

int reset(vpt_session* s, const vpt_session_params& np) {
  vpt_camera cam;
  if (int rc = vpt_scene_get_camera(s->scene, np.render.camera, &cam)) return rc;
  s->down += sizeof(vpt_camera);
  int width = 0, height = 0, pw = 0, ph = 0;
  frame_size(np.render.resolution, cam.aspect, width, height);
  frame_size(np.render.resolution / np.pratio, cam.aspect, pw, ph);
  REQUIRE(width >= 1 && height >= 1 && pw >= 1 && ph >= 1, "camera aspect %g leaves an empty frame (%d x %d, preview %d x %d)", (double)cam.aspect,
      width, height, pw, ph);
  HIP_TRY(hipStreamSynchronize(s->st));   // nothing of the previous frame is in flight when its buffers go
  drop_run(s);                            // an adaptive run ends here; the first advance makes the next
  if (width != s->width || height != s->height || pw != s->pw || ph != s->ph || (np.denoise != 0) != s->denoise_allocated)
    if (int rc = allocate(s, width, height, pw, ph, np.denoise != 0)) return rc;
  s->p = np, s->samples = 0, s->a = 0, s->filtered_valid = false, s->has_albedo = false, s->ids_valid = false, s->sdf_ids_valid = false;
  if (np.denoise) {
    if (implicit_shader(np.render.shader)) {
      if (int rc = render_guide(s, VPT_SHADER_IMPLICIT_NORMAL, s->normal.get())) return rc;
    } else {
      if (int rc = render_mesh_guides(s)) return rc;
      s->has_albedo = true;
    }
  }
  if (int rc = vpt_state_init_device(&s->lay, s->s_image.get(), s->s_hits.get(), s->s_rng.get(), s->st)) return rc;
  // the preview: a fresh state of resolution / pratio, samples = 1 (the pixel-centre branch), resolved and replicated
  vpt_params pp = np.render;
  pp.resolution = np.render.resolution / np.pratio, pp.samples = 1;
  if (int rc = vpt_state_init_device(&s->play, s->p_image.get(), s->p_hits.get(), s->p_rng.get(), s->st)) return rc;
  if (int rc = vpt_render_device(s->scene, &pp, &s->play, 1, s->p_image.get(), s->p_hits.get(), s->p_rng.get(), s->st)) return rc;
  if (int rc = vpt_resolve_device(&s->play, s->p_image.get(), 1, s->p_rows.get(), s->st)) return rc;
  if (int rc = vpt_upscale_device(np.pratio, pw, ph, s->p_rows.get(), width, height, s->image.get(), s->st)) return rc;
  s->launches += 5;
  if (int rc = tonemap_display(s)) return rc;
  if (implicit_shader(np.render.shader)) {   // the implicit kernels ran: their watchdog
    HIP_TRY(hipStreamSynchronize(s->st));
    if (int rc = vpt_check_watchdog(s->scene)) return rc;
    s->down += 4;
  }
  return VPT_OK;
}

int fetch(vpt_session* s, void* host, const device_buffer& from, size_t bytes) {
  HIP_TRY(hipMemcpyAsync(host, from.get(), bytes, hipMemcpyDeviceToHost, s->st));
  s->down += (int64_t)bytes;
  return VPT_OK;
}

// vpt_session_advance in adaptive mode (include/vpt.h): whole rounds of the run, the per-pixel resolve, the noise planes, the filter
// with the handed-over variance, the tone map
int advance_adaptive(vpt_session* s, int nsamples) {
  const int want = (int)(((long long)nsamples + s->ad.step - 1) / s->ad.step);
  if (want <= 0) return VPT_OK;
  HIP_TRY(hipSetDevice(s->device));
  void *img = s->s_image.get(), *hit = s->s_hits.get(), *rng = s->s_rng.get();
  const size_t n = (size_t)s->width * s->height;
  if (!s->run) {
    if (s->a_pixels != (long long)n) {
      s->a_pixels = 0;
      for (device_buffer* b : {&s->a_se2, &s->a_var, &s->a_hits, &s->a_mean, &s->a_m2})
        if (int rc = b->allocate(n * 4)) return rc;
      s->a_pixels = (long long)n;
    }
    if (int rc = vpt_adaptive_run_create(s->scene, &s->p.render, &s->ad, &s->lay, img, hit, rng, s->st, &s->run)) return rc;
    s->launches++, s->down += 16;
  }
  int     done = 0, active = 0, rounds = 0, hits = 0;
  int64_t taken = 0;
  if (int rc = vpt_adaptive_run_rounds(s->run, want, &done, &taken, &active)) return rc;
  if (done == 0) return VPT_OK;   // every pixel has stopped: nothing was enqueued, state and displays stay
  s->launches += done, s->down += (implicit_shader(s->p.render.shader) ? 20 : 16) * (int64_t)done;   // the read-back, the watchdog's word
  if (int rc = vpt_adaptive_run_progress(s->run, &rounds, nullptr, nullptr, &hits)) return rc;
  s->samples = hits;
  if (int rc = vpt_resolve_hits_device(&s->lay, img, hit, s->image.get(), s->st)) return rc;
  if (int rc = vpt_adaptive_run_noise_device(s->run, s->a_se2.get(), s->a_hits.get(), s->st)) return rc;
  if (int rc = vpt_box3_device(s->width, s->height, s->a_se2.get(), s->a_var.get(), s->st)) return rc;
  s->launches += 3;
  if (s->p.denoise) {
    if (int rc = vpt_denoise_device(&s->p.filter, s->width, s->height, s->image.get(), s->normal.get(), s->has_albedo ? s->albedo.get() : nullptr,
            rounds >= 2 ? s->a_var.get() : nullptr, s->filtered.get(), s->scratch.get(), s->st))
      return rc;
    s->filtered_valid = true, s->launches++;
  }
  return tonemap_display(s);
}

// one of the edits of a resident scene - apply(scene, edit) is its vpt_scene_* entry point - then a reset
template <class Edit, class Apply>
int session_edit(vpt_session* s, const Edit* edit, Apply apply) {
  REQUIRE(s && edit, "null argument");
  begin_call(s);
  if (int rc = apply(s->scene, edit)) return rc;   // a refused edit has changed nothing, here or there
  int     launches = 0;
  int64_t bytes    = 0;
  float   ms       = 0;
  if (vpt_scene_update_stats(s->scene, &launches, &bytes, &ms) == VPT_OK) s->launches += launches, s->up += bytes;
  return reset(s, s->p);
}

}  // namespace

extern "C" {

int vpt_session_create(vpt_scene* scene, const vpt_session_params* params, vpt_session** out) {
  REQUIRE(scene && out, "null argument");
  *out = nullptr;
  if (int rc = check_session_params(params)) return rc;
  const int device = vpt_scene_get_device(scene);
  if (device < 0) return device;
  HIP_TRY(hipSetDevice(device));
  vpt_session* s = new vpt_session{};
  s->scene = scene, s->device = device;
  struct guard { vpt_session*& s; ~guard() { if (s) vpt_session_destroy(s); } } g{s};
  HIP_TRY(hipStreamCreate(&s->st));
  if (int rc = reset(s, *params)) return rc;
  *out = s;
  s    = nullptr;   // release the guard
  return VPT_OK;
}

void vpt_session_destroy(vpt_session* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);   // the buffers are freed on the session's device
  drop_run(s);
  if (s->st) (void)hipStreamSynchronize(s->st), (void)hipStreamDestroy(s->st);
  delete s;
}

int vpt_session_reset(vpt_session* s, const vpt_session_params* params_or_null) {
  REQUIRE(s, "null session");
  if (params_or_null)
    if (int rc = check_session_params(params_or_null)) return rc;
  if (params_or_null && s->adaptive)
    if (int rc = check_session_adaptive(&s->ad, params_or_null->render.samples)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  const vpt_session_params np = params_or_null ? *params_or_null : s->p;
  return reset(s, np);
}

int vpt_session_advance(vpt_session* s, int nsamples) {
  REQUIRE(s, "null session");
  REQUIRE(nsamples >= 0, "negative sample count");
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  begin_call(s);
  if (s->adaptive) return advance_adaptive(s, nsamples);
  const int todo = std::min(nsamples, s->p.render.samples - s->samples);   // a no-op once reached, yocto_pathtrace.cpp:1055
  if (todo <= 0) return VPT_OK;
  HIP_TRY(hipSetDevice(s->device));
  void *img = s->s_image.get(), *hit = s->s_hits.get(), *rng = s->s_rng.get();
  if (s->p.denoise && s->samples > 0 && s->samples >= 2 * s->a) {   // the variance rule of include/vpt.h: keep the sums of the first half
    if (int rc = vpt_resolve_device(&s->lay, img, 1, s->sum_a.get(), s->st)) return rc;   // * (1 / 1): the sums themselves, row-major
    s->a = s->samples, s->launches++;
  }
  if (int rc = vpt_render_device(s->scene, &s->p.render, &s->lay, todo, img, hit, rng, s->st)) return rc;
  s->samples += todo;
  if (int rc = vpt_resolve_device(&s->lay, img, s->samples, s->image.get(), s->st)) return rc;
  s->launches += 2;
  if (s->p.denoise) {
    if (s->a > 0) {
      if (int rc = vpt_resolve_device(&s->lay, img, 1, s->sum_n.get(), s->st)) return rc;
      if (int rc = vpt_half_variance_device(s->width, s->height, s->sum_a.get(), s->a, s->sum_n.get(), s->samples, s->variance.get(), s->st)) return rc;
      s->launches += 2;
    }
    if (int rc = vpt_denoise_device(&s->p.filter, s->width, s->height, s->image.get(), s->normal.get(), s->has_albedo ? s->albedo.get() : nullptr,
            s->a > 0 ? s->variance.get() : nullptr, s->filtered.get(), s->scratch.get(), s->st))
      return rc;
    s->filtered_valid = true, s->launches++;
  }
  if (int rc = tonemap_display(s)) return rc;
  if (implicit_shader(s->p.render.shader)) {
    HIP_TRY(hipStreamSynchronize(s->st));
    if (int rc = vpt_check_watchdog(s->scene)) return rc;
    s->down += 4;   // the watchdog's word
  }
  return VPT_OK;
}

int vpt_session_set_display(vpt_session* s, const vpt_display_params* display) {
  REQUIRE(s, "null session");
  if (int rc = check_display(display)) return rc;
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  s->p.display = *display;
  return tonemap_display(s);
}

int vpt_session_edit(vpt_session* s, const vpt_scene_edit* edit) { return session_edit(s, edit, vpt_scene_update); }
int vpt_session_edit_lights(vpt_session* s, const vpt_scene_edit* edit) { return session_edit(s, edit, vpt_scene_update_lights); }
int vpt_session_edit_textures(vpt_session* s, const vpt_texture_edit* edit) { return session_edit(s, edit, vpt_scene_update_textures); }
int vpt_session_edit_volumes(vpt_session* s, const vpt_volume_edit* edit) { return session_edit(s, edit, vpt_scene_update_volumes); }
int vpt_session_sculpt_volumes(vpt_session* s, const vpt_sculpt_edit* edit) { return session_edit(s, edit, vpt_scene_sculpt_volumes); }
int vpt_session_rebuild_bvh(vpt_session* s, const vpt_bvh_rebuild* what) { return vpt_session_rebuild_bvh_quality(s, what, VPT_BVH_MIDDLE); }
int vpt_session_rebuild_bvh_quality(vpt_session* s, const vpt_bvh_rebuild* what, int quality) {
  return session_edit(s, what, [quality](vpt_scene* scene, const vpt_bvh_rebuild* w) { return vpt_scene_rebuild_bvh_quality(scene, w, quality); });
}
int vpt_session_edit_instances(vpt_session* s, const vpt_instance_edit* edit) { return session_edit(s, edit, vpt_scene_update_instances); }
int vpt_session_edit_shapes(vpt_session* s, const vpt_shape_edit* edit) { return session_edit(s, edit, vpt_scene_update_shapes); }
int vpt_session_edit_subdivs(vpt_session* s, const vpt_subdiv_edit* edit) { return session_edit(s, edit, vpt_scene_update_subdivs); }

int vpt_session_get_display(vpt_session* s, uint8_t* rgba8, float* display_f) {
  REQUIRE(s, "null session");
  REQUIRE(rgba8 || display_f, "null rgba8 and display_f: nothing to fetch");
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  const size_t n = (size_t)s->width * s->height;
  if (rgba8)
    if (int rc = fetch(s, rgba8, s->rgba8, n * 4)) return rc;
  if (display_f)
    if (int rc = fetch(s, display_f, s->display_f, n * 16)) return rc;
  HIP_TRY(hipStreamSynchronize(s->st));
  return VPT_OK;
}

int vpt_session_get_image(vpt_session* s, float* linear) {
  REQUIRE(s && linear, "null argument");
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  if (int rc = fetch(s, linear, s->image, (size_t)s->width * s->height * 16)) return rc;
  HIP_TRY(hipStreamSynchronize(s->st));
  return VPT_OK;
}

int vpt_session_get_denoised(vpt_session* s, float* linear) {
  REQUIRE(s && linear, "null argument");
  REQUIRE(s->filtered_valid, "no filtered image: the session needs denoise = 1 and an advance since its last reset");
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  if (int rc = fetch(s, linear, s->filtered, (size_t)s->width * s->height * 16)) return rc;
  HIP_TRY(hipStreamSynchronize(s->st));
  return VPT_OK;
}

int vpt_session_get_state(vpt_session* s, float* image_rgba, int32_t* hits, uint64_t* rng, int* samples) {
  REQUIRE(s && image_rgba && hits && rng && samples, "null argument");
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  const size_t n = (size_t)s->width * s->height;
  if (s->r_pixels != (long long)n) {
    s->r_pixels = 0;
    if (int rc = s->r_image.allocate(n * 16)) return rc;
    if (int rc = s->r_hits.allocate(n * 4)) return rc;
    if (int rc = s->r_rng.allocate(n * 16)) return rc;
    s->r_pixels = (long long)n;
  }
  // the one-rank layout owns every pixel: the row-major staging is written in full
  const layout_plane state[3] = {{s->s_image.get(), s->r_image.get(), 16}, {s->s_hits.get(), s->r_hits.get(), 4}, {s->s_rng.get(), s->r_rng.get(), 16}};
  if (int rc = layout_copy(&s->lay, LAYOUT_TILES_TO_ROWS, state, 3, s->st)) return rc;
  s->launches++;
  if (int rc = fetch(s, image_rgba, s->r_image, n * 16)) return rc;
  if (int rc = fetch(s, hits, s->r_hits, n * 4)) return rc;
  if (int rc = fetch(s, rng, s->r_rng, n * 16)) return rc;
  HIP_TRY(hipStreamSynchronize(s->st));
  *samples = s->samples;
  return VPT_OK;
}

int vpt_session_get_guides(vpt_session* s, float* normal, float* albedo) {
  REQUIRE(s, "null session");
  REQUIRE(normal || albedo, "null normal and albedo: nothing to fetch");
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  REQUIRE(s->p.denoise, "no guides: the session needs denoise = 1");
  REQUIRE(!albedo || s->has_albedo, "no albedo guide: the implicit shaders have none");
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  const size_t n = (size_t)s->width * s->height;
  if (normal)
    if (int rc = fetch(s, normal, s->normal, n * 16)) return rc;
  if (albedo)
    if (int rc = fetch(s, albedo, s->albedo, n * 16)) return rc;
  HIP_TRY(hipStreamSynchronize(s->st));
  return VPT_OK;
}

int vpt_session_get_ids(vpt_session* s, int32_t* ids, float* uvt) {
  REQUIRE(s, "null session");
  REQUIRE(ids || uvt, "null ids and uvt: nothing to fetch");
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  if (int rc = ensure_ids(s)) return rc;
  const size_t n = (size_t)s->width * s->height;
  if (ids)
    if (int rc = fetch(s, ids, s->ids, n * 8)) return rc;
  if (uvt)
    if (int rc = fetch(s, uvt, s->uvt, n * 12)) return rc;
  HIP_TRY(hipStreamSynchronize(s->st));
  return VPT_OK;
}

int vpt_session_pick(vpt_session* s, int x, int y, vpt_pick* out) {
  REQUIRE(s && out, "null argument");
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  REQUIRE(x >= 0 && x < s->width && y >= 0 && y < s->height, "pixel (%d, %d) outside the %d x %d frame", x, y, s->width, s->height);
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  if (int rc = ensure_ids(s)) return rc;
  hipLaunchKernelGGL(vpt_pick_kernel, dim3(1), dim3(64), 0, s->st, s->ids.get<const int2>(), s->uvt.get<const float>(), (long long)y * s->width + x,
      s->pick.get<int>());
  HIP_TRY(hipGetLastError());
  s->launches++;
  struct { int32_t hit, instance, element; float u, v, distance; } rec;
  static_assert(sizeof(rec) == 24, "the 24 bytes of a pick");
  HIP_TRY(hipMemcpyAsync(&rec, s->pick.get(), sizeof(rec), hipMemcpyDeviceToHost, s->st));
  s->down += (int64_t)sizeof(rec);
  HIP_TRY(hipStreamSynchronize(s->st));
  *out = {rec.hit, rec.instance, rec.element, -1, -1, rec.u, rec.v, rec.distance};
  if (rec.hit && (size_t)rec.instance < s->instances.size()) out->shape = s->instances[(size_t)rec.instance].shape, out->material = s->instances[(size_t)rec.instance].material;
  return VPT_OK;
}

int vpt_session_get_sdf_ids(vpt_session* s, int32_t* ids, float* hit) {
  REQUIRE(s, "null session");
  REQUIRE(ids || hit, "null ids and hit: nothing to fetch");
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  if (int rc = ensure_sdf_ids(s)) return rc;
  const size_t n = (size_t)s->width * s->height;
  if (ids)
    if (int rc = fetch(s, ids, s->sdf_ids, n * 8)) return rc;
  if (hit)
    if (int rc = fetch(s, hit, s->sdf_hit, n * 16)) return rc;
  HIP_TRY(hipStreamSynchronize(s->st));
  return VPT_OK;
}

int vpt_session_pick_sdf(vpt_session* s, int x, int y, vpt_sdf_pick* out) {
  static_assert(sizeof(vpt_sdf_pick) == 48, "the 48 bytes of a pick");
  REQUIRE(s && out, "null argument");
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  REQUIRE(x >= 0 && x < s->width && y >= 0 && y < s->height, "pixel (%d, %d) outside the %d x %d frame", x, y, s->width, s->height);
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  if (int rc = ensure_sdf_ids(s)) return rc;
  if (int rc = vpt_sdf_pick_device(s->scene, s->sdf_ids.get(), s->sdf_hit.get(), (long long)y * s->width + x, s->sdf_pick.get(), s->st)) return rc;
  s->launches++;
  HIP_TRY(hipMemcpyAsync(out, s->sdf_pick.get(), sizeof(vpt_sdf_pick), hipMemcpyDeviceToHost, s->st));
  s->down += (int64_t)sizeof(vpt_sdf_pick);
  HIP_TRY(hipStreamSynchronize(s->st));
  return VPT_OK;
}

int vpt_session_set_adaptive(vpt_session* s, const vpt_adaptive* a) {
  REQUIRE(s, "null session");
  if (a)
    if (int rc = check_session_adaptive(a, s->p.render.samples)) return rc;
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  s->adaptive = a != nullptr;
  if (a) s->ad = *a;
  return reset(s, s->p);
}

int vpt_session_progress(const vpt_session* s, int* rounds, int64_t* rendered, int* active) {
  REQUIRE(s, "null session");
  REQUIRE(s->adaptive, "the session is not in adaptive mode");
  if (s->run) return vpt_adaptive_run_progress(s->run, rounds, rendered, active, nullptr);
  if (rounds) *rounds = 0;
  if (rendered) *rendered = 0;
  if (active) *active = s->width * s->height;   // nothing has rendered: every pixel is to
  return VPT_OK;
}

int vpt_session_get_hits(vpt_session* s, int32_t* hits) {
  REQUIRE(s && hits, "null argument");
  REQUIRE(s->adaptive, "the session is not in adaptive mode");
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  begin_call(s);
  const size_t n = (size_t)s->width * s->height;
  if (!s->run) {
    memset(hits, 0, n * 4);
    return VPT_OK;
  }
  HIP_TRY(hipSetDevice(s->device));
  if (int rc = fetch(s, hits, s->a_hits, n * 4)) return rc;
  HIP_TRY(hipStreamSynchronize(s->st));
  return VPT_OK;
}

int vpt_session_get_noise(vpt_session* s, float* se2, float* variance) {
  REQUIRE(s, "null session");
  REQUIRE(se2 || variance, "null se2 and variance: nothing to fetch");
  REQUIRE(s->adaptive, "the session is not in adaptive mode");
  REQUIRE(s->run, "no noise estimate: no advance has run since the last reset");
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  const size_t n = (size_t)s->width * s->height;
  if (se2)
    if (int rc = fetch(s, se2, s->a_se2, n * 4)) return rc;
  if (variance)
    if (int rc = fetch(s, variance, s->a_var, n * 4)) return rc;
  HIP_TRY(hipStreamSynchronize(s->st));
  return VPT_OK;
}

int vpt_session_get_adaptive_stats(vpt_session* s, float* mean, float* m2) {
  REQUIRE(s && mean && m2, "null argument");
  REQUIRE(s->adaptive, "the session is not in adaptive mode");
  REQUIRE(s->run, "no statistics: no advance has run since the last reset");
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  const size_t n = (size_t)s->width * s->height;
  if (int rc = vpt_adaptive_run_stats_device(s->run, s->a_mean.get(), s->a_m2.get(), s->st)) return rc;
  s->launches++;
  if (int rc = fetch(s, mean, s->a_mean, n * 4)) return rc;
  if (int rc = fetch(s, m2, s->a_m2, n * 4)) return rc;
  HIP_TRY(hipStreamSynchronize(s->st));
  return VPT_OK;
}

int vpt_session_size(const vpt_session* s, int* width, int* height) {
  REQUIRE(s && width && height, "null argument");
  *width = s->width, *height = s->height;
  return VPT_OK;
}

int vpt_session_samples(const vpt_session* s) { return s ? s->samples : vpt_set_error(VPT_ERR_INVALID_ARG, "null session"); }

int vpt_session_stats(const vpt_session* s, int* launches, int64_t* bytes_to_device, int64_t* bytes_to_host) {
  REQUIRE(s && launches && bytes_to_device && bytes_to_host, "null argument");
  *launches = s->launches, *bytes_to_device = s->up, *bytes_to_host = s->down;
  return VPT_OK;
}

}  // extern "C"
