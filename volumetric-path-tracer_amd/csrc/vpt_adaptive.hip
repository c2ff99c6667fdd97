// vpt_adaptive.hip — adaptive sampling on the device (include/vpt.h: vpt_adaptive_run, vpt_render_device_adaptive,
// vpt_resolve_hits_device, vpt_box3_device).
// After every round of the loop in vpt_capi.hip: the noise estimate of each pixel still rendering, the stop decision, and a
// stable compaction of the pixels left into the lane -> slot table the render kernels read (sched_cfg::lane_slot), so that
// they run 64 to a wave and converged pixels leave the launch.  For a session: the statistics as row-major planes
// and the box3 that makes the filter's variance of them.  Plain C++, vector stores only.
#include <cstdint>
#include "vpt_kernels.hip.h"
#include "vpt_adaptive.h"
#include "vpt_layout.h"   // vpt_layout_dparams

namespace {
constexpr int k_block = 256;   // four waves of 64 slots each
constexpr int k_scan  = 1024;  // threads of the one-block scan

VPT_DEV int lanes_below_mask(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
}  // namespace

// One lane per tile-major slot; the grid covers whole waves of slots (pr.nslots is a multiple of 64), so each wave is either
// entirely inside the layout or entirely past its end.  The rule is the one include/vpt.h states for vpt_adaptive.
__global__ void __launch_bounds__(k_block) vpt_adaptive_update_kernel(DParams pr, const float4* __restrict__ image,
    const int* __restrict__ hits, float4* __restrict__ stats, int* __restrict__ wave_count, int* __restrict__ info, int n, float m,
    float threshold, int min_samples, int cap) {
  const int slot = blockIdx.x * k_block + threadIdx.x;
  if (slot - (int)(threadIdx.x & 63) >= pr.nslots) return;   // the whole wave is past the layout
  const int lane = threadIdx.x & 63;
  bool active = false;
  if (n == 0) {
    int px, py;
    const bool owner = slot_to_pixel(pr, slot, px, py);
    int lo = 0x7fffffff, hi = (int)0x80000000;
    float4 st = make_float4(0, 0, 0, 0);
    if (owner) {
      const float4 v = image[slot];
      const int    h = hits[slot];
      st.x = (v.x + v.y + v.z) / 3.0f, lo = h, hi = h;
      active = h < cap;
    }
    st.w = __int_as_float(active ? 1 : 0);
    stats[slot] = st;
    for (int d = 32; d > 0; d >>= 1) lo = min(lo, __shfl_xor(lo, d)), hi = max(hi, __shfl_xor(hi, d));
    if (lane == 0 && lo <= hi) atomicMin(&info[1], lo), atomicMax(&info[2], hi);
  } else {
    float4 st = stats[slot];
    if (__float_as_int(st.w) != 0) {
      const float4 v = image[slot];
      const float  L = (v.x + v.y + v.z) / 3.0f;
      const float  b = (L - st.x) / m;   // mean luminance of this round's samples
      st.x = L;
      const float delta = b - st.y;      // Welford over the rounds' means
      st.y = st.y + delta / (float)n;
      st.z = st.z + delta * (b - st.y);
      const int h    = hits[slot];
      bool      done = h >= cap;
      if (threshold > 0 && n >= 2 && h >= min_samples) {
        const float var = st.z / ((float)n * (float)(n - 1));   // squared standard error of the pixel's mean
        const float tol = threshold * fmaxf(st.y, 1.0f / 256.0f);
        done = done || var <= tol * tol;
      }
      active = !done;
      st.w   = __int_as_float(active ? 1 : 0);
      stats[slot] = st;
    }
  }
  const unsigned long long mask = __builtin_amdgcn_ballot_w64(active);
  if (lane == 0) wave_count[slot >> 6] = __popcll(mask);
}

// Exclusive scan of the per-wave counts in place, in one block: each thread sums a contiguous run, the block scans the runs'
// sums, each thread writes its run's offsets.  info[0] = total.
__global__ void __launch_bounds__(k_scan) vpt_adaptive_scan_kernel(int* __restrict__ wave_count, int nwaves, int* __restrict__ info) {
  __shared__ int s_wave[k_scan / 64];
  const int per = (nwaves + k_scan - 1) / k_scan;
  const int lo = min(nwaves, (int)threadIdx.x * per), hi = min(nwaves, lo + per);
  int sum = 0;
  for (int i = lo; i < hi; i++) sum += wave_count[i];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = sum;   // inclusive scan inside the wave
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) s_wave[w] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int k = 0; k < k_scan / 64; k++) {
      const int t = s_wave[k];
      s_wave[k] = acc, acc += t;
    }
    info[0] = acc;
  }
  __syncthreads();
  int run = s_wave[w] + x - sum;
  for (int i = lo; i < hi; i++) {
    const int c = wave_count[i];
    wave_count[i] = run, run += c;
  }
}

// The active slots, in tile-major order, to lane_slot[offset of their wave + active lanes below them]; the last wave of the
// table is padded with -1.  Tile-major order keeps neighbouring pixels in one wave.
__global__ void __launch_bounds__(k_block) vpt_adaptive_compact_kernel(DParams pr, const float4* __restrict__ stats,
    const int* __restrict__ wave_offset, const int* __restrict__ info, int* __restrict__ lane_slot) {
  const int slot = blockIdx.x * k_block + threadIdx.x;
  if (slot - (int)(threadIdx.x & 63) >= pr.nslots) return;
  const bool active = __float_as_int(stats[slot].w) != 0;
  const unsigned long long mask = __builtin_amdgcn_ballot_w64(active);
  if (active) lane_slot[wave_offset[slot >> 6] + lanes_below_mask(mask)] = slot;
  if (blockIdx.x == 0 && threadIdx.x < 64) {   // padding: [total, total rounded up to 64), never past nslots
    const int total = info[0], p = total + (int)threadIdx.x;
    if (p < ((total + 63) & ~63)) lane_slot[p] = -1;
  }
}

// get_render with each pixel's own sample count: the gathered tile-major float4 sums and hit counts of all ranks
// ([nranks][nslots]) -> row-major image[p] * (1 / hits[p]); a pixel without hits gives 0.  The reciprocal is the same
// correctly rounded quotient vpt_resolve_device takes on the host, so a uniform hits[] gives the same bits.
__global__ void vpt_resolve_hits_kernel(DParams pr, const float4* __restrict__ tiles_all, const int* __restrict__ hits_all,
    float4* __restrict__ rows_image) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= pr.nslots * pr.nranks) return;
  DParams q = pr;
  q.rank    = g / pr.nslots;
  int px, py;
  if (!slot_to_pixel(q, g - q.rank * pr.nslots, px, py)) return;
  const int h = hits_all[g];
  float4    out = make_float4(0, 0, 0, 0);
  if (h > 0) {
    const float4 v     = tiles_all[g];
    const float  scale = 1.0f / (float)h;
    out = make_float4(v.x * scale, v.y * scale, v.z * scale, v.w * scale);
  }
  rows_image[(long long)py * pr.width + px] = out;
}

// The statistics of a run as row-major planes (include/vpt.h: vpt_adaptive_run_noise_device).  One lane per tile-major slot, whole
// waves inside or outside the layout as in the update kernel; a lane whose slot owns no pixel writes nothing.  Each plane is
// optional: a null pointer is the same for every lane, so the branches are uniform.
__global__ void __launch_bounds__(k_block) vpt_adaptive_noise_kernel(DParams pr, const float4* __restrict__ stats,
    const int* __restrict__ hits, int step, float* __restrict__ se2, int* __restrict__ hits_out, float* __restrict__ mean_out,
    float* __restrict__ m2_out) {
  const int slot = blockIdx.x * k_block + threadIdx.x;
  if (slot - (int)(threadIdx.x & 63) >= pr.nslots) return;   // the whole wave is past the layout
  int px, py;
  if (!slot_to_pixel(pr, slot, px, py)) return;   // padding, or another rank's
  const float4    st = stats[slot];
  const int       h  = hits[slot];
  const int       n  = (h + step - 1) / step;   // rounds this pixel rendered (the run started from hits 0)
  const long long p  = (long long)py * pr.width + px;
  if (se2) se2[p] = n >= 2 ? st.z / ((float)n * (float)(n - 1)) : 0.0f;
  if (hits_out) hits_out[p] = h;
  if (mean_out) mean_out[p] = st.y;
  if (m2_out) m2_out[p] = st.z;
}

// box3 of a row-major float plane by the denoiser's rule (include/vpt.h; csrc/vpt_denoise.hip takes it the same way inside its two
// variance seeds): dy outer, dx inner, taps outside the image skipped, the count summed as 1s.  A wave is 64 pixels of one row.
__global__ void __launch_bounds__(k_block) vpt_box3_kernel(const float* __restrict__ in, float* __restrict__ out, int width, int height) {
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
      sum = sum + in[(size_t)qy * width + qx], count = count + 1.0f;
    }
  }
  out[(size_t)py * width + px] = sum / count;
}

extern "C" int vpt_box3_device(int width, int height, const void* d_in, void* d_out, void* stream) {
  REQUIRE(width >= 1 && height >= 1, "bad image size: width %d, height %d", width, height);
  REQUIRE((long long)width * height <= (1LL << 28), "image too large: width %d, height %d", width, height);   // as vpt_denoise: every index fits
  REQUIRE(d_in, "null in");
  REQUIRE(d_out, "null out");
  const uintptr_t a = (uintptr_t)d_in, b = (uintptr_t)d_out, bytes = (uintptr_t)width * height * 4;
  REQUIRE(!(a < b + bytes && b < a + bytes), "out aliases in");
  hipLaunchKernelGGL(vpt_box3_kernel, dim3((width + 63) / 64, (height + 3) / 4), dim3(k_block), 0, (hipStream_t)stream, (const float*)d_in,
      (float*)d_out, width, height);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

int adaptive_noise(const DParams& pr, const adaptive_buffers& b, const int* hits, int step, float* se2, int* hits_out, float* mean_out,
    float* m2_out, hipStream_t st) {
  hipLaunchKernelGGL(vpt_adaptive_noise_kernel, dim3((pr.nslots + k_block - 1) / k_block), dim3(k_block), 0, st, pr, (const float4*)b.stats, hits,
      step, se2, hits_out, mean_out, m2_out);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

int adaptive_update(const DParams& pr, const float4* image, const int* hits, const adaptive_buffers& b, int n, int m,
    const vpt_adaptive& a, int cap, hipStream_t st) {
  const int nwaves = pr.nslots / 64, blocks = (pr.nslots + k_block - 1) / k_block;
  if (n == 0) {
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(b.info + 1), 0x7fffffff, 1, st));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(b.info + 2), (int)0x80000000, 1, st));
  }
  hipLaunchKernelGGL(vpt_adaptive_update_kernel, dim3(blocks), dim3(k_block), 0, st, pr, image, hits, b.stats, b.wave_count, b.info, n,
      (float)m, a.threshold, a.min_samples, cap);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(vpt_adaptive_scan_kernel, dim3(1), dim3(k_scan), 0, st, b.wave_count, nwaves, b.info);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(vpt_adaptive_compact_kernel, dim3(blocks), dim3(k_block), 0, st, pr, (const float4*)b.stats, (const int*)b.wave_count,
      (const int*)b.info, b.lane_slot);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

extern "C" int vpt_resolve_hits_device(const vpt_layout* layout, const void* d_tiles_all_ranks, const void* d_hits_all_ranks,
    void* d_image_rowmajor, void* stream) {
  if (!layout || !d_tiles_all_ranks || !d_hits_all_ranks || !d_image_rowmajor) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  DParams pr;
  if (int rc = vpt_layout_dparams(layout, pr)) return rc;
  long long total = (long long)pr.nslots * pr.nranks;
  if (total >= (1LL << 31)) return vpt_set_error(VPT_ERR_INVALID_ARG, "image too large");
  hipLaunchKernelGGL(vpt_resolve_hits_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pr,
      (const float4*)d_tiles_all_ranks, (const int*)d_hits_all_ranks, (float4*)d_image_rowmajor);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}
