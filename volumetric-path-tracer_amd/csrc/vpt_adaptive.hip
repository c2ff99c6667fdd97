// vpt_adaptive.hip — adaptive sampling on the device (include/vpt.h: vpt_adaptive_run, vpt_render_device_adaptive,
// vpt_render_adaptive, vpt_resolve_hits_device, vpt_box3_device), whole: kernels, their launchers, the round loop, the C-ABI.
// After every round of the loop below: the noise estimate of each pixel still rendering, the stop decision, and a
// stable compaction of the pixels left into the lane -> slot table the render kernels read (sched_cfg::lane_slot), so that
// they run 64 to a wave and converged pixels leave the launch.  For a session: the statistics as row-major planes
// and the box3 that makes the filter's variance of them.  Plain C++, vector stores only.  The render kernels of a round are
// launched through the scene handle's render side (vpt_scene_handle.h: traversal_setup, launcher_of).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <memory>
#include "vpt_kernels.hip.h"
#include "vpt_scene_handle.h"

// Scratch of a run, sized for pr.nslots (a multiple of 64):
//   stats      float4 per slot: {lum_prev, mean, m2, active (int bits)}
//   wave_count int per 64 slots: pixels of the 64 still rendering, turned into exclusive offsets by the scan
//   lane_slot  int per slot: the dense [waves][64] table of the slots still rendering, tile-major, padded with -1
//   info       int[4]: {active pixels, min hits, max hits (both from the first call only), unused}
struct adaptive_buffers {
  float4* stats;
  int*    wave_count;
  int*    lane_slot;
  int*    info;
};

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

// b.stats and `hits` (tile-major) as row-major width x height planes, each nullable: the squared standard error of vpt.h's rule
// with n_p = ceil(hits / step), the hits, and the Welford mean and m2 themselves.  Pixels of other ranks are left as they are.
static int adaptive_noise(const DParams& pr, const adaptive_buffers& b, const int* hits, int step, float* se2, int* hits_out, float* mean_out,
    float* m2_out, hipStream_t st) {
  hipLaunchKernelGGL(vpt_adaptive_noise_kernel, dim3((pr.nslots + k_block - 1) / k_block), dim3(k_block), 0, st, pr, (const float4*)b.stats, hits,
      step, se2, hits_out, mean_out, m2_out);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

// n == 0: start (lum_prev from the entry image, active = slot owns a pixel and hits < cap, min / max of hits);
// n >= 1: the pixels still active have just rendered their n-th round of m samples: update and decide (vpt.h).
// Then the compaction of the active slots into b.lane_slot and their count into b.info[0].  Asynchronous on `st`.
static int adaptive_update(const DParams& pr, const float4* image, const int* hits, const adaptive_buffers& b, int n, int m,
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
  REQUIRE(layout && d_tiles_all_ranks && d_hits_all_ranks && d_image_rowmajor, "null argument");
  DParams pr;
  if (int rc = vpt_layout_dparams(layout, pr)) return rc;
  long long total = (long long)pr.nslots * pr.nranks;
  REQUIRE(total < (1LL << 31), "image too large");
  hipLaunchKernelGGL(vpt_resolve_hits_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pr,
      (const float4*)d_tiles_all_ranks, (const int*)d_hits_all_ranks, (float4*)d_image_rowmajor);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

// vpt_adaptive_run (include/vpt.h): what the round loop of an adaptive render holds between rounds
struct vpt_adaptive_run {
  vpt_scene*       s = nullptr;
  vpt_params       params = {};
  vpt_adaptive     a = {};
  DParams          pr = {};
  hipStream_t      st = nullptr;
  float4*          img = nullptr;
  int*             hit = nullptr;
  ulonglong2*      rng = nullptr;
  bool             implicit = false;
  device_buffer    d_stats, d_wave_count, d_lane_slot, d_info;   // adaptive_buffers, sized for the full layout
  adaptive_buffers b = {};
  int              info[4] = {0, 0, 0, 0};   // the last read-back: {pixels still rendering, min hits, max hits on entry, unused}
  int              h = 0, n = 0;             // hits of every pixel still rendering, rounds so far
  long long        taken = 0;                // samples so far
  bool             timing_open = false;      // ev0 was recorded by create and no round has run since
  int read_info() {   // the one read-back of a round: what sizes the next launch
    HIP_TRY(hipMemcpyAsync(info, b.info, sizeof(info), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return VPT_OK;
  }
};

// the arguments of an adaptive render, checked before anything touches the device
static int check_adaptive(const vpt_scene* s, const vpt_params* params, const vpt_adaptive* a) {
  REQUIRE(params && a, "null argument");
  REQUIRE(std::isfinite(a->threshold) && a->threshold >= 0, "adaptive threshold must be finite and >= 0");
  REQUIRE(a->step >= 1, "adaptive step must be >= 1");
  REQUIRE(params->samples >= 1, "params->samples (the per-pixel cap) must be >= 1");
  REQUIRE(a->min_samples >= 1 && a->min_samples <= params->samples, "adaptive min_samples must be in 1 .. params->samples (%d)", params->samples);
  REQUIRE(params->bounces >= 0, "negative bounce count");
  REQUIRE(s, "null scene");
  if (int rc = check_shader(params)) return rc;
  return check_camera(s, params);
}

extern "C" {

// Adaptive sampling (include/vpt.h): rounds of one launch each over the pixels still rendering, packed 64 to a
// wave through sched_cfg::lane_slot by the kernels above.  No pilot, no order, no costs, no tile splitting: the handle's
// launch schedule for the layout stays as vpt_render_device left it.  A run holds what the round loop holds, so that the loop can
// stop after any round and go on in a later call.
int vpt_adaptive_run_create(vpt_scene* s, const vpt_params* params, const vpt_adaptive* a, const vpt_layout* layout, void* d_image,
    void* d_hits, void* d_rng, void* stream, vpt_adaptive_run** out) {
  REQUIRE(out, "null argument");
  *out = nullptr;
  if (int rc = check_adaptive(s, params, a)) return rc;
  REQUIRE(layout && d_image && d_hits && d_rng, "null argument");
  std::unique_ptr<vpt_adaptive_run> r(new vpt_adaptive_run{});
  if (int rc = make_dparams(params, layout, 0, r->pr)) return rc;
  r->s = s, r->params = *params, r->a = *a, r->st = (hipStream_t)stream;
  r->img = (float4*)d_image, r->hit = (int*)d_hits, r->rng = (ulonglong2*)d_rng;
  r->implicit = params->shader >= VPT_SHADER_IMPLICIT;   // K2 and K3: the kernels that report through the watchdog word
  HIP_TRY(hipSetDevice(s->device));
  if (int rc = shader_setup(s, params, r->st)) return rc;   // (an edit ends a run's validity: what is set up here holds for its rounds)
  const DParams&   pr = r->pr;
  traversal_launch full;   // the spilled stacks are indexed by global lane: sized for the full layout, a compacted grid is never larger
  if (int rc = traversal_setup(s, pr.nslots, full)) return rc;
  if (int rc = r->d_stats.allocate((size_t)pr.nslots * 16)) return rc;
  if (int rc = r->d_wave_count.allocate((size_t)full.grid.x * 4)) return rc;
  if (int rc = r->d_lane_slot.allocate((size_t)pr.nslots * 4)) return rc;
  if (int rc = r->d_info.allocate(16)) return rc;
  r->b = {r->d_stats.get<float4>(), r->d_wave_count.get<int>(), r->d_lane_slot.get<int>(), r->d_info.get<int>()};
  HIP_TRY(hipEventRecord(s->ev0, r->st));
  s->sched.no_pause();
  if (int rc = adaptive_update(pr, r->img, r->hit, r->b, 0, 0, r->a, params->samples, r->st)) return rc;
  if (int rc = r->read_info()) return rc;
  REQUIRE(r->info[1] >= r->info[2], "hits[] must be equal on entry (found %d .. %d)", r->info[1], r->info[2]);
  r->h = r->info[1], r->timing_open = true;
  *out = r.release();
  return VPT_OK;
}

int vpt_adaptive_run_rounds(vpt_adaptive_run* r, int max_rounds, int* rounds_done, int64_t* rendered, int* active) {
  if (rounds_done) *rounds_done = 0;
  if (rendered) *rendered = 0;
  if (active) *active = 0;
  REQUIRE(r, "null run");
  REQUIRE(max_rounds >= 0, "negative round count");
  vpt_scene* s   = r->s;
  const int  cap = r->params.samples;
  if (active) *active = r->info[0];
  if (max_rounds == 0 || r->info[0] <= 0 || r->h >= cap) return VPT_OK;   // nothing is enqueued
  HIP_TRY(hipSetDevice(s->device));
  const DParams&   pr = r->pr;
  traversal_launch full;   // taken per call: a larger launch on the handle in between may have moved the spilled stacks
  if (int rc = traversal_setup(s, pr.nslots, full)) return rc;
  const launch_ctx L = {s, r->st, r->img, r->hit, r->rng, full.stack, full.lds};
  if (!r->timing_open) {   // the first call's timing starts where the run was created; a later call's at its own first round
    HIP_TRY(hipEventRecord(s->ev0, r->st));
    s->sched.no_pause();
  }
  r->timing_open = false;
  int       done  = 0;
  long long taken = 0;
  for (int act = r->info[0]; done < max_rounds && act > 0 && r->h < cap; act = r->info[0]) {
    DParams rp  = pr;
    rp.nsamples = std::min(r->a.step, cap - r->h);
    const sched_cfg sch = {nullptr, nullptr, r->b.lane_slot};
    launcher_of(r->params.shader)(L, false, dim3((unsigned)((act + VPT_BLOCK - 1) / VPT_BLOCK)), rp, sch);
    HIP_TRY(hipGetLastError());
    taken += (long long)act * rp.nsamples, r->h += rp.nsamples, r->n++, done++;
    if (int rc = adaptive_update(pr, r->img, r->hit, r->b, r->n, rp.nsamples, r->a, cap, r->st)) return rc;
    if (int rc = r->read_info()) return rc;
    if (r->implicit)
      if (int rc = vpt_check_watchdog(s)) return rc;
  }
  HIP_TRY(hipEventRecord(s->ev1, r->st));
  s->timed = true;
  r->taken += taken;
  if (rounds_done) *rounds_done = done;
  if (rendered) *rendered = taken;
  if (active) *active = r->info[0];
  return VPT_OK;
}

int vpt_adaptive_run_progress(const vpt_adaptive_run* r, int* rounds, int64_t* rendered, int* active, int* max_hits) {
  REQUIRE(r, "null run");
  if (rounds) *rounds = r->n;
  if (rendered) *rendered = r->taken;
  if (active) *active = r->h >= r->params.samples ? 0 : r->info[0];
  if (max_hits) *max_hits = r->h;
  return VPT_OK;
}

int vpt_adaptive_run_noise_device(vpt_adaptive_run* r, void* d_se2_rowmajor, void* d_hits_rowmajor, void* stream) {
  REQUIRE(r && d_se2_rowmajor, "null argument");
  HIP_TRY(hipSetDevice(r->s->device));
  return adaptive_noise(r->pr, r->b, r->hit, r->a.step, (float*)d_se2_rowmajor, (int*)d_hits_rowmajor, nullptr, nullptr, (hipStream_t)stream);
}

int vpt_adaptive_run_stats_device(vpt_adaptive_run* r, void* d_mean_rowmajor, void* d_m2_rowmajor, void* stream) {
  REQUIRE(r && d_mean_rowmajor && d_m2_rowmajor, "null argument");
  HIP_TRY(hipSetDevice(r->s->device));
  return adaptive_noise(r->pr, r->b, r->hit, r->a.step, nullptr, nullptr, (float*)d_mean_rowmajor, (float*)d_m2_rowmajor, (hipStream_t)stream);
}

void vpt_adaptive_run_destroy(vpt_adaptive_run* r) {
  if (!r) return;
  (void)hipSetDevice(r->s->device);
  (void)hipStreamSynchronize(r->st);   // nothing reads the scratch when it goes
  delete r;
}

int vpt_render_device_adaptive(vpt_scene* s, const vpt_params* params, const vpt_adaptive* a, const vpt_layout* layout, void* d_image,
    void* d_hits, void* d_rng, void* stream, int* rounds, int64_t* rendered) {
  if (rounds) *rounds = 0;
  if (rendered) *rendered = 0;
  vpt_adaptive_run* r = nullptr;
  if (int rc = vpt_adaptive_run_create(s, params, a, layout, d_image, d_hits, d_rng, stream, &r)) return rc;
  struct guard { vpt_adaptive_run* r; ~guard() { vpt_adaptive_run_destroy(r); } } g{r};
  int     n     = 0;
  int64_t taken = 0;
  if (int rc = vpt_adaptive_run_rounds(r, INT_MAX, &n, &taken, nullptr)) return rc;
  if (n == 0) {   // nothing to render: the call's timing still closes, as it always has
    HIP_TRY(hipEventRecord(s->ev1, (hipStream_t)stream));
    s->timed = true;
  }
  if (rounds) *rounds = n;
  if (rendered) *rendered = taken;
  return VPT_OK;
}

int vpt_render_adaptive(vpt_scene* s, const vpt_params* params, const vpt_adaptive* a, int width, int height, float* image_rgba,
    int32_t* hits, uint64_t* rng, int* samples_io, int64_t* rendered) {
  if (rendered) *rendered = 0;
  if (int rc = check_adaptive(s, params, a)) return rc;
  REQUIRE(image_rgba && hits && rng && samples_io, "null argument");
  REQUIRE(width > 0 && height > 0, "bad image size");
  const long long pixels = (long long)width * height;
  for (long long i = 1; i < pixels; i++)
    REQUIRE(hits[i] == hits[0], "hits[] must be equal on entry (pixel %lld has %d, pixel 0 %d)", i, hits[i], hits[0]);
  *samples_io = hits[0];
  if (hits[0] >= params->samples) return VPT_OK;
  if (int rc = render_staged(s, width, height, image_rgba, hits, rng, [&](const vpt_layout* lay, void* const* t) {
        return vpt_render_device_adaptive(s, params, a, lay, t[0], t[1], t[2], nullptr, nullptr, rendered);
      }))
    return rc;
  *samples_io = *std::max_element(hits, hits + pixels);
  return VPT_OK;
}

}  // extern "C"
