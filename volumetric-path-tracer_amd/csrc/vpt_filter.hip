// vpt_filter.hip — the voxel grids of a resident scene filtered in place: remap, separable blur, fractal value noise (include/vpt.h:
// vpt_scene_filter_volumes).  The arithmetic is csrc/vpt_filter_rule.h's, which the host mirror (host/vpt_filter.cpp)
// compiles too: this unit is built with -ffp-contract=off like it.  Here: the validation of an edit, the ops' records, and three kernels -
// the pointwise run, the blur of one 8 x 8 x 8 brick per workgroup through LDS, and the move of a blur's scratch into place.
#include <algorithm>
#include <vector>

#include "vpt_error.h"
#include "vpt_filter.h"
#include "vpt_filter_rule.h"
#include "vpt_update_helpers.h"

namespace {

struct filter_grid {
  int   w, h, d;               // the volume
  int   lo_x, lo_y, lo_z;      // the region
  int   rw, rh, rd;
  float origin[3], step[3];
};

// region voxel idx (x fastest) -> its place in the volume
__device__ inline size_t place_of(const filter_grid& g, unsigned idx, int& i, int& j, int& k) {
  const unsigned x = idx % (unsigned)g.rw, y = (idx / (unsigned)g.rw) % (unsigned)g.rh, z = idx / ((unsigned)g.rw * (unsigned)g.rh);
  i = g.lo_x + (int)x, j = g.lo_y + (int)y, k = g.lo_z + (int)z;
  return (size_t)i + (size_t)j * (size_t)g.w + (size_t)k * (size_t)g.w * (size_t)g.h;
}

// A run of pointwise ops (REMAP, NOISE).  One lane per voxel of the region (n <= 2^30 of them, x fastest: a wave's loads and stores of the
// grid are consecutive); the value is read once and written once however many ops there are.  The records are read-only and indexed by the
// loop counter alone, so every lane of a wave reads the same one: uniform loads into scalar registers, and the op loop, the switch on the
// type and the octave loop are uniform branches.
__global__ __launch_bounds__(BLOCK) void filter_pointwise_kernel(float* __restrict__ grid, filter_grid g, unsigned n, const vpt_filter_record* __restrict__ records, int num) {
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  int          i, j, k;
  const size_t at = place_of(g, idx, i, j, k);
  const float  sx = vpt_filter_sample(g.origin[0], g.step[0], i), sy = vpt_filter_sample(g.origin[1], g.step[1], j), sz = vpt_filter_sample(g.origin[2], g.step[2], k);
  float v = grid[at];
  for (int s = 0; s < num; s++) v = vpt_filter_pointwise(records[s], sx, sy, sz, v);
  grid[at] = v;
}

// One BLUR op: a workgroup makes one 8 x 8 x 8 brick of outputs (bricks counted from the region's corner).  T = 8 + 2R.
//  1. Stage.  The T^3 source nodes around the brick, indices clamped to the volume, into LDS: consecutive lanes read consecutive x of a
//     row (runs of T floats of the grid).  Layout A: row (ty, tz) at line * (T + 1), line = ty + T * tz.
//  2. x pass.  Lane = line: it reads its row into registers (stride T + 1, odd: 32 consecutive lanes touch 32 banks) and makes the row's
//     eight outputs from them - T LDS reads for eight outputs, not 8 (2R + 1).  Barrier; the outputs go to layout B, out[xo] at
//     ty * (8T + 1) + (xo + 8 tz), over the dead tile: the values wait in registers across the barrier, so ONE buffer serves all passes.
//  3. y pass.  Lane = m = xo + 8 tz (8T columns): it reads B[ty * (8T + 1) + m], consecutive lanes consecutive words, makes eight outputs.
//     Barrier; they go to layout C, out[yo] at tz * 72 + (xo + 8 yo) (72 = 8 mod 32: the 32 stores of a half wave touch 32 banks).
//  4. z pass.  Lane = xo + 8 yo (64 columns, one wave): it reads C[tz * 72 + lane], makes eight outputs and writes those inside the region
//     to the scratch buffer, region order: the volume itself is only read, so every workgroup sees it as it was before the op.
// Every LDS read is free of bank conflicts (lane-consecutive words, or an odd stride); the stores of 1. and 2. are two-way at worst.
// A region that is not a multiple of 8, or a volume narrower than the halo, takes the same path: the loads clamp, the stores are masked.
template <int R>
__global__ __launch_bounds__(BLOCK) void filter_blur_kernel(const float* __restrict__ grid, float* __restrict__ scratch, filter_grid g, unsigned bricks_x, unsigned bricks_y,
    const vpt_filter_record* __restrict__ record) {
  constexpr int T = 8 + 2 * R, SA = T + 1, QB = 8 * T + 1, QC = 72;
  static_assert(T * T <= BLOCK && T * QB <= T * T * SA && T * QC <= T * T * SA, "one line per lane, one buffer for the three layouts");
  __shared__ float lds[T * T * SA];   // R = 4: 17 408 bytes
  const int      tid = (int)threadIdx.x;
  const unsigned bx = blockIdx.x % bricks_x, by = (blockIdx.x / bricks_x) % bricks_y, bz = blockIdx.x / (bricks_x * bricks_y);
  const int      x0 = g.lo_x + 8 * (int)bx, y0 = g.lo_y + 8 * (int)by, z0 = g.lo_z + 8 * (int)bz;   // the brick's corner in the volume
  float w[R + 1];
#pragma unroll
  for (int i = 0; i <= R; i++) w[i] = record->p[i];   // uniform: scalar registers

  for (int l = tid; l < T * T * T; l += BLOCK) {
    const int    tx = l % T, line = l / T, ty = line % T, tz = line / T;
    const size_t gx = (size_t)vpt_filter_clamp(x0 + tx - R, g.w), gy = (size_t)vpt_filter_clamp(y0 + ty - R, g.h), gz = (size_t)vpt_filter_clamp(z0 + tz - R, g.d);
    lds[line * SA + tx] = grid[gx + gy * (size_t)g.w + gz * (size_t)g.w * (size_t)g.h];
  }
  __syncthreads();

  float in[T], out[8];
  if (tid < T * T) {
#pragma unroll
    for (int t = 0; t < T; t++) in[t] = lds[tid * SA + t];
#pragma unroll
    for (int o = 0; o < 8; o++) out[o] = vpt_filter_blur_taps<R>(w, in, o + R);
  }
  __syncthreads();
  if (tid < T * T) {
    const int ty = tid % T, tz = tid / T;
#pragma unroll
    for (int o = 0; o < 8; o++) lds[ty * QB + o + 8 * tz] = out[o];
  }
  __syncthreads();

  if (tid < 8 * T) {
#pragma unroll
    for (int t = 0; t < T; t++) in[t] = lds[t * QB + tid];
#pragma unroll
    for (int o = 0; o < 8; o++) out[o] = vpt_filter_blur_taps<R>(w, in, o + R);
  }
  __syncthreads();
  if (tid < 8 * T) {
    const int xo = tid % 8, tz = tid / 8;
#pragma unroll
    for (int o = 0; o < 8; o++) lds[tz * QC + xo + 8 * o] = out[o];
  }
  __syncthreads();

  if (tid < 64) {
#pragma unroll
    for (int t = 0; t < T; t++) in[t] = lds[t * QC + tid];
    const int x = 8 * (int)bx + tid % 8, y = 8 * (int)by + tid / 8;   // in the region
    if (x < g.rw && y < g.rh) {
#pragma unroll
      for (int o = 0; o < 8; o++) {
        const int z = 8 * (int)bz + o;
        if (z < g.rd) scratch[(size_t)x + (size_t)y * (size_t)g.rw + (size_t)z * (size_t)g.rw * (size_t)g.rh] = vpt_filter_blur_taps<R>(w, in, o + R);
      }
    }
  }
}

// a blur's results from the scratch (region order) into their place: one lane per voxel of the region
__global__ __launch_bounds__(BLOCK) void filter_place_kernel(float* __restrict__ grid, const float* __restrict__ scratch, filter_grid g, unsigned n) {
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  int i, j, k;
  grid[place_of(g, idx, i, j, k)] = scratch[idx];
}

int validate_edit(const DScene& d, const edit_mirrors& m, const vpt_filter_edit& e) {
  REQUIRE(e.num_entries >= 0 && (e.num_entries == 0 || e.entries), "filter: the entry list is null or has a negative count");
  REQUIRE(e.num_ops >= 0 && (e.num_ops == 0 || e.ops), "filter: the op list is null or has a negative count");
  for (int i = 0; i < e.num_ops; i++)
    if (const char* fault = vpt_filter_op_fault(e.ops[i])) return vpt_set_error(VPT_ERR_INVALID_ARG, "filter: op %d: %s", i, fault);
  for (int i = 0; i < e.num_entries; i++) {
    const vpt_filter_entry& en = e.entries[i];
    REQUIRE(en.volume >= 0 && en.volume < d.num_volumes, "filter: entry %d: volume %d out of range (%d)", i, en.volume, d.num_volumes);
    bool unsupported;
    if (const char* fault = vpt_filter_entry_fault(en, m.volumes[(size_t)en.volume].whd, e.ops, e.num_ops, &unsupported))
      return vpt_set_error(unsupported ? VPT_ERR_UNSUPPORTED : VPT_ERR_INVALID_ARG, "filter: entry %d: %s", i, fault);
  }
  return VPT_OK;
}

long long region_voxels(const vpt_filter_entry& en) { return (long long)en.region_whd[0] * en.region_whd[1] * en.region_whd[2]; }
bool      has_work(const vpt_filter_entry& en) { return region_voxels(en) > 0 && en.num_ops > 0; }

int launch_blur(resident& r, const float* grid, const filter_grid& g, const vpt_filter_record* record, int radius) {
  const unsigned nbx = (unsigned)(g.rw + 7) / 8, nby = (unsigned)(g.rh + 7) / 8, nbz = (unsigned)(g.rd + 7) / 8;   // <= 2^27 bricks in all
  const dim3     blocks(nbx * nby * nbz), lanes(BLOCK);
  float*         scratch = r.d_filter_scratch.get<float>();
  switch (radius) {
    case 1: hipLaunchKernelGGL(filter_blur_kernel<1>, blocks, lanes, 0, 0, grid, scratch, g, nbx, nby, record); break;
    case 2: hipLaunchKernelGGL(filter_blur_kernel<2>, blocks, lanes, 0, 0, grid, scratch, g, nbx, nby, record); break;
    case 3: hipLaunchKernelGGL(filter_blur_kernel<3>, blocks, lanes, 0, 0, grid, scratch, g, nbx, nby, record); break;
    default: hipLaunchKernelGGL(filter_blur_kernel<4>, blocks, lanes, 0, 0, grid, scratch, g, nbx, nby, record); break;   // validation leaves no other radius
  }
  LAUNCHED(r);
  return VPT_OK;
}

}  // namespace

int filter_apply(resident& r, const vpt_filter_edit& e, edit_outcome& out) {
  DScene& d = r.d;
  if (int rc = validate_edit(d, r.m, e)) return rc;
  out.changed = true;   // (an edit without entries too: it starts the counters again)
  if (int rc = begin_update(r)) return rc;
  bool   any = false;
  size_t scratch_bytes = 0;   // the largest blurred region
  for (int i = 0; i < e.num_entries; i++) {
    const vpt_filter_entry& en = e.entries[i];
    if (!has_work(en)) continue;
    any = true;
    for (int s = en.first_op; s < en.first_op + en.num_ops; s++)
      if (e.ops[s].type == VPT_FILTER_BLUR) scratch_bytes = std::max(scratch_bytes, (size_t)region_voxels(en) * sizeof(float));
  }
  device_buffer records;   // gone when the call returns (it ends with the device idle)
  if (any) {
    std::vector<vpt_filter_record> host((size_t)e.num_ops);
    for (int i = 0; i < e.num_ops; i++) host[(size_t)i] = vpt_filter_make_record(e.ops[i]);
    if (int rc = send(r, records, host)) return rc;
  }
  if (scratch_bytes > r.filter_scratch_bytes) {
    if (int rc = r.d_filter_scratch.allocate(scratch_bytes)) return r.filter_scratch_bytes = 0, rc;
    r.filter_scratch_bytes = scratch_bytes;
  }
  HIP_TRY(hipEventRecord(r.upd_ev0, 0));
  for (int i = 0; i < e.num_entries; i++) {
    const vpt_filter_entry& en = e.entries[i];
    if (!has_work(en)) continue;
    const long long   n = region_voxels(en);
    const vpt_volume& v = r.m.volumes[(size_t)en.volume];
    const filter_grid g = {v.whd[0], v.whd[1], v.whd[2], en.region_lo[0], en.region_lo[1], en.region_lo[2], en.region_whd[0], en.region_whd[1], en.region_whd[2],
        {en.origin[0], en.origin[1], en.origin[2]}, {en.step[0], en.step[1], en.step[2]}};
    float*                   grid = mut(d.voxels) + v.offset;
    const vpt_filter_record* recs = records.get<const vpt_filter_record>();
    for (int s = en.first_op, end = en.first_op + en.num_ops; s < end;) {
      if (e.ops[s].type == VPT_FILTER_BLUR) {
        if (int rc = launch_blur(r, grid, g, recs + s, e.ops[s].count)) return rc;
        LAUNCH(r, filter_place_kernel, n, grid, r.d_filter_scratch.get<const float>(), g, (unsigned)n);
        s++;
      } else {
        int run = 1;   // the pointwise ops up to the next BLUR: one launch
        while (s + run < end && e.ops[s + run].type != VPT_FILTER_BLUR) run++;
        LAUNCH(r, filter_pointwise_kernel, n, grid, g, (unsigned)n, recs + s, run);
        s += run;
      }
    }
  }
  if (int rc = mark_end(r)) return rc;
  return finish_update(r);
}
