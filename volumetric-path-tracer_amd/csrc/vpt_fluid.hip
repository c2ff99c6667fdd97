// vpt_fluid.hip — smoke that moves: one step of Stam's Stable Fluids over four volumes of a resident scene, a density and the three
// components of a velocity (include/vpt.h: vpt_scene_fluid_step).  The arithmetic is csrc/vpt_fluid_rule.h's, which the
// host mirror (host/vpt_fluid.cpp) compiles too: this unit is built with -ffp-contract=off like it.  Here: the validation of a step and six
// kernels - force + walls, the advection into scratch, its move into place + walls, the divergence, the temporally blocked Jacobi sweep
// of one 8 x 8 x 8 tile per workgroup through LDS, and project + walls.
#include <cstdlib>

#include "vpt_error.h"
#include "vpt_fluid.h"
#include "vpt_fluid_rule.h"
#include "vpt_update_helpers.h"

namespace {

struct fluid_fields {
  float* f[4];   // density, u, v, w: four volumes of the pool, or the four fields of the scratch
};

// node idx (x fastest) of the volume
__device__ inline void node_of(const vpt_fluid_record& g, unsigned idx, int& i, int& j, int& k) {
  i = (int)(idx % (unsigned)g.w), j = (int)((idx / (unsigned)g.w) % (unsigned)g.h), k = (int)(idx / ((unsigned)g.w * (unsigned)g.h));
}

// Stages 1 and 2.  One lane per node (n <= 2^30 of them, x fastest: a wave's loads and stores are consecutive words of each field); the
// step's record is a kernel argument, so its words sit in scalar registers.
__global__ __launch_bounds__(BLOCK) void fluid_force_kernel(fluid_fields f, vpt_fluid_record g, unsigned n) {
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  int i, j, k;
  node_of(g, idx, i, j, k);
  const float rho = f.f[0][idx];
  f.f[1][idx] = vpt_fluid_wall(vpt_fluid_force(f.f[1][idx], g.keep_velocity, g.force[0], rho), i, g.w, g.open, 0);
  f.f[2][idx] = vpt_fluid_wall(vpt_fluid_force(f.f[2][idx], g.keep_velocity, g.force[1], rho), j, g.h, g.open, 1);
  f.f[3][idx] = vpt_fluid_wall(vpt_fluid_force(f.f[3][idx], g.keep_velocity, g.force[2], rho), k, g.d, g.open, 2);
  f.f[0][idx] = vpt_fluid_decay(rho, g.keep_density);
}

// Stage 3.  One lane per node: one back-trace, then four trilerps at the same point from plain loads (the gather address depends on the
// data; staging an eight-corner read in LDS was slower than plain loads in vpt_sdf_mesh.hip).  The fields are only read here and the
// results go to the scratch: every workgroup sees the state before the advection.
__global__ __launch_bounds__(BLOCK) void fluid_advect_kernel(fluid_fields f, fluid_fields out, vpt_fluid_record g, unsigned n) {
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  int i, j, k;
  node_of(g, idx, i, j, k);
  const float qx = vpt_fluid_backtrace(i, g.dt, f.f[1][idx], g.w), qy = vpt_fluid_backtrace(j, g.dt, f.f[2][idx], g.h), qz = vpt_fluid_backtrace(k, g.dt, f.f[3][idx], g.d);
#pragma unroll
  for (int c = 0; c < 4; c++) out.f[c][idx] = vpt_fluid_advect(f.f[c], g.w, g.h, g.d, qx, qy, qz);
}

// The scratch becomes the fields, and stage 4
__global__ __launch_bounds__(BLOCK) void fluid_place_kernel(fluid_fields f, fluid_fields from, vpt_fluid_record g, unsigned n) {
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  int i, j, k;
  node_of(g, idx, i, j, k);
  f.f[0][idx] = from.f[0][idx];
  f.f[1][idx] = vpt_fluid_wall(from.f[1][idx], i, g.w, g.open, 0);
  f.f[2][idx] = vpt_fluid_wall(from.f[2][idx], j, g.h, g.open, 1);
  f.f[3][idx] = vpt_fluid_wall(from.f[3][idx], k, g.d, g.open, 2);
}

// Stage 5, and the pressure's start: p = 0 (a store here, not a memset on the stream)
__global__ __launch_bounds__(BLOCK) void fluid_divergence_kernel(fluid_fields f, float* __restrict__ div, float* __restrict__ p, vpt_fluid_record g, unsigned n) {
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  int i, j, k;
  node_of(g, idx, i, j, k);
  const int   at = (int)idx, sy = g.w, sz = g.w * g.h;
  const float du = f.f[1][at + (vpt_filter_clamp(i + 1, g.w) - i)] - f.f[1][at + (vpt_filter_clamp(i - 1, g.w) - i)];
  const float dv = f.f[2][at + (vpt_filter_clamp(j + 1, g.h) - j) * sy] - f.f[2][at + (vpt_filter_clamp(j - 1, g.h) - j) * sy];
  const float dw = f.f[3][at + (vpt_filter_clamp(k + 1, g.d) - k) * sz] - f.f[3][at + (vpt_filter_clamp(k - 1, g.d) - k) * sz];
  div[idx] = vpt_fluid_divergence(du, dv, dw);
  p[idx]   = 0.0f;
}

// Stage 6, K sweeps a launch: a temporally blocked Jacobi.  A workgroup makes one 8 x 8 x 8 tile of p after K sweeps; T = 8 + 2K.
//  1. Stage.  The T^3 nodes of p around the tile and the (T - 2)^3 nodes of d every sweep reads, into LDS: consecutive lanes read
//     consecutive x of a row.  A position outside the volume is NOT a node: it is staged as 0 and never read or computed below.
//  2. Sweep s = 1 .. K makes the positions [s, T - s)^3 from buffer (s - 1) & 1 into buffer s & 1; the last sweep's 8^3 go straight to
//     HBM.  A sweep depends on one node all round, so what sweep s reads, [s - 1, T - s + 1)^3, is what sweep s - 1 made (or the staged
//     tile): K sweeps here are K global sweeps bit for bit, PROVIDED a position inside the volume takes its neighbours as the volume
//     does - vpt_fluid_jacobi decides "across a face" on the node's VOLUME coordinates and then reads p[at] itself (closed) or nothing
//     (open), so a position outside the volume is never a source.  Staging clamped loads and sweeping the halo as interior would be
//     wrong from the second sweep on: the clamped copies would evolve with the interior's stencil.
// LDS layout: p dense, position (tx, ty, tz) at l = tx + T (ty + T tz), no padding.  A lane's work items are l = base + tid + 256 m over
// whole z-slabs of the sweep's region, so the 32 lanes of a group read 32 consecutive words for the centre and for each of the six
// neighbours (l -+ 1, l -+ T, l -+ T^2 shift all lanes alike): every LDS read of the sweep is free of bank conflicts without a padded
// stride, at the price of masking the lanes on the slab's rim ((T - 2s)^2 of T^2 work).  d dense at (T - 2)^3: the active lanes of a group
// map to strictly increasing words less than 32 apart, free of conflicts too.
template <int K>
__global__ __launch_bounds__(BLOCK) void fluid_jacobi_kernel(const float* __restrict__ p_in, float* __restrict__ p_out, const float* __restrict__ div, vpt_fluid_record g,
    unsigned tiles_x, unsigned tiles_y) {
  constexpr int T = 8 + 2 * K, TD = T - 2, PLANE = T * T, CELLS = T * T * T;
  __shared__ float pbuf[(K > 1 ? 2 : 1) * CELLS];   // K = 4: 2 x 16^3 + 14^3 floats, 43 744 bytes
  __shared__ float dbuf[TD * TD * TD];
  const int      tid = (int)threadIdx.x;
  const unsigned bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, bz = blockIdx.x / (tiles_x * tiles_y);
  const int      x0 = 8 * (int)bx - K, y0 = 8 * (int)by - K, z0 = 8 * (int)bz - K;   // tile position 0 in the volume

  for (int l = tid; l < CELLS; l += BLOCK) {
    const int  tx = l % T, ty = (l / T) % T, tz = l / PLANE;
    const int  gx = x0 + tx, gy = y0 + ty, gz = z0 + tz;
    const bool node = gx >= 0 && gx < g.w && gy >= 0 && gy < g.h && gz >= 0 && gz < g.d;
    const int  at = node ? gx + g.w * (gy + g.h * gz) : 0;
    pbuf[l] = node ? p_in[at] : 0.0f;
    if (tx >= 1 && tx < T - 1 && ty >= 1 && ty < T - 1 && tz >= 1 && tz < T - 1) dbuf[(tx - 1) + TD * ((ty - 1) + TD * (tz - 1))] = node ? div[at] : 0.0f;
  }
  __syncthreads();

#pragma unroll
  for (int s = 1; s <= K; s++) {
    const float* src = pbuf + ((s - 1) & 1) * CELLS;
    float*       dst = pbuf + (s & 1) * (K > 1 ? CELLS : 0);
    for (int l = s * PLANE + tid; l < (T - s) * PLANE; l += BLOCK) {
      const int tx = l % T, ty = (l / T) % T, tz = l / PLANE;
      const int gx = x0 + tx, gy = y0 + ty, gz = z0 + tz;
      if (tx < s || tx >= T - s || ty < s || ty >= T - s || gx < 0 || gx >= g.w || gy < 0 || gy >= g.h || gz < 0 || gz >= g.d) continue;
      const float r = vpt_fluid_jacobi(src, l, 1, T, PLANE, gx, gy, gz, g, dbuf[(tx - 1) + TD * ((ty - 1) + TD * (tz - 1))]);
      if (s == K) p_out[gx + g.w * (gy + g.h * gz)] = r;
      else dst[l] = r;
    }
    if (s < K) __syncthreads();
  }
}

// Stage 7 and the walls after it: p is only read, a velocity component only at its own node
__global__ __launch_bounds__(BLOCK) void fluid_project_kernel(fluid_fields f, const float* __restrict__ p, vpt_fluid_record g, unsigned n) {
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  int i, j, k;
  node_of(g, idx, i, j, k);
  const int at = (int)idx;
  f.f[1][idx] = vpt_fluid_wall(vpt_fluid_project(f.f[1][idx], p, at, 1, i, g.w, g.open, 0), i, g.w, g.open, 0);
  f.f[2][idx] = vpt_fluid_wall(vpt_fluid_project(f.f[2][idx], p, at, g.w, j, g.h, g.open, 1), j, g.h, g.open, 1);
  f.f[3][idx] = vpt_fluid_wall(vpt_fluid_project(f.f[3][idx], p, at, g.w * g.h, k, g.d, g.open, 2), k, g.d, g.open, 2);
}

int validate_step(const DScene& d, const edit_mirrors& m, const vpt_fluid_step& s) {
  bool unsupported;
  if (const char* fault = vpt_fluid_step_fault(s, d.num_volumes, [&](int id) { return m.volumes[(size_t)id].whd; }, &unsupported))
    return vpt_set_error(unsupported ? VPT_ERR_UNSUPPORTED : VPT_ERR_INVALID_ARG, "fluid: %s", fault);
  return VPT_OK;
}

// sweeps per Jacobi launch: VPT_FLUID_BLOCK = 1 | 2 | 4 forces it; the default is what won on the measured grids
constexpr int DEFAULT_BLOCK = 2;   // 2 beat 1 by 8 % at 96^3 and 6 % at 256^3, 4 took twice as long (profiles/fluid_measure.json)
int jacobi_block() {
  const char* e = getenv("VPT_FLUID_BLOCK");
  if (e && (e[0] == '1' || e[0] == '2' || e[0] == '4') && !e[1]) return e[0] - '0';
  return DEFAULT_BLOCK;
}

int launch_jacobi(resident& r, int sweeps, const float* from, float* to, const float* div, const vpt_fluid_record& g) {
  const unsigned nbx = (unsigned)(g.w + 7) / 8, nby = (unsigned)(g.h + 7) / 8, nbz = (unsigned)(g.d + 7) / 8;   // <= 2^30 tiles in all
  const dim3     blocks(nbx * nby * nbz), lanes(BLOCK);
  switch (sweeps) {
    case 1: hipLaunchKernelGGL(fluid_jacobi_kernel<1>, blocks, lanes, 0, 0, from, to, div, g, nbx, nby); break;
    case 2: hipLaunchKernelGGL(fluid_jacobi_kernel<2>, blocks, lanes, 0, 0, from, to, div, g, nbx, nby); break;
    default: hipLaunchKernelGGL(fluid_jacobi_kernel<4>, blocks, lanes, 0, 0, from, to, div, g, nbx, nby); break;   // jacobi_block leaves no other
  }
  LAUNCHED(r);
  return VPT_OK;
}

}  // namespace

int fluid_apply(resident& r, const vpt_fluid_step& s, edit_outcome& out) {
  DScene& d = r.d;
  if (int rc = validate_step(d, r.m, s)) return rc;
  out.changed = true;   // (a step that launches nothing too: it starts the counters again)
  if (int rc = begin_update(r)) return rc;
  const vpt_volume&      rho = r.m.volumes[(size_t)s.density];
  const vpt_fluid_record g   = vpt_fluid_make_record(rho.whd, s);
  const long long        n   = (long long)g.w * g.h * g.d;
  const bool             any = s.steps > 0 && n > 0;
  if (any && 4 * (size_t)n * sizeof(float) > r.fluid_scratch_bytes) {
    if (int rc = r.d_fluid_scratch.allocate(4 * (size_t)n * sizeof(float))) return r.fluid_scratch_bytes = 0, rc;
    r.fluid_scratch_bytes = 4 * (size_t)n * sizeof(float);
  }
  HIP_TRY(hipEventRecord(r.upd_ev0, 0));
  if (any) {
    r.last_bytes += (long long)sizeof(vpt_fluid_record);   // the step, in the kernels' argument block
    float* const       pool = mut(d.voxels);
    const fluid_fields f    = {{pool + rho.offset, pool + r.m.volumes[(size_t)s.velocity[0]].offset, pool + r.m.volumes[(size_t)s.velocity[1]].offset,
        pool + r.m.volumes[(size_t)s.velocity[2]].offset}};
    float* const       sc   = r.d_fluid_scratch.get<float>();
    const fluid_fields scratch = {{sc, sc + n, sc + 2 * n, sc + 3 * n}};
    float *div = sc, *p = sc + n, *q = sc + 2 * n;   // once the advected fields are in place the scratch is free: d and the two p
    const int block = jacobi_block();
    for (int step = 0; step < s.steps; step++) {
      LAUNCH(r, fluid_force_kernel, n, f, g, (unsigned)n);
      LAUNCH(r, fluid_advect_kernel, n, f, scratch, g, (unsigned)n);
      LAUNCH(r, fluid_place_kernel, n, f, scratch, g, (unsigned)n);
      LAUNCH(r, fluid_divergence_kernel, n, f, div, p, g, (unsigned)n);
      for (int left = s.iterations, k = block; left > 0;) {   // iterations / block launches of `block` sweeps, the remainder at smaller K
        while (k > left) k /= 2;
        if (int rc = launch_jacobi(r, k, p, q, div, g)) return rc;
        std::swap(p, q);
        left -= k;
      }
      LAUNCH(r, fluid_project_kernel, n, f, (const float*)p, g, (unsigned)n);
    }
  }
  if (int rc = mark_end(r)) return rc;
  return finish_update(r);
}
