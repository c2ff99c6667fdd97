// vpt_fluid.hip — smoke that moves: one step of Stam's Stable Fluids over four volumes of a resident scene, a density and the three
// components of a velocity (include/vpt.h: vpt_scene_fluid_step).  The arithmetic is csrc/vpt_fluid_rule.h's, which the
// host mirror (host/vpt_fluid.cpp) compiles too: this unit is built with -ffp-contract=off like it.  Here: the validation of a step and six
// kernels - force + walls, the advection into scratch, its move into place + walls, the divergence, the temporally blocked Jacobi sweep
// of one 8 x 8 x 8 tile per workgroup through LDS, and project + walls - and, for vpt_scene_fluid_step_solver, the three kernels of a
// multigrid V-cycle in the Jacobi's place: a temporally blocked red-black smoother that prolongs as it stages, the residual and its
// restriction in one launch, and the coarsest level in one workgroup.  For vpt_scene_fluid_step_detail two more: the
// vorticity confinement, a two-level stencil of one 8 x 8 x 8 tile through LDS that applies the force as it stages, and the second pass
// of the MacCormack advection.
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

// ---- stage 6 by multigrid (include/vpt.h: vpt_scene_fluid_step_solver) -----------------------------------------------------
// A tile of a level in LDS, laid out BY COLOUR: the positions of one colour of a T^3 tile are a dense (T / 2) x T x T array (x halved: in a
// row the positions of a colour have one parity of tx), the other colour's lie MG_HALF words on.  A red-black half-sweep writes one
// colour and reads only the other, so one buffer serves in place; and a lane that owns position (tx, ty, tz) of the colour written finds
// its neighbours along y and z at tx >> 1 of the rows beside it and those along x at (tx - 1) >> 1 and (tx + 1) >> 1 of its own row: lanes
// with consecutive m read consecutive words for all six, as they would in a dense array of a plain stencil - the checkerboard costs no
// stride of two.  par: the parity of the tile's position 0 in the level, so that the colour is the level's, (I + J + K) & 1.
constexpr int MG_PAD = 32;   // between the halves: the two colours of a staged row start half the banks apart
template <int T> struct mg_tile {
  static constexpr int ROW = T / 2, HALF = T * T * T / 2 + MG_PAD;
  __device__ static int word(int tx, int ty, int tz, int par) { return ((tx + ty + tz + par) & 1) * HALF + (tx >> 1) + ROW * (ty + T * tz); }
};

// H half-sweeps a launch of the red-black Gauss-Seidel, colours first, first ^ 1, first, ...: a workgroup makes one 8^3 tile of p after
// them; T = 8 + 2H.  The argument of the blocked Jacobi above, for a region that shrinks by one node per HALF-sweep: half-sweep s makes
// the nodes of its colour in [s, T - s)^3; it reads the other colour in [s - 1, T - s + 1)^3, which half-sweep s - 1 made (or the staging
// left, for s = 1), and keeps its own colour where D == 0, which half-sweep s - 2 made in a larger region still.  So the 8^3 centre holds
// what H global half-sweeps leave, bit for bit, PROVIDED a position outside the level is no node: it is staged as 0, never computed and,
// since vpt_fluid_mg_sums decides `inside` on the node's LEVEL coordinates, never read.
//  1. Stage p and s_l * b (the product of every half-sweep, made once) of the T^3 positions.  With `coarse` the staged p is the
//     prolongation, p_in + coarse[parent]: the V-cycle's way up is this kernel's staging, not a launch.
//  2. Half-sweep s: an item is (m, y, z) of the region's colour-written positions, tx = s + 2m + q with q the parity that gives the row
//     its colour, so EVERY lane of a pass owns a node of the colour - not every other one.
//  3. The 8^3 centre goes to p_out: p_in's other tiles are still being staged by other workgroups, so HBM is ping-pong.
template <int H>
__global__ __launch_bounds__(BLOCK) void fluid_mg_smooth_kernel(const float* __restrict__ p_in, float* __restrict__ p_out, const float* __restrict__ b,
    const float* __restrict__ coarse, vpt_fluid_mg_level g, int first, unsigned tiles_x, unsigned tiles_y) {
  constexpr int T = 8 + 2 * H, CELLS = T * T * T, ROW = mg_tile<T>::ROW, HALF = mg_tile<T>::HALF;
  __shared__ float pbuf[2 * HALF];   // H = 4: 2 x (2048 + 32) floats, and as many of s_l * b: 33 280 bytes in all
  __shared__ float sbuf[2 * HALF];
  const int      tid = (int)threadIdx.x;
  const unsigned bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, bz = blockIdx.x / (tiles_x * tiles_y);
  const int      x0 = 8 * (int)bx - H, y0 = 8 * (int)by - H, z0 = 8 * (int)bz - H;   // tile position 0 in the level
  const int      par = (x0 + y0 + z0) & 1;
  const int      cw = (g.w + 1) / 2, ch = (g.h + 1) / 2;   // the coarser level's, for the parent

  for (int l = tid; l < CELLS; l += BLOCK) {
    const int  tx = l % T, ty = (l / T) % T, tz = l / (T * T);
    const int  gx = x0 + tx, gy = y0 + ty, gz = z0 + tz;
    const bool node = gx >= 0 && gx < g.w && gy >= 0 && gy < g.h && gz >= 0 && gz < g.d;
    float      v = 0.0f, sb = 0.0f;
    if (node) {
      const int at = gx + g.w * (gy + g.h * gz);
      v = p_in[at];
      if (coarse) v = vpt_fluid_mg_correct(v, coarse[(gx >> 1) + cw * ((gy >> 1) + ch * (gz >> 1))]);
      sb = vpt_fluid_mg_scaled(g, b[at]);
    }
    const int word = mg_tile<T>::word(tx, ty, tz, par);
    pbuf[word] = v, sbuf[word] = sb;
  }
  __syncthreads();

#pragma unroll
  for (int s = 1; s <= H; s++) {
    const int R = T - 2 * s, HR = R / 2;   // the region's side; the nodes of one colour in a row of it
    const int colour = first ^ ((s - 1) & 1);
    for (int item = tid; item < HR * R * R; item += BLOCK) {
      const int m = item % HR, ty = s + (item / HR) % R, tz = s + item / (HR * R);
      const int tx = s + 2 * m + ((colour + s + ty + tz + par) & 1);
      const int gx = x0 + tx, gy = y0 + ty, gz = z0 + tz;
      if (gx < 0 || gx >= g.w || gy < 0 || gy >= g.h || gz < 0 || gz >= g.d) continue;
      const int row = ROW * (ty + T * tz), own = colour * HALF + row + (tx >> 1), other = (colour ^ 1) * HALF + row;
      const int near[6] = {other + ((tx - 1) >> 1), other + ((tx + 1) >> 1), other + (tx >> 1) - ROW, other + (tx >> 1) + ROW, other + (tx >> 1) - ROW * T,
          other + (tx >> 1) + ROW * T};
      float S, D;
      vpt_fluid_mg_sums(pbuf, near, gx, gy, gz, g, S, D);
      pbuf[own] = vpt_fluid_mg_relax(S, D, sbuf[own], pbuf[own]);
    }
    __syncthreads();
  }

  for (int l = tid; l < 512; l += BLOCK) {
    const int tx = H + (l & 7), ty = H + ((l >> 3) & 7), tz = H + (l >> 6);
    const int gx = x0 + tx, gy = y0 + ty, gz = z0 + tz;
    if (gx < g.w && gy < g.h && gz < g.d) p_out[gx + g.w * (gy + g.h * gz)] = pbuf[mg_tile<T>::word(tx, ty, tz, par)];
  }
}

// The way down in one launch: a workgroup stages an 8^3 tile of p with a halo of 1 (10^3, dense), makes the residual of its 512 nodes
// into LDS, and 64 of its lanes sum the up to eight children of a coarse node each, in the rule's order, into the coarser level's
// right-hand side - and store that level's p = 0 beside it (a store, not a memset on the stream).  A position outside the level is no
// node: no residual, no child.
__global__ __launch_bounds__(BLOCK) void fluid_mg_restrict_kernel(const float* __restrict__ p, const float* __restrict__ b, float* __restrict__ b_coarse,
    float* __restrict__ p_coarse, vpt_fluid_mg_level g, unsigned tiles_x, unsigned tiles_y) {
  constexpr int T = 10, PLANE = T * T, CELLS = T * T * T;
  __shared__ float pbuf[CELLS];
  __shared__ float rbuf[512];
  const int      tid = (int)threadIdx.x;
  const unsigned bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, bz = blockIdx.x / (tiles_x * tiles_y);
  const int      x0 = 8 * (int)bx - 1, y0 = 8 * (int)by - 1, z0 = 8 * (int)bz - 1;

  for (int l = tid; l < CELLS; l += BLOCK) {
    const int  gx = x0 + l % T, gy = y0 + (l / T) % T, gz = z0 + l / PLANE;
    const bool node = gx >= 0 && gx < g.w && gy >= 0 && gy < g.h && gz >= 0 && gz < g.d;
    pbuf[l] = node ? p[gx + g.w * (gy + g.h * gz)] : 0.0f;
  }
  __syncthreads();
  for (int l = tid; l < 512; l += BLOCK) {
    const int tx = 1 + (l & 7), ty = 1 + ((l >> 3) & 7), tz = 1 + (l >> 6);
    const int gx = x0 + tx, gy = y0 + ty, gz = z0 + tz;
    float     res = 0.0f;
    if (gx < g.w && gy < g.h && gz < g.d) {
      const int c = tx + T * (ty + T * tz);
      const int near[6] = {c - 1, c + 1, c - T, c + T, c - PLANE, c + PLANE};
      float     S, D;
      vpt_fluid_mg_sums(pbuf, near, gx, gy, gz, g, S, D);
      res = vpt_fluid_mg_residual(S, D, pbuf[c], vpt_fluid_mg_b(g, b[gx + g.w * (gy + g.h * gz)]), g.s);
    }
    rbuf[l] = res;
  }
  __syncthreads();
  if (tid < 64) {
    const int cx = tid & 3, cy = (tid >> 2) & 3, cz = tid >> 4;
    const int I = 4 * (int)bx + cx, J = 4 * (int)by + cy, K = 4 * (int)bz + cz;
    const int cw = (g.w + 1) / 2, ch = (g.h + 1) / 2, cd = (g.d + 1) / 2;
    if (I < cw && J < ch && K < cd) {
      float sum = 0.0f;
      for (int c = 0; c < 2 && 2 * K + c < g.d; c++)
        for (int e = 0; e < 2 && 2 * J + e < g.h; e++)
          for (int a = 0; a < 2 && 2 * I + a < g.w; a++) sum = sum + rbuf[(2 * cx + a) + 8 * ((2 * cy + e) + 8 * (2 * cz + c))];
      b_coarse[I + cw * (J + ch * K)] = vpt_filter_one_nan(sum);
      p_coarse[I + cw * (J + ch * K)] = 0.0f;
    }
  }
}

// The coarsest level, at most 8^3 nodes, in ONE workgroup: p and s_l * b in LDS (dense, stride 8) for all `sweeps` pre-order sweeps, a
// lane per node of the colour written (x = 2m + ((y + z + colour) & 1), m = lane & 3), p read and written once.
__global__ __launch_bounds__(BLOCK) void fluid_mg_coarse_kernel(float* __restrict__ p, const float* __restrict__ b, vpt_fluid_mg_level g, int sweeps) {
  __shared__ float pbuf[512];
  __shared__ float sbuf[512];
  const int tid = (int)threadIdx.x;
  for (int l = tid; l < 512; l += BLOCK) {
    const int  x = l & 7, y = (l >> 3) & 7, z = l >> 6;
    const bool node = x < g.w && y < g.h && z < g.d;
    const int  at = node ? x + g.w * (y + g.h * z) : 0;
    pbuf[l] = node ? p[at] : 0.0f;
    sbuf[l] = node ? vpt_fluid_mg_scaled(g, b[at]) : 0.0f;
  }
  __syncthreads();
  const int m = tid & 3, y = (tid >> 2) & 7, z = tid >> 5;
  for (int n = 0; n < 2 * sweeps; n++) {
    const int x = 2 * m + ((y + z + n) & 1);   // colour n & 1
    if (x < g.w && y < g.h && z < g.d) {
      const int c = x + 8 * (y + 8 * z);
      const int near[6] = {c - 1, c + 1, c - 8, c + 8, c - 64, c + 64};
      float     S, D;
      vpt_fluid_mg_sums(pbuf, near, x, y, z, g, S, D);
      pbuf[c] = vpt_fluid_mg_relax(S, D, sbuf[c], pbuf[c]);
    }
    __syncthreads();
  }
  for (int l = tid; l < 512; l += BLOCK) {
    const int x = l & 7, y2 = (l >> 3) & 7, z2 = l >> 6;
    if (x < g.w && y2 < g.h && z2 < g.d) p[x + g.w * (y2 + g.h * z2)] = pbuf[l];
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

// ---- what vpt_scene_fluid_step_detail adds (include/vpt.h) -------------------------------------------------------------------
// Stage 2b, and with FORCE stages 1 and 2 before it in the same launch: a two-level stencil through LDS.  The new velocity at a node needs
// m = |omega| at its six neighbours and omega needs the velocity at theirs, so a workgroup that makes one 8 x 8 x 8 tile reads the
// velocity of the 12^3 positions around it (halo 2).
//  1. Stage the three components of the 12^3 positions.  With FORCE what is staged is wall(force(u, rho)) of the fields as the last step
//     left them - stages 1 and 2 per position, the way the multigrid's smoother prolongs while it stages - and this launch takes
//     fluid_force_kernel's place; the lanes of the 8^3 centre store the decayed density as they pass.  A position outside the volume is
//     NOT a node: it is staged as 0 and never computed or read below, since vpt_fluid_difference clamps on the node's VOLUME coordinates.
//  2. Phase A: m at the nodes of the 10^3 region, into LDS.  omega is NOT kept: 3 x 10^3 words more, for what phase B makes again from twelve
//     LDS reads of the staged tile.
//  3. Phase B: omega again at the nodes of the 8^3 centre, eta from m, N x omega, the new velocity and its walls.
// Other workgroups' halos still read `f`, so everything goes to `out`, the scratch: never in place.
// LDS layout: the components dense at l = tx + 12 (ty + 12 tz), no padding; a lane's items are l = base + tid + 256 n over whole z-slabs of
// a phase's region with the rim masked, as in fluid_jacobi_kernel: the 32 lanes of a group read consecutive words for every neighbour.  m
// dense at 10^3: the active lanes of a group map to strictly increasing words less than 32 apart.
template <bool FORCE>
__global__ __launch_bounds__(BLOCK) void fluid_confine_kernel(fluid_fields f, fluid_fields out, vpt_fluid_record g, float strength, unsigned tiles_x, unsigned tiles_y) {
  constexpr int T = 12, PLANE = T * T, CELLS = T * T * T, TM = T - 2;
  __shared__ float ubuf[3 * CELLS];   // 20 736 bytes, and 4 000 of m
  __shared__ float mbuf[TM * TM * TM];
  const int      tid = (int)threadIdx.x;
  const unsigned bx = blockIdx.x % tiles_x, by = (blockIdx.x / tiles_x) % tiles_y, bz = blockIdx.x / (tiles_x * tiles_y);
  const int      x0 = 8 * (int)bx - 2, y0 = 8 * (int)by - 2, z0 = 8 * (int)bz - 2;   // tile position 0 in the volume
  const float *  ub = ubuf, *vb = ubuf + CELLS, *wb = ubuf + 2 * CELLS;

  for (int l = tid; l < CELLS; l += BLOCK) {
    const int  tx = l % T, ty = (l / T) % T, tz = l / PLANE;
    const int  gx = x0 + tx, gy = y0 + ty, gz = z0 + tz;
    const bool node = gx >= 0 && gx < g.w && gy >= 0 && gy < g.h && gz >= 0 && gz < g.d;
    float      u = 0.0f, v = 0.0f, w = 0.0f;
    if (node) {
      const int  at = gx + g.w * (gy + g.h * gz);
      const bool centre = tx >= 2 && tx < T - 2 && ty >= 2 && ty < T - 2 && tz >= 2 && tz < T - 2;
      u = f.f[1][at], v = f.f[2][at], w = f.f[3][at];
      if (FORCE) {
        const float rho = f.f[0][at];
        u = vpt_fluid_wall(vpt_fluid_force(u, g.keep_velocity, g.force[0], rho), gx, g.w, g.open, 0);
        v = vpt_fluid_wall(vpt_fluid_force(v, g.keep_velocity, g.force[1], rho), gy, g.h, g.open, 1);
        w = vpt_fluid_wall(vpt_fluid_force(w, g.keep_velocity, g.force[2], rho), gz, g.d, g.open, 2);
        if (centre) out.f[0][at] = vpt_fluid_decay(rho, g.keep_density);
      } else if (centre) {
        out.f[0][at] = f.f[0][at];
      }
    }
    ubuf[l] = u, ubuf[CELLS + l] = v, ubuf[2 * CELLS + l] = w;
  }
  __syncthreads();

  for (int l = PLANE + tid; l < (T - 1) * PLANE; l += BLOCK) {
    const int tx = l % T, ty = (l / T) % T, tz = l / PLANE;
    const int gx = x0 + tx, gy = y0 + ty, gz = z0 + tz;
    if (tx < 1 || tx >= T - 1 || ty < 1 || ty >= T - 1 || gx < 0 || gx >= g.w || gy < 0 || gy >= g.h || gz < 0 || gz >= g.d) continue;
    float omega[3];
    vpt_fluid_curl(ub, vb, wb, l, 1, T, PLANE, gx, gy, gz, g, omega);
    mbuf[(tx - 1) + TM * ((ty - 1) + TM * (tz - 1))] = vpt_fluid_length(omega);
  }
  __syncthreads();

  for (int l = 2 * PLANE + tid; l < (T - 2) * PLANE; l += BLOCK) {
    const int tx = l % T, ty = (l / T) % T, tz = l / PLANE;
    const int gx = x0 + tx, gy = y0 + ty, gz = z0 + tz;
    if (tx < 2 || tx >= T - 2 || ty < 2 || ty >= T - 2 || gx >= g.w || gy >= g.h || gz >= g.d) continue;   // (the centre starts inside the volume)
    float omega[3], force[3];
    vpt_fluid_curl(ub, vb, wb, l, 1, T, PLANE, gx, gy, gz, g, omega);
    const int ml = (tx - 1) + TM * ((ty - 1) + TM * (tz - 1));
    vpt_fluid_confinement(vpt_fluid_difference(mbuf, ml, 1, gx, g.w), vpt_fluid_difference(mbuf, ml, TM, gy, g.h), vpt_fluid_difference(mbuf, ml, TM * TM, gz, g.d), omega,
        force);
    const int at = gx + g.w * (gy + g.h * gz);
    out.f[1][at] = vpt_fluid_wall(vpt_fluid_confine(ub[l], strength, force[0]), gx, g.w, g.open, 0);
    out.f[2][at] = vpt_fluid_wall(vpt_fluid_confine(vb[l], strength, force[1]), gy, g.h, g.open, 1);
    out.f[3][at] = vpt_fluid_wall(vpt_fluid_confine(wb[l], strength, force[2]), gz, g.d, g.open, 2);
  }
}

// Stage 3's second pass with VPT_FLUID_MACCORMACK; the first is fluid_advect_kernel, which left `hat`.  One lane per node and plain
// loads, as there: one back-trace and one forward trace, then per field the eight corners of `f` at the back-trace - the first pass's,
// loaded again for their least and greatest, which gives the first pass's value too - the eight of `hat` at the forward trace, and the
// node's own.  f, hat and out are three different sets of buffers.
__global__ __launch_bounds__(BLOCK) void fluid_maccormack_kernel(fluid_fields f, fluid_fields hat, fluid_fields out, vpt_fluid_record g, unsigned n) {
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  int i, j, k;
  node_of(g, idx, i, j, k);
  const float u = f.f[1][idx], v = f.f[2][idx], w = f.f[3][idx];
  const float qx = vpt_fluid_backtrace(i, g.dt, u, g.w), qy = vpt_fluid_backtrace(j, g.dt, v, g.h), qz = vpt_fluid_backtrace(k, g.dt, w, g.d);
  const float rx = vpt_fluid_foretrace(i, g.dt, u, g.w), ry = vpt_fluid_foretrace(j, g.dt, v, g.h), rz = vpt_fluid_foretrace(k, g.dt, w, g.d);
#pragma unroll
  for (int c = 0; c < 4; c++) {
    float       lo, hi;
    const float first = vpt_fluid_advect_bounds(f.f[c], g.w, g.h, g.d, qx, qy, qz, lo, hi);
    const float bar   = vpt_volgrid_trilerp(hat.f[c], g.w, g.h, g.d, rx, ry, rz);
    out.f[c][idx] = vpt_fluid_maccormack(first, f.f[c][idx], bar, lo, hi);
  }
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

// half-sweeps per smoothing launch: VPT_FLUID_MG_BLOCK = 2 | 4 forces it
constexpr int DEFAULT_MG_BLOCK = 2;
int mg_block() {
  const char* e = getenv("VPT_FLUID_MG_BLOCK");
  if (e && (e[0] == '2' || e[0] == '4') && !e[1]) return e[0] - '0';
  return DEFAULT_MG_BLOCK;
}

// stages 1 and 2 in the confinement launch's staging unless VPT_FLUID_CONFINE_FUSED = 0 asks for fluid_force_kernel and a launch more
bool confine_fused() {
  const char* e = getenv("VPT_FLUID_CONFINE_FUSED");
  return !(e && e[0] == '0' && !e[1]);
}
int launch_confine(resident& r, bool fused, const fluid_fields& f, const fluid_fields& out, const vpt_fluid_record& g, float strength) {
  const unsigned nbx = (unsigned)(g.w + 7) / 8, nby = (unsigned)(g.h + 7) / 8, nbz = (unsigned)(g.d + 7) / 8;
  const dim3     blocks(nbx * nby * nbz), lanes(BLOCK);
  if (fused) hipLaunchKernelGGL(fluid_confine_kernel<true>, blocks, lanes, 0, 0, f, out, g, strength, nbx, nby);
  else hipLaunchKernelGGL(fluid_confine_kernel<false>, blocks, lanes, 0, 0, f, out, g, strength, nbx, nby);
  LAUNCHED(r);
  return VPT_OK;
}

struct mg_fields {
  float *p, *q, *b;   // a level's pressure, its ping-pong partner, its right-hand side (level 0: stage 5's d)
};
dim3 mg_tiles(const vpt_fluid_mg_level& g, unsigned& nbx, unsigned& nby) {
  nbx = (unsigned)(g.w + 7) / 8, nby = (unsigned)(g.h + 7) / 8;
  return dim3(nbx * nby * ((unsigned)(g.d + 7) / 8));   // <= 2^30 / 512 tiles and some
}
// `smooth` sweeps from colour `first`, `block` half-sweeps a launch and a remainder of two in one more; `coarse`: the prolongation first
int mg_smooth(resident& r, const vpt_fluid_mg_level& g, mg_fields& at, const float* coarse, int smooth, int first, int block) {
  unsigned   nbx, nby;
  const dim3 blocks = mg_tiles(g, nbx, nby), lanes(BLOCK);
  for (int left = 2 * smooth; left > 0; coarse = nullptr) {   // an even number of half-sweeps done: the next colour is `first` again
    const int h = left >= block ? block : 2;
    if (h == 4) hipLaunchKernelGGL(fluid_mg_smooth_kernel<4>, blocks, lanes, 0, 0, (const float*)at.p, at.q, (const float*)at.b, coarse, g, first, nbx, nby);
    else hipLaunchKernelGGL(fluid_mg_smooth_kernel<2>, blocks, lanes, 0, 0, (const float*)at.p, at.q, (const float*)at.b, coarse, g, first, nbx, nby);
    LAUNCHED(r);
    std::swap(at.p, at.q);
    left -= h;
  }
  return VPT_OK;
}
// one V-cycle over the levels' fields: down by pre-smoothing and restriction, the coarsest level, up by prolonging post-smoothing
int mg_cycle(resident& r, const vpt_fluid_mg_level* levels, int count, mg_fields* at, const vpt_fluid_solver& s, int block) {
  for (int l = 0; l + 1 < count; l++) {
    if (int rc = mg_smooth(r, levels[l], at[l], nullptr, s.smooth, 0, block)) return rc;
    unsigned   nbx, nby;
    const dim3 blocks = mg_tiles(levels[l], nbx, nby);
    hipLaunchKernelGGL(fluid_mg_restrict_kernel, blocks, dim3(BLOCK), 0, 0, (const float*)at[l].p, (const float*)at[l].b, at[l + 1].b, at[l + 1].p, levels[l], nbx, nby);
    LAUNCHED(r);
  }
  hipLaunchKernelGGL(fluid_mg_coarse_kernel, dim3(1), dim3(BLOCK), 0, 0, at[count - 1].p, (const float*)at[count - 1].b, levels[count - 1], s.coarse_sweeps);
  LAUNCHED(r);
  for (int l = count - 2; l >= 0; l--)
    if (int rc = mg_smooth(r, levels[l], at[l], (const float*)at[l + 1].p, s.smooth, 1, block)) return rc;
  return VPT_OK;
}

}  // namespace

int fluid_apply(resident& r, const vpt_fluid_step& s, const vpt_fluid_solver* solver, const vpt_fluid_detail* detail, edit_outcome& out) {
  DScene& d = r.d;
  if (int rc = validate_step(d, r.m, s)) return rc;
  if (const char* fault = vpt_fluid_solver_fault(solver)) return vpt_set_error(VPT_ERR_INVALID_ARG, "fluid: %s", fault);
  if (const char* fault = vpt_fluid_detail_fault(detail)) return vpt_set_error(VPT_ERR_INVALID_ARG, "fluid: %s", fault);
  out.changed = true;   // (a step that launches nothing too: it starts the counters again)
  if (int rc = begin_update(r)) return rc;
  const vpt_volume&      rho = r.m.volumes[(size_t)s.density];
  const vpt_fluid_record g   = vpt_fluid_make_record(rho.whd, s);
  const long long        n   = (long long)g.w * g.h * g.d;
  const bool             any = s.steps > 0 && n > 0;
  const bool             confines = vpt_fluid_confines(detail), maccormack = vpt_fluid_maccormacks(detail);
  const size_t           fields = maccormack ? 8 : 4;   // the second pass reads the fields, the first pass's and writes a third set
  if (any && fields * (size_t)n * sizeof(float) > r.fluid_scratch_bytes) {
    if (int rc = r.d_fluid_scratch.allocate(fields * (size_t)n * sizeof(float))) return r.fluid_scratch_bytes = 0, rc;
    r.fluid_scratch_bytes = fields * (size_t)n * sizeof(float);
  }
  // the multigrid's levels above 0: p, its partner and b of each, sized from the level's own whd (halves round up)
  vpt_fluid_mg_level levels[VPT_FLUID_MG_MAX_LEVELS];
  const int          count = any && vpt_fluid_multigrid(solver) ? vpt_fluid_mg_levels(g, levels) : 0;
  size_t             above = 0;
  for (int l = 1; l < count; l++) above += 3 * (size_t)levels[l].w * (size_t)levels[l].h * (size_t)levels[l].d * sizeof(float);
  if (above > r.fluid_mg_bytes) {
    if (int rc = r.d_fluid_mg.allocate(above)) return r.fluid_mg_bytes = 0, rc;
    r.fluid_mg_bytes = above;
  }
  HIP_TRY(hipEventRecord(r.upd_ev0, 0));
  if (any) {
    r.last_bytes += (long long)sizeof(vpt_fluid_record);   // the step, in the kernels' argument block
    if (confines || maccormack) r.last_bytes += (long long)sizeof(vpt_fluid_detail_record);
    const vpt_fluid_detail_record detailed = vpt_fluid_make_detail(s, detail);
    float* const       pool = mut(d.voxels);
    const fluid_fields f    = {{pool + rho.offset, pool + r.m.volumes[(size_t)s.velocity[0]].offset, pool + r.m.volumes[(size_t)s.velocity[1]].offset,
        pool + r.m.volumes[(size_t)s.velocity[2]].offset}};
    float* const       sc   = r.d_fluid_scratch.get<float>();
    const fluid_fields scratch = {{sc, sc + n, sc + 2 * n, sc + 3 * n}};
    const fluid_fields second  = {{sc + 4 * n, sc + 5 * n, sc + 6 * n, sc + 7 * n}};   // (with MacCormack only)
    const bool         fused   = confine_fused();
    float *div = sc, *p = sc + n, *q = sc + 2 * n;   // once the advected fields are in place the scratch is free: d and the two p
    const int block = jacobi_block(), half_sweeps = mg_block();
    mg_fields at[VPT_FLUID_MG_MAX_LEVELS];
    float*    next = r.d_fluid_mg.get<float>();
    for (int l = 1; l < count; l++) {
      const size_t nodes = (size_t)levels[l].w * (size_t)levels[l].h * (size_t)levels[l].d;
      at[l] = {next, next + nodes, next + 2 * nodes};
      next += 3 * nodes;
    }
    for (int step = 0; step < s.steps; step++) {
      if (!confines || !fused) LAUNCH(r, fluid_force_kernel, n, f, g, (unsigned)n);
      if (confines) {   // the fields after 2b are in the scratch: the advection goes from there back into the pool, and place runs in place
        if (int rc = launch_confine(r, fused, f, scratch, g, detailed.k)) return rc;
        if (maccormack) {
          LAUNCH(r, fluid_advect_kernel, n, scratch, second, g, (unsigned)n);
          LAUNCH(r, fluid_maccormack_kernel, n, scratch, second, f, g, (unsigned)n);
        } else {
          LAUNCH(r, fluid_advect_kernel, n, scratch, f, g, (unsigned)n);
        }
        LAUNCH(r, fluid_place_kernel, n, f, f, g, (unsigned)n);
      } else {
        LAUNCH(r, fluid_advect_kernel, n, f, scratch, g, (unsigned)n);
        if (maccormack) LAUNCH(r, fluid_maccormack_kernel, n, f, scratch, second, g, (unsigned)n);
        LAUNCH(r, fluid_place_kernel, n, f, maccormack ? second : scratch, g, (unsigned)n);
      }
      LAUNCH(r, fluid_divergence_kernel, n, f, div, p, g, (unsigned)n);
      if (count) {   // `cycles` V-cycles from the p = 0 the divergence launch stored; level 0 lives in the scratch
        at[0] = {p, q, div};
        for (int cycle = 0; cycle < solver->cycles; cycle++)
          if (int rc = mg_cycle(r, levels, count, at, *solver, half_sweeps)) return rc;
        p = at[0].p, q = at[0].q;
      }
      for (int left = count ? 0 : s.iterations, k = block; left > 0;) {   // iterations / block launches of `block` sweeps, the remainder at smaller K
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
