// vpt_fluid_rule.h — the rule of vpt_scene_fluid_step (include/vpt.h), written once: one step of Stam's Stable Fluids on a collocated node
// grid, stage by stage at one node.  Compiled by the fluid kernels (csrc/vpt_fluid.hip) and by the host mirror (host/vpt_fluid.cpp), both
// with -ffp-contract=off: float32 throughout, nothing fused, every sum in the order written here - so both give the same bits, and THIS
// FILE IS THE CONTRACT'S OPERATION ORDER.  Velocities are node spacings per unit time: there is no cell size.  A result that is a NaN is
// stored as 0x7fc00000 (vpt_filter_one_nan, csrc/vpt_filter_rule.h); the back-trace reads the grid through vpt_volgrid_trilerp, the
// function the renderer reads it with (csrc/vpt_volgrid_rule.h).
#pragma once
#include "vpt_filter_rule.h"
#include "vpt_volgrid_rule.h"

#define VPT_FLUID_HD VPT_FILTER_HD

// what the kernels get as an argument and the mirror reads: VPT_FLUID_RECORD_BYTES, made on the host by vpt_fluid_make_record
struct vpt_fluid_record {
  int32_t  w, h, d;
  uint32_t open;      // bit 0 .. 5: the faces -x, +x, -y, +y, -z, +z are open
  float    dt;
  float    force[3];  // dt * lift[c], one float32 product each
  float    keep_density, keep_velocity;
  int32_t  iterations, unused;
};
static_assert(sizeof(vpt_fluid_record) == VPT_FLUID_RECORD_BYTES, "include/vpt.h states the size of a step's record");

inline vpt_fluid_record vpt_fluid_make_record(const int32_t whd[3], const vpt_fluid_step& s) {
  return {whd[0], whd[1], whd[2], (uint32_t)s.open_faces, s.dt, {s.dt * s.lift[0], s.dt * s.lift[1], s.dt * s.lift[2]}, s.keep_density, s.keep_velocity,
      s.iterations, 0};
}
VPT_FLUID_HD bool vpt_fluid_open(uint32_t open, int axis, int side) { return (open >> (2 * axis + side)) & 1u; }   // side 0: the low face

// ---- 1. force: the velocity decays and is lifted by the density as it was, then the density decays ----------------------------------
VPT_FLUID_HD float vpt_fluid_force(float u, float keep_velocity, float force, float rho) {
  u = u * keep_velocity;
  u = u + force * rho;
  return vpt_filter_one_nan(u);
}
VPT_FLUID_HD float vpt_fluid_decay(float rho, float keep_density) { return vpt_filter_one_nan(rho * keep_density); }

// ---- 2. walls: the component normal to a closed face, at node i of the W along its axis ---------------------------------------------
VPT_FLUID_HD float vpt_fluid_wall(float u, int i, int W, uint32_t open, int axis) {
  const bool closed = (i == 0 && !vpt_fluid_open(open, axis, 0)) || (i == W - 1 && !vpt_fluid_open(open, axis, 1));
  return closed ? 0.0f : u;
}

// ---- 3. advect: where node i came from along one axis; the clamps are selects, a NaN becomes 0 ---------------------------------------
VPT_FLUID_HD float vpt_fluid_backtrace(int i, float dt, float u, int W) {
  float q = (float)i - dt * u;
  q       = q > 0.0f ? q : 0.0f;
  q       = q < (float)(W - 1) ? q : (float)(W - 1);
  return q;
}
VPT_FLUID_HD float vpt_fluid_advect(const float* field, int W, int H, int D, float qx, float qy, float qz) {
  return vpt_filter_one_nan(vpt_volgrid_trilerp(field, W, H, D, qx, qy, qz));
}

// ---- 2b. / 3'. what vpt_scene_fluid_step_detail adds (include/vpt.h): vorticity confinement and the MacCormack advection ----------------
// the detail as the kernels get it: VPT_FLUID_DETAIL_BYTES, made on the host by vpt_fluid_make_detail (a null detail: off)
struct vpt_fluid_detail_record {
  int32_t advection;
  float   k;   // dt * vorticity, one float32 product
};
static_assert(sizeof(vpt_fluid_detail_record) == VPT_FLUID_DETAIL_BYTES, "include/vpt.h states the size of a detail's record");
inline vpt_fluid_detail_record vpt_fluid_make_detail(const vpt_fluid_step& s, const vpt_fluid_detail* d) {
  return {d ? d->advection : VPT_FLUID_SEMI_LAGRANGIAN, d ? s.dt * d->vorticity : 0.0f};
}
inline bool vpt_fluid_confines(const vpt_fluid_detail* d) { return d && d->vorticity > 0.0f; }
inline bool vpt_fluid_maccormacks(const vpt_fluid_detail* d) { return d && d->advection == VPT_FLUID_MACCORMACK; }
// null, or what is wrong with the detail (null: off)
inline const char* vpt_fluid_detail_fault(const vpt_fluid_detail* d) {
  if (!d) return nullptr;
  if (d->advection != VPT_FLUID_SEMI_LAGRANGIAN && d->advection != VPT_FLUID_MACCORMACK)
    return "detail: advection is not one of VPT_FLUID_SEMI_LAGRANGIAN, VPT_FLUID_MACCORMACK";
  if (!std::isfinite(d->vorticity) || d->vorticity < 0.0f) return "detail: vorticity is not finite or is negative";
  return nullptr;
}

// a[+1] - a[-1] along one axis at node i of the W along it, `step` words between neighbours, the indices clamped to the volume: a[at +- step]
// is read only inside the volume, so `a` may as well be a tile in LDS whose positions outside the volume hold nothing
VPT_FLUID_HD float vpt_fluid_difference(const float* a, int at, int step, int i, int W) {
  return a[at + (vpt_filter_clamp(i + 1, W) - i) * step] - a[at + (vpt_filter_clamp(i - 1, W) - i) * step];
}
// omega at node (i, j, k) of the volume: u, v, w the three components at strides sx, sy, sz, [at] the node
VPT_FLUID_HD void vpt_fluid_curl(const float* u, const float* v, const float* w, int at, int sx, int sy, int sz, int i, int j, int k, const vpt_fluid_record& g,
    float omega[3]) {
  omega[0] = 0.5f * (vpt_fluid_difference(w, at, sy, j, g.h) - vpt_fluid_difference(v, at, sz, k, g.d));
  omega[1] = 0.5f * (vpt_fluid_difference(u, at, sz, k, g.d) - vpt_fluid_difference(w, at, sx, i, g.w));
  omega[2] = 0.5f * (vpt_fluid_difference(v, at, sx, i, g.w) - vpt_fluid_difference(u, at, sy, j, g.h));
}
VPT_FLUID_HD float vpt_fluid_length(const float a[3]) { return sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); }
// N x omega from the three clamped differences of m = |omega| and the node's own omega
VPT_FLUID_HD void vpt_fluid_confinement(float dmx, float dmy, float dmz, const float omega[3], float f[3]) {
  const float eta[3] = {0.5f * dmx, 0.5f * dmy, 0.5f * dmz};
  const float len    = vpt_fluid_length(eta) + 1e-12f;
  const float N[3]   = {eta[0] / len, eta[1] / len, eta[2] / len};
  f[0] = N[1] * omega[2] - N[2] * omega[1];
  f[1] = N[2] * omega[0] - N[0] * omega[2];
  f[2] = N[0] * omega[1] - N[1] * omega[0];
}
VPT_FLUID_HD float vpt_fluid_confine(float u, float k, float f) { return vpt_filter_one_nan(u + k * f); }

// where node i goes along one axis: vpt_fluid_backtrace with the other sign
VPT_FLUID_HD float vpt_fluid_foretrace(int i, float dt, float u, int W) {
  float r = (float)i + dt * u;
  r       = r > 0.0f ? r : 0.0f;
  r       = r < (float)(W - 1) ? r : (float)(W - 1);
  return r;
}
// vpt_fluid_advect, restated from vpt_volgrid_trilerp (the same i, ii, j, jj, k, kk, the same sum), that also answers the least and the
// greatest of the eight corners it loaded, by selects in the order of the sum's terms
VPT_FLUID_HD float vpt_fluid_advect_bounds(const float* vox, int W, int H, int D, float s, float t, float r, float& lo, float& hi) {
  int i = (int)s, j = (int)t, k = (int)r;
  i = i > 0 ? (i < W - 1 ? i : W - 1) : 0, j = j > 0 ? (j < H - 1 ? j : H - 1) : 0, k = k > 0 ? (k < D - 1 ? k : D - 1) : 0;
  const int   ii = i + 1 < W - 1 ? i + 1 : W - 1, jj = j + 1 < H - 1 ? j + 1 : H - 1, kk = k + 1 < D - 1 ? k + 1 : D - 1;
  const float u = s - i, v = t - j, w = r - k;
  const int   WH = W * H, r0 = j * W + k * WH, r1 = jj * W + k * WH, r2 = j * W + kk * WH, r3 = jj * W + kk * WH;
  const float c[8] = {vox[i + r0], vox[ii + r0], vox[i + r1], vox[i + r2], vox[i + r3], vox[ii + r2], vox[ii + r1], vox[ii + r3]};   // v000 v100 v010 v001 v011 v101 v110 v111
  lo = hi = c[0];
  for (int n = 1; n < 8; n++) lo = c[n] < lo ? c[n] : lo, hi = c[n] > hi ? c[n] : hi;
  return vpt_filter_one_nan(c[0] * (1 - u) * (1 - v) * (1 - w) + c[1] * u * (1 - v) * (1 - w) + c[2] * (1 - u) * v * (1 - w) + c[3] * (1 - u) * (1 - v) * w +
                            c[4] * (1 - u) * v * w + c[5] * u * (1 - v) * w + c[6] * u * v * (1 - w) + c[7] * u * v * w);
}
// the corrected value: hat the first pass's, own the node's before the advection, bar the first pass's traced forward again
VPT_FLUID_HD float vpt_fluid_maccormack(float hat, float own, float bar, float lo, float hi) {
  float v = hat + 0.5f * (own - bar);
  v       = v < lo ? lo : v;
  v       = v > hi ? hi : v;
  return vpt_filter_one_nan(v);
}

// ---- 5. divergence from the three central differences, each u[i + 1] - u[i - 1] with the indices clamped to the volume ----------------
VPT_FLUID_HD float vpt_fluid_divergence(float du, float dv, float dw) { return vpt_filter_one_nan(0.5f * ((du + dv) + dw)); }

// ---- 6. / 7. the pressure's neighbours ------------------------------------------------------------------------------------------------
// p at the neighbour `step` words from p[at]; outside: that neighbour lies across a face of the volume - the clamped node, which is the
// node itself, behind a closed face (Neumann), 0 behind an open one (Dirichlet).  p[at + step] is read only inside the volume, so `p` may
// as well be a tile in LDS whose positions outside the volume hold nothing.
VPT_FLUID_HD float vpt_fluid_near(const float* p, int at, int step, bool outside, bool open) { return outside ? (open ? 0.0f : p[at]) : p[at + step]; }

// one Jacobi sweep at node (i, j, k) of the volume, p[at] its value, sx / sy / sz the strides of `p`, d the divergence there
VPT_FLUID_HD float vpt_fluid_jacobi(const float* p, int at, int sx, int sy, int sz, int i, int j, int k, const vpt_fluid_record& g, float d) {
  float s = vpt_fluid_near(p, at, -sx, i == 0, vpt_fluid_open(g.open, 0, 0)) + vpt_fluid_near(p, at, sx, i == g.w - 1, vpt_fluid_open(g.open, 0, 1));
  s       = s + vpt_fluid_near(p, at, -sy, j == 0, vpt_fluid_open(g.open, 1, 0));
  s       = s + vpt_fluid_near(p, at, sy, j == g.h - 1, vpt_fluid_open(g.open, 1, 1));
  s       = s + vpt_fluid_near(p, at, -sz, k == 0, vpt_fluid_open(g.open, 2, 0));
  s       = s + vpt_fluid_near(p, at, sz, k == g.d - 1, vpt_fluid_open(g.open, 2, 1));
  s       = s - d;
  return vpt_filter_one_nan(s * (1.0f / 6.0f));
}
// a velocity component minus half the pressure difference along its axis (node i of W, stride `step`)
VPT_FLUID_HD float vpt_fluid_project(float u, const float* p, int at, int step, int i, int W, uint32_t open, int axis) {
  const float hi = vpt_fluid_near(p, at, step, i == W - 1, vpt_fluid_open(open, axis, 1));
  const float lo = vpt_fluid_near(p, at, -step, i == 0, vpt_fluid_open(open, axis, 0));
  return vpt_filter_one_nan(u - 0.5f * (hi - lo));
}

// ---- 6'. the pressure by multigrid (include/vpt.h: vpt_scene_fluid_step_solver): aggregation, Galerkin coarse operators -----------------
// one level as the kernels get it and the mirror reads it: its own size, the volume's, its index and its factor s_l
struct vpt_fluid_mg_level {
  int32_t  w, h, d;      // nodes of this level
  int32_t  w0, h0, d0;   // nodes of level 0
  int32_t  l;
  uint32_t open;
  float    s;            // s_0 = 1, s_{l+1} = s_l * 1.5f
};
constexpr int VPT_FLUID_MG_COARSEST = 8;   // the coarsest level is the first whose every axis is <= this
constexpr int VPT_FLUID_MG_MAX_LEVELS = 32;
VPT_FLUID_HD bool vpt_fluid_mg_coarsest(const vpt_fluid_mg_level& g) {
  return g.w <= VPT_FLUID_MG_COARSEST && g.h <= VPT_FLUID_MG_COARSEST && g.d <= VPT_FLUID_MG_COARSEST;
}
inline vpt_fluid_mg_level vpt_fluid_mg_level0(const vpt_fluid_record& g) { return {g.w, g.h, g.d, g.w, g.h, g.d, 0, g.open, 1.0f}; }
inline vpt_fluid_mg_level vpt_fluid_mg_coarser(const vpt_fluid_mg_level& g) {
  return {(g.w + 1) / 2, (g.h + 1) / 2, (g.d + 1) / 2, g.w0, g.h0, g.d0, g.l + 1, g.open, g.s * 1.5f};
}
// the levels of a volume, finest first; returns how many (the coarsest is the last)
inline int vpt_fluid_mg_levels(const vpt_fluid_record& g, vpt_fluid_mg_level out[VPT_FLUID_MG_MAX_LEVELS]) {
  int n  = 1;
  out[0] = vpt_fluid_mg_level0(g);
  while (!vpt_fluid_mg_coarsest(out[n - 1])) out[n] = vpt_fluid_mg_coarser(out[n - 1]), n++;
  return n;
}
// how many nodes of level 0 index I of level l covers along an axis of n0 nodes
VPT_FLUID_HD float vpt_fluid_mg_cover(int I, int l, int n0) {
  const int left = n0 - (I << l);
  return (float)(left < (1 << l) ? left : (1 << l));
}
// the right-hand side as stored: level 0 keeps stage 5's d, and b_0 = -d
VPT_FLUID_HD float vpt_fluid_mg_b(const vpt_fluid_mg_level& g, float stored) { return g.l == 0 ? -stored : stored; }
VPT_FLUID_HD int   vpt_fluid_mg_colour(int I, int J, int K) { return (I + J + K) & 1; }

// S and D at node (I, J, K) of level g.  at[0..5]: where in `p` its neighbours -x, +x, -y, +y, -z, +z lie; one outside the level is not read
VPT_FLUID_HD void vpt_fluid_mg_sums(const float* p, const int at[6], int I, int J, int K, const vpt_fluid_mg_level& g, float& S, float& D) {
  const float cx = vpt_fluid_mg_cover(I, g.l, g.w0), cy = vpt_fluid_mg_cover(J, g.l, g.h0), cz = vpt_fluid_mg_cover(K, g.l, g.d0);
  const float wgt[3]    = {cy * cz, cx * cz, cx * cy};
  const bool  inside[6] = {I > 0, I < g.w - 1, J > 0, J < g.h - 1, K > 0, K < g.d - 1};
  S = 0.0f, D = 0.0f;
  for (int n = 0; n < 6; n++) {
    if (inside[n]) S = S + wgt[n >> 1] * p[at[n]];
    if (inside[n] || ((g.open >> n) & 1u)) D = D + wgt[n >> 1];
  }
}
// a half-sweep's new value at a node of its colour: `was` where D == 0; sb = s_l * b
VPT_FLUID_HD float vpt_fluid_mg_scaled(const vpt_fluid_mg_level& g, float stored) { return g.s * vpt_fluid_mg_b(g, stored); }
VPT_FLUID_HD float vpt_fluid_mg_relax(float S, float D, float sb, float was) { return D == 0.0f ? was : vpt_filter_one_nan((S + sb) / D); }
// the residual in b's units at a node whose value is `centre`
VPT_FLUID_HD float vpt_fluid_mg_residual(float S, float D, float centre, float b, float s) { return vpt_filter_one_nan(b - (D * centre - S) / s); }
// the prolongation: a node's value plus its parent's
VPT_FLUID_HD float vpt_fluid_mg_correct(float fine, float parent) { return vpt_filter_one_nan(fine + parent); }

// null, or what is wrong with the solver (null: the Jacobi of stage 6)
inline const char* vpt_fluid_solver_fault(const vpt_fluid_solver* s) {
  if (!s || s->kind == VPT_FLUID_JACOBI) return nullptr;
  if (s->kind != VPT_FLUID_MULTIGRID) return "solver: kind is not one of VPT_FLUID_JACOBI, VPT_FLUID_MULTIGRID";
  if (s->cycles < 0 || s->cycles > VPT_FLUID_MAX_CYCLES) return "solver: cycles is not one of 0..64";
  if (s->smooth < 1 || s->smooth > VPT_FLUID_MAX_SMOOTH) return "solver: smooth is not one of 1..4";
  if (s->coarse_sweeps < 1 || s->coarse_sweeps > VPT_FLUID_MAX_COARSE_SWEEPS) return "solver: coarse_sweeps is not one of 1..64";
  return nullptr;
}
inline bool vpt_fluid_multigrid(const vpt_fluid_solver* s) { return s && s->kind == VPT_FLUID_MULTIGRID; }

// ---- what both sides refuse, in the same words ------------------------------------------------------------------------------------------
constexpr long long VPT_FLUID_MAX_NODES = 1ll << 30;
// null, or what is wrong with step `s` over `num_volumes` volumes whose sizes whd_of(id) answers; *unsupported: the size guard refused it
template <typename WhdOf>
inline const char* vpt_fluid_step_fault(const vpt_fluid_step& s, int num_volumes, WhdOf whd_of, bool* unsupported) {
  *unsupported = false;
  const int32_t ids[4] = {s.density, s.velocity[0], s.velocity[1], s.velocity[2]};
  for (int a = 0; a < 4; a++) {
    if (ids[a] < 0 || ids[a] >= num_volumes) return a == 0 ? "density: volume id out of range" : "velocity: volume id out of range";
    for (int b = 0; b < a; b++)
      if (ids[a] == ids[b]) return "density and velocity: two of the four volume ids are equal";
  }
  const int32_t* whd = whd_of(ids[0]);
  for (int a = 1; a < 4; a++)
    for (int k = 0; k < 3; k++)
      if (whd_of(ids[a])[k] != whd[k]) return "velocity: a volume's whd is not the density's";
  if (!std::isfinite(s.dt)) return "dt is not finite";
  if (!vpt_filter_finite(s.lift, 3)) return "lift is not finite";
  if (!std::isfinite(s.keep_density)) return "keep_density is not finite";
  if (!std::isfinite(s.keep_velocity)) return "keep_velocity is not finite";
  if (s.steps < 0) return "steps is negative";
  if (s.iterations < 0 || s.iterations > VPT_FLUID_MAX_ITERATIONS) return "iterations is not one of 0..1024";
  if (s.open_faces < 0 || s.open_faces > 63) return "open_faces has bits above the six faces";
  if ((long long)whd[0] * whd[1] * whd[2] > VPT_FLUID_MAX_NODES) return *unsupported = true, "more than 2^30 nodes in a volume";
  return nullptr;
}
