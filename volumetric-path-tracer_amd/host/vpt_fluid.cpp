// vpt_fluid.cpp — a stable-fluids step on the CPU: the rule of include/vpt.h (vpt_scene_fluid_step) through the same header as the
// kernels (csrc/vpt_fluid_rule.h), one stage after another in plain serial loops over the whole grid - the statement the kernels are held
// to bit for bit.  Every stage is a function of its own, so that the tests can hold each to float64.
#include <algorithm>
#include <cstdio>

#include "vpt_fluid_rule.h"
#include "vpt_host.h"

namespace vpt {

namespace {

// f[0] the density, f[1..3] the velocity; every loop x fastest
template <typename Node>
void each_node(const vpt_fluid_record& g, Node node) {
  for (auto k = 0; k < g.d; k++)
    for (auto j = 0; j < g.h; j++)
      for (auto i = 0; i < g.w; i++) node(i, j, k, i + g.w * (j + g.h * k));
}
size_t nodes_of(const vpt_fluid_record& g) { return (size_t)g.w * (size_t)g.h * (size_t)g.d; }

void force(float* const f[4], const vpt_fluid_record& g) {
  each_node(g, [&](int, int, int, int at) {
    const auto rho = f[0][at];
    for (auto c = 0; c < 3; c++) f[1 + c][at] = vpt_fluid_force(f[1 + c][at], g.keep_velocity, g.force[c], rho);
    f[0][at] = vpt_fluid_decay(rho, g.keep_density);
  });
}
void walls(float* const f[4], const vpt_fluid_record& g) {
  each_node(g, [&](int i, int j, int k, int at) {
    f[1][at] = vpt_fluid_wall(f[1][at], i, g.w, g.open, 0);
    f[2][at] = vpt_fluid_wall(f[2][at], j, g.h, g.open, 1);
    f[3][at] = vpt_fluid_wall(f[3][at], k, g.d, g.open, 2);
  });
}
void advect(float* const f[4], const vpt_fluid_record& g) {
  vector<float> old[4];
  for (auto c = 0; c < 4; c++) old[c].assign(f[c], f[c] + nodes_of(g));
  each_node(g, [&](int i, int j, int k, int at) {
    const auto qx = vpt_fluid_backtrace(i, g.dt, old[1][at], g.w), qy = vpt_fluid_backtrace(j, g.dt, old[2][at], g.h), qz = vpt_fluid_backtrace(k, g.dt, old[3][at], g.d);
    for (auto c = 0; c < 4; c++) f[c][at] = vpt_fluid_advect(old[c].data(), g.w, g.h, g.d, qx, qy, qz);
  });
}
// stage 2b: every node reads the velocity as stage 2 left it; m = |omega| over the whole grid first, then the force
void confine(float* const f[4], const vpt_fluid_record& g, float strength) {
  vector<float> old[3];
  for (auto c = 0; c < 3; c++) old[c].assign(f[1 + c], f[1 + c] + nodes_of(g));
  auto       m  = vector<float>(nodes_of(g));
  const auto sy = g.w, sz = g.w * g.h;
  each_node(g, [&](int i, int j, int k, int at) {
    float omega[3];
    vpt_fluid_curl(old[0].data(), old[1].data(), old[2].data(), at, 1, sy, sz, i, j, k, g, omega);
    m[at] = vpt_fluid_length(omega);
  });
  each_node(g, [&](int i, int j, int k, int at) {
    float omega[3], push[3];
    vpt_fluid_curl(old[0].data(), old[1].data(), old[2].data(), at, 1, sy, sz, i, j, k, g, omega);
    vpt_fluid_confinement(vpt_fluid_difference(m.data(), at, 1, i, g.w), vpt_fluid_difference(m.data(), at, sy, j, g.h), vpt_fluid_difference(m.data(), at, sz, k, g.d), omega,
        push);
    for (auto c = 0; c < 3; c++) f[1 + c][at] = vpt_fluid_confine(old[c][at], strength, push[c]);
  });
  walls(f, g);
}
// stage 3 with VPT_FLUID_MACCORMACK: the first pass over the whole grid, then the corrected and limited second
void advect_maccormack(float* const f[4], const vpt_fluid_record& g) {
  vector<float> old[4], hat[4];
  for (auto c = 0; c < 4; c++) old[c].assign(f[c], f[c] + nodes_of(g)), hat[c].resize(nodes_of(g));
  each_node(g, [&](int i, int j, int k, int at) {
    const auto qx = vpt_fluid_backtrace(i, g.dt, old[1][at], g.w), qy = vpt_fluid_backtrace(j, g.dt, old[2][at], g.h), qz = vpt_fluid_backtrace(k, g.dt, old[3][at], g.d);
    for (auto c = 0; c < 4; c++) hat[c][at] = vpt_fluid_advect(old[c].data(), g.w, g.h, g.d, qx, qy, qz);
  });
  each_node(g, [&](int i, int j, int k, int at) {
    const auto qx = vpt_fluid_backtrace(i, g.dt, old[1][at], g.w), qy = vpt_fluid_backtrace(j, g.dt, old[2][at], g.h), qz = vpt_fluid_backtrace(k, g.dt, old[3][at], g.d);
    const auto rx = vpt_fluid_foretrace(i, g.dt, old[1][at], g.w), ry = vpt_fluid_foretrace(j, g.dt, old[2][at], g.h), rz = vpt_fluid_foretrace(k, g.dt, old[3][at], g.d);
    for (auto c = 0; c < 4; c++) {
      float      lo, hi;
      const auto first = vpt_fluid_advect_bounds(old[c].data(), g.w, g.h, g.d, qx, qy, qz, lo, hi);
      const auto bar   = vpt_volgrid_trilerp(hat[c].data(), g.w, g.h, g.d, rx, ry, rz);
      f[c][at] = vpt_fluid_maccormack(first, old[c][at], bar, lo, hi);
    }
  });
}
void divergence(const float* const f[4], const vpt_fluid_record& g, float* div) {
  const int sy = g.w, sz = g.w * g.h;
  each_node(g, [&](int i, int j, int k, int at) {
    const auto du = f[1][at + (vpt_filter_clamp(i + 1, g.w) - i)] - f[1][at + (vpt_filter_clamp(i - 1, g.w) - i)];
    const auto dv = f[2][at + (vpt_filter_clamp(j + 1, g.h) - j) * sy] - f[2][at + (vpt_filter_clamp(j - 1, g.h) - j) * sy];
    const auto dw = f[3][at + (vpt_filter_clamp(k + 1, g.d) - k) * sz] - f[3][at + (vpt_filter_clamp(k - 1, g.d) - k) * sz];
    div[at] = vpt_fluid_divergence(du, dv, dw);
  });
}
void pressure(const vpt_fluid_record& g, const float* div, float* p) {
  auto from = vector<float>(nodes_of(g), 0.0f), to = from;
  for (auto n = 0; n < g.iterations; n++) {
    each_node(g, [&](int i, int j, int k, int at) { to[at] = vpt_fluid_jacobi(from.data(), at, 1, g.w, g.w * g.h, i, j, k, g, div[at]); });
    from.swap(to);
  }
  std::copy(from.begin(), from.end(), p);
}

// ---- the pressure by multigrid: the V-cycle of include/vpt.h over the rule header's functions, a level at a time, in place ---------------
template <typename Node>
void each_node(const vpt_fluid_mg_level& g, Node node) {
  for (auto k = 0; k < g.d; k++)
    for (auto j = 0; j < g.h; j++)
      for (auto i = 0; i < g.w; i++) node(i, j, k, i + g.w * (j + g.h * k));
}
void mg_sums(const vpt_fluid_mg_level& g, const float* p, int i, int j, int k, int at, float& S, float& D) {
  const int near[6] = {at - 1, at + 1, at - g.w, at + g.w, at - g.w * g.h, at + g.w * g.h};
  vpt_fluid_mg_sums(p, near, i, j, k, g, S, D);
}
void mg_half_sweep(const vpt_fluid_mg_level& g, const float* b, float* p, int colour) {
  each_node(g, [&](int i, int j, int k, int at) {
    if (vpt_fluid_mg_colour(i, j, k) != colour) return;
    float S, D;
    mg_sums(g, p, i, j, k, at, S, D);
    p[at] = vpt_fluid_mg_relax(S, D, vpt_fluid_mg_scaled(g, b[at]), p[at]);
  });
}
void mg_sweeps(const vpt_fluid_mg_level& g, const float* b, float* p, int sweeps, int first) {
  for (auto n = 0; n < sweeps; n++) mg_half_sweep(g, b, p, first), mg_half_sweep(g, b, p, first ^ 1);
}
struct mg_fields {
  vector<float> p, b;   // of the levels above 0
};
void mg_cycle(const vpt_fluid_mg_level* levels, int count, int l, const float* b, float* p, vector<mg_fields>& coarse, const vpt_fluid_solver& s) {
  const auto& g = levels[l];
  if (l == count - 1) return mg_sweeps(g, b, p, s.coarse_sweeps, 0);
  mg_sweeps(g, b, p, s.smooth, 0);
  const auto& c    = levels[l + 1];
  auto&       next = coarse[(size_t)l + 1];
  next.p.assign((size_t)c.w * c.h * c.d, 0.0f);
  next.b.assign(next.p.size(), 0.0f);
  auto r = vector<float>((size_t)g.w * g.h * g.d);
  each_node(g, [&](int i, int j, int k, int at) {
    float S, D;
    mg_sums(g, p, i, j, k, at, S, D);
    r[at] = vpt_fluid_mg_residual(S, D, p[at], vpt_fluid_mg_b(g, b[at]), g.s);
  });
  each_node(c, [&](int I, int J, int K, int at) {
    auto sum = 0.0f;
    for (auto z = 2 * K; z < 2 * K + 2 && z < g.d; z++)
      for (auto y = 2 * J; y < 2 * J + 2 && y < g.h; y++)
        for (auto x = 2 * I; x < 2 * I + 2 && x < g.w; x++) sum = sum + r[x + g.w * (y + g.h * z)];
    next.b[at] = vpt_filter_one_nan(sum);
  });
  mg_cycle(levels, count, l + 1, next.b.data(), next.p.data(), coarse, s);
  each_node(g, [&](int i, int j, int k, int at) { p[at] = vpt_fluid_mg_correct(p[at], next.p[(i / 2) + c.w * ((j / 2) + c.h * (k / 2))]); });
  mg_sweeps(g, b, p, s.smooth, 1);
}
void pressure_multigrid(const vpt_fluid_record& g, const vpt_fluid_solver& s, const float* div, float* p) {
  vpt_fluid_mg_level levels[VPT_FLUID_MG_MAX_LEVELS];
  const auto         count  = vpt_fluid_mg_levels(g, levels);
  auto               coarse = vector<mg_fields>((size_t)count);
  std::fill(p, p + nodes_of(g), 0.0f);
  for (auto n = 0; n < s.cycles; n++) mg_cycle(levels, count, 0, div, p, coarse, s);
}

void project(float* const f[4], const vpt_fluid_record& g, const float* p) {
  each_node(g, [&](int i, int j, int k, int at) {
    f[1][at] = vpt_fluid_project(f[1][at], p, at, 1, i, g.w, g.open, 0);
    f[2][at] = vpt_fluid_project(f[2][at], p, at, g.w, j, g.h, g.open, 1);
    f[3][at] = vpt_fluid_project(f[3][at], p, at, g.w * g.h, k, g.d, g.open, 2);
  });
  walls(f, g);
}

// the step's fault with the ids left to the caller: the four arrays are four volumes of `whd`
const char* fault_of(const int32_t whd[3], vpt_fluid_step s) {
  if (whd[0] < 0 || whd[1] < 0 || whd[2] < 0) return "bad volume size";
  s.density = 0, s.velocity[0] = 1, s.velocity[1] = 2, s.velocity[2] = 3;
  bool unsupported;
  return vpt_fluid_step_fault(s, 4, [&](int) { return whd; }, &unsupported);
}

}  // namespace

bool fluid_stage(int stage, float* const f[4], float* p, float* div, const int32_t whd[3], const vpt_fluid_step& s, string& error) {
  if (auto fault = fault_of(whd, s)) return error = string{"fluid: "} + fault, false;
  const auto g = vpt_fluid_make_record(whd, s);
  switch (stage) {
    case 0: force(f, g); break;
    case 1: walls(f, g); break;
    case 2: advect(f, g); break;
    case 3: divergence(f, g, div); break;
    case 4: pressure(g, div, p); break;
    case 5: project(f, g, p); break;
    default: return error = "fluid: stage is not one of 0..5", false;
  }
  return true;
}

bool fluid_detail_stage(int stage, float* const f[4], const int32_t whd[3], const vpt_fluid_step& s, const vpt_fluid_detail& detail, string& error) {
  if (auto fault = fault_of(whd, s)) return error = string{"fluid: "} + fault, false;
  if (auto fault = vpt_fluid_detail_fault(&detail)) return error = string{"fluid: "} + fault, false;
  const auto g = vpt_fluid_make_record(whd, s);
  switch (stage) {
    case 0: confine(f, g, vpt_fluid_make_detail(s, &detail).k); break;
    case 1: advect_maccormack(f, g); break;
    default: return error = "fluid: detail stage is not one of 0, 1", false;
  }
  return true;
}

bool fluid_step(float* const f[4], const int32_t whd[3], const vpt_fluid_step& s, const vpt_fluid_solver* solver, const vpt_fluid_detail* detail, string& error) {
  if (auto fault = fault_of(whd, s)) return error = string{"fluid: "} + fault, false;
  if (auto fault = vpt_fluid_solver_fault(solver)) return error = string{"fluid: "} + fault, false;
  if (auto fault = vpt_fluid_detail_fault(detail)) return error = string{"fluid: "} + fault, false;
  const auto g = vpt_fluid_make_record(whd, s);
  auto       div = vector<float>(nodes_of(g)), p = div;
  for (auto n = 0; n < s.steps && nodes_of(g) > 0; n++) {
    force(f, g), walls(f, g);
    if (vpt_fluid_confines(detail)) confine(f, g, vpt_fluid_make_detail(s, detail).k);
    if (vpt_fluid_maccormacks(detail)) advect_maccormack(f, g);
    else advect(f, g);
    walls(f, g);
    divergence(f, g, div.data());
    if (vpt_fluid_multigrid(solver)) pressure_multigrid(g, *solver, div.data(), p.data());
    else pressure(g, div.data(), p.data());
    project(f, g, p.data());
  }
  return true;
}
bool fluid_step(float* const f[4], const int32_t whd[3], const vpt_fluid_step& s, const vpt_fluid_solver* solver, string& error) {
  return fluid_step(f, whd, s, solver, nullptr, error);
}
bool fluid_step(float* const f[4], const int32_t whd[3], const vpt_fluid_step& s, string& error) { return fluid_step(f, whd, s, nullptr, nullptr, error); }

bool fluid_multigrid_pressure(const float* div, float* p, const int32_t whd[3], int open_faces, const vpt_fluid_solver& solver, string& error) {
  auto step = vpt_fluid_step{};
  step.open_faces = open_faces;
  if (auto fault = fault_of(whd, step)) return error = string{"fluid: "} + fault, false;
  if (auto fault = vpt_fluid_solver_fault(&solver)) return error = string{"fluid: "} + fault, false;
  if (!vpt_fluid_multigrid(&solver)) return error = "fluid: solver: kind is not VPT_FLUID_MULTIGRID", false;
  const auto g = vpt_fluid_make_record(whd, step);
  if (nodes_of(g) > 0) pressure_multigrid(g, solver, div, p);
  return true;
}

}  // namespace vpt

extern "C" {

// the host mirror on four host arrays of whd[0] * whd[1] * whd[2] nodes (x fastest); the step's volume ids are ignored.  A refused call writes nothing.
int vpth_fluid_step_detail(float* density, float* u, float* v, float* w, const int32_t* whd, const vpt_fluid_step* step, const vpt_fluid_solver* solver,
    const vpt_fluid_detail* detail, char* err, int errlen) {
  auto         error = vpt::string{};
  float* const f[4]  = {density, u, v, w};
  if (!density || !u || !v || !w || !whd || !step) error = "fluid: null argument";
  else if (vpt::fluid_step(f, whd, *step, solver, detail, error)) return 0;
  if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", error.c_str());
  return -1;
}
int vpth_fluid_step_solver(float* density, float* u, float* v, float* w, const int32_t* whd, const vpt_fluid_step* step, const vpt_fluid_solver* solver, char* err,
    int errlen) {
  return vpth_fluid_step_detail(density, u, v, w, whd, step, solver, nullptr, err, errlen);
}
int vpth_fluid_step(float* density, float* u, float* v, float* w, const int32_t* whd, const vpt_fluid_step* step, char* err, int errlen) {
  return vpth_fluid_step_solver(density, u, v, w, whd, step, nullptr, err, errlen);
}
// one stage of vpt_scene_fluid_step_detail's rule alone: 0 stage 2b and its walls (whatever detail->vorticity), 1 stage 3 with VPT_FLUID_MACCORMACK
int vpth_fluid_detail_stage(int stage, float* density, float* u, float* v, float* w, const int32_t* whd, const vpt_fluid_step* step, const vpt_fluid_detail* detail, char* err,
    int errlen) {
  auto         error = vpt::string{};
  float* const f[4]  = {density, u, v, w};
  if (!density || !u || !v || !w || !whd || !step || !detail) error = "fluid: null argument";
  else if (vpt::fluid_detail_stage(stage, f, whd, *step, *detail, error)) return 0;
  if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", error.c_str());
  return -1;
}
// stage 6 alone by multigrid (include/vpt.h: vpt_scene_fluid_step_solver): div -> p, `solver->cycles` V-cycles from 0
int vpth_fluid_multigrid_pressure(const float* div, float* p, const int32_t* whd, int open_faces, const vpt_fluid_solver* solver, char* err, int errlen) {
  auto error = vpt::string{};
  if (!div || !p || !whd || !solver) error = "fluid: null argument";
  else if (vpt::fluid_multigrid_pressure(div, p, whd, open_faces, *solver, error)) return 0;
  if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", error.c_str());
  return -1;
}
// one stage of the rule alone: 0 force, 1 walls, 2 advect, 3 divergence (into div), 4 pressure (div -> p, step->iterations sweeps from 0),
// 5 project (reads p) and walls.  p and div are read or written by stages 3 .. 5 only
int vpth_fluid_stage(int stage, float* density, float* u, float* v, float* w, float* p, float* div, const int32_t* whd, const vpt_fluid_step* step, char* err, int errlen) {
  auto         error = vpt::string{};
  float* const f[4]  = {density, u, v, w};
  if (!density || !u || !v || !w || !whd || !step || (stage >= 3 && !div) || (stage >= 4 && !p)) error = "fluid: null argument";
  else if (vpt::fluid_stage(stage, f, p, div, whd, *step, error)) return 0;
  if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", error.c_str());
  return -1;
}

}  // extern "C"
