// vpt_split_policy.cpp — tile splitting (K1, K2): which tiles run as several partly filled waves, and the lane table of that launch.
// A wave runs all samples of its 64 pixels one after the other, so a launch cannot be shorter than its costliest tile.
// On one GPU that tile (273 ms of a 280 ms launch on 03_volume) is level with total work / wave slots and nothing is
// gained by shortening it; once the frame is shared among N GPUs the work per GPU falls with N and the chain does not.
// A tile can be run as 2^k waves that hold every 2^k-th pixel in their first 64 >> k lanes: fewer live lanes diverge
// less, the wave's trips get faster (g[k] below, measured on MI355X: DESIGN.md §5) - at 2^k g[k] times the slot time.
// Policy (split_factors): for a range of candidate spans S every tile is split just enough for its waves to fit S and the
// resulting launch is simulated (longest-first list scheduling on the chip's wave slots, durations scaled by how full the
// chip is); the shortest simulated launch wins if it beats the unsplit one by 2 %.  Taken once per layout / shader /
// camera from the per-tile costs of an unsplit launch, when the launch is short of waves: the frame is shared among ranks
// or holds fewer than three tiles per wave slot (1280x533 on one MI355X has 3.5 and never gains).  Pixels keep their own RNG streams and accumulators, so the result does
// not depend on it.
#include "vpt_split_policy.h"

#include <algorithm>
#include <cmath>
#include <functional>
#include <queue>

const double split_gain[7] = {1.0, 0.75, 0.57, 0.44, 0.34, 0.27, 0.20};   // duration of a 64 >> k lane wave of a costly tile / its full wave (round 4's
                                                                         // kernel, whose partly filled waves use their empty lanes as helpers: 0.753 / 0.566 / 0.436 / 0.343 measured, was 0.81 / 0.62 / 0.45 / 0.35)
const double split_gain_k2[7] = {1.0, 0.82, 0.67, 0.63, 0.60, 0.58, 0.56};   // the same for K2 (implicit shaders): 0.82 / 0.67 / 0.63 measured on 06_gridsdf_full (profiles/r04_k2_lane_histogram.txt), the rest extrapolated
static constexpr double split_load0 = 0.46, split_margin = 0.98;   // load_factor's intercept; a split has to beat the unsplit launch by this factor

// makespan of longest-first list scheduling of `costs` (any order) on `slots` machines: what the hardware's dispatch of
// the launch in d_order amounts to
static double lpt_makespan(std::vector<double>& costs, int slots) {
  std::sort(costs.begin(), costs.end(), std::greater<double>());
  std::priority_queue<double, std::vector<double>, std::greater<double>> load;
  double span = 0;
  for (size_t i = 0; i < costs.size(); i++) {
    double at = 0;
    if ((int)load.size() >= slots) at = load.top(), load.pop();
    load.push(at + costs[i]);
    span = std::max(span, at + costs[i]);
  }
  return span;
}
// A wave also runs faster when fewer waves share its SIMD: the costliest tile of 03_volume takes 273 ms with all 3 072
// slots busy and 187 ms when 1 340 waves are resident: duration ~ (0.46 + 0.54 * occupancy) * duration at 1
static double load_factor(double waves, int slots) { return split_load0 + (1 - split_load0) * std::min(1.0, waves / slots); }

std::vector<int> split_factors(const std::vector<unsigned>& cost, int slots, const double* gain, int forced_k) {
  const int        ntiles = (int)cost.size();
  std::vector<int> k((size_t)ntiles, 0);
  double cmax = 0;
  int    live = 0;
  for (unsigned c : cost) cmax = std::max(cmax, (double)c), live += c > 0;
  if (cmax <= 0) return k;
  const double measured_at = load_factor(live, slots);   // the costs were measured with `live` waves resident
  std::vector<double> waves;
  auto plan = [&](double S, bool apply) {   // predicted span when every tile is split just enough for its waves to fit S
    waves.clear();
    for (int t = 0; t < ntiles; t++) {
      if (cost[t] == 0) continue;
      int kt = 0;
      while (kt < 6 && cost[t] * gain[kt] > S) kt++;
      if (apply) k[t] = kt;
      for (int p = 0; p < (1 << kt); p++) waves.push_back(cost[t] * gain[kt]);
    }
    double f = load_factor((double)waves.size(), slots) / measured_at;
    for (double& w : waves) w *= f;
    return lpt_makespan(waves, slots);
  };
  if (forced_k >= 0) {
    for (int t = 0; t < ntiles; t++) k[t] = std::min(forced_k, 6);
  } else {
    double best_S = cmax, best = plan(cmax, false);
    for (int i = 1; i <= 24; i++) {   // candidates from the costliest tile down to its 1-lane duration
      double S = cmax * std::pow(gain[6], i / 24.0), span = plan(S, false);
      if (span < best * split_margin) best = span, best_S = S;   // a split has to pay at least 2 %
    }
    plan(best_S, true);
  }
  return k;
}

split_table make_split_table(const std::vector<int>& k, const std::vector<unsigned>& cost, const double* gain, int lanes) {
  const int   ntiles = (int)k.size();
  split_table out;
  long long   waves = 0;
  int         nsplit = 0;
  for (int t = 0; t < ntiles; t++) waves += 1ll << k[t], nsplit += k[t] > 0;
  if (nsplit == 0 || waves > (1ll << 24)) return out;
  out.lane_slot.assign((size_t)waves * lanes, -1);
  out.wave_cost.resize((size_t)waves);
  long long w = 0;
  for (int t = 0; t < ntiles; t++)
    for (int part = 0; part < (1 << k[t]); part++, w++) {
      out.wave_cost[(size_t)w] = (unsigned)(cost[t] * gain[k[t]]);
      for (int lane = 0; lane < (lanes >> k[t]); lane++) out.lane_slot[(size_t)w * lanes + lane] = t * lanes + (lane << k[t]) + part;
    }
  return out;
}
