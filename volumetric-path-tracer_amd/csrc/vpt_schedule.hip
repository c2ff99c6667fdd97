// vpt_schedule.hip — launch_schedule (vpt_schedule.h).  A .hip unit for rocPRIM's sort; the policy is vpt_split_policy.cpp's.
#include "vpt_schedule.h"

#include <cstdlib>
#include <numeric>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "vpt_kat.h"

static int env_int(const char* name) {   // -1: unset
  const char* e = getenv(name);
  return e ? atoi(e) : -1;
}
int split_mode() { static int v = env_int("VPT_SPLIT"); return v; }
int split_forced_k() { static int v = env_int("VPT_SPLIT_K"); return v; }


int launch_schedule::grow(long long waves) {
  if (waves <= sched_waves) return VPT_OK;
  if (!ev_order) {   // the first call, on the scene's device
    for (hipEvent_t* e : {&ev_host0, &ev_host1}) HIP_TRY(hipEventCreate(e));
    HIP_TRY(hipEventCreateWithFlags(&ev_order, hipEventDisableTiming));
  }
  sched_waves = 0, order_valid = false, cost_weight = 0;
  for (device_buffer* b : {&d_cost, &d_cost_sorted, &d_cost_key, &d_cost_avg, &d_order, &d_iota})
    if (int rc = b->allocate(waves * 4)) return rc;
  HIP_TRY(hipMemset(d_cost.get(), 0, waves * 4));   // waves that own no pixel never write theirs
  std::vector<int> iota((size_t)waves);
  std::iota(iota.begin(), iota.end(), 0);
  HIP_TRY(hipMemcpy(d_iota.get(), iota.data(), waves * 4, hipMemcpyHostToDevice));
  size_t bytes = 0;
  HIP_TRY(rocprim::radix_sort_pairs_desc((void*)nullptr, bytes, d_cost.get<unsigned>(), d_cost_sorted.get<unsigned>(), d_iota.get<int>(),
      d_order.get<int>(), (size_t)waves));
  if (int rc = sort_temp.allocate(bytes)) return rc;
  sort_temp_bytes = bytes, sched_waves = waves;
  return VPT_OK;
}

static constexpr float k_cost_horizon = 6;   // launches behind the running average
int launch_schedule::update(long long waves, hipStream_t st, int nsamples) {
  // nsamples > 0: d_cost holds the durations of a launch over that many samples: they enter the running average, whose order the next launch takes;
  // nsamples == 0: d_cost holds predictions (a fresh split table): they start a new average
  if (nsamples <= 0) cost_weight = 0;
  const float n = nsamples > 0 ? (float)nsamples : 1.0f;
  hipLaunchKernelGGL(vpt_cost_average_kernel, dim3((unsigned)((waves + 255) / 256)), dim3(256), 0, st, d_cost.get<unsigned>(), d_cost_avg.get<float>(),
      d_cost_key.get<unsigned>(), (int)waves, n, cost_weight);
  HIP_TRY(hipGetLastError());
  if (nsamples > 0) cost_weight = std::min(cost_weight + n, k_cost_horizon * n);   // the last few launches
  size_t bytes = sort_temp_bytes;
  HIP_TRY(rocprim::radix_sort_pairs_desc(sort_temp.get(), bytes, d_cost_key.get<unsigned>(), d_cost_sorted.get<unsigned>(), d_iota.get<int>(),
      d_order.get<int>(), (size_t)waves, 0, 32, st));
  HIP_TRY(hipEventRecord(ev_order, st));
  order_valid = true, order_stream = st;
  return VPT_OK;
}

// the policy on the costs of the unsplit launch that `st` has run; a table, if any tile is split, replaces the schedule of the layout
int launch_schedule::decide_split(int ntiles, int slots, hipStream_t st, const double* gain) {
  split_decided = true, split_waves = 0;
  HIP_TRY(hipStreamSynchronize(st));
  std::vector<unsigned> cost((size_t)ntiles);
  HIP_TRY(hipMemcpy(cost.data(), d_cost.get(), cost.size() * 4, hipMemcpyDeviceToHost));
  const split_table table = make_split_table(split_factors(cost, slots, gain, split_forced_k()), cost, gain, VPT_BLOCK);
  const long long   waves = (long long)table.wave_cost.size();
  if (waves == 0) return VPT_OK;
  if ((long long)table.lane_slot.size() > lane_cap) {
    lane_cap = 0;
    if (int rc = d_lane_slot.allocate(table.lane_slot.size() * 4)) return rc;
    lane_cap = (long long)table.lane_slot.size();
  }
  if (int rc = grow(waves)) return rc;   // may reallocate d_cost / d_order for the larger wave count
  HIP_TRY(hipMemcpy(d_lane_slot.get(), table.lane_slot.data(), table.lane_slot.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_cost.get(), table.wave_cost.data(), table.wave_cost.size() * 4, hipMemcpyHostToDevice));
  split_waves = (int)waves;
  return update(waves, st, 0);   // order of the split launch from the predicted costs; measured ones take over afterwards
}

extern "C" int vpt_split_plan(int kernel, const unsigned* costs, int ntiles, int wave_slots, int forced_k, int* k_out, int* waves_out) {
  if (kernel < 0 || kernel > 1 || ntiles < 0 || (ntiles > 0 && (!costs || !k_out)) || wave_slots <= 0 || !waves_out)
    return vpt_set_error(VPT_ERR_INVALID_ARG, "bad argument");
  const std::vector<unsigned> cost(costs, costs + ntiles);
  const double*               gain = kernel ? split_gain_k2 : split_gain;
  const std::vector<int>      k = split_factors(cost, wave_slots, gain, forced_k);
  const split_table           table = make_split_table(k, cost, gain, VPT_BLOCK);
  std::copy(k.begin(), k.end(), k_out);
  *waves_out = table.wave_cost.empty() ? ntiles : (int)table.wave_cost.size();
  return VPT_OK;
}
