// vpt_schedule.h — the launch schedule of one scene handle (sched_cfg, vpt_launch.h): per-wave costs, the longest-wave-first order
// made from them, pilot launches and the tile-splitting decision (vpt_split_policy.h).  Only run() changes it (vpt_render_device).
#pragma once
#include <algorithm>
#include <cstring>

#include "vpt_device_buffer.h"
#include "vpt_launch.h"
#include "vpt_split_policy.h"

int split_mode();       // VPT_SPLIT: 0 never, 1 always consider, unset (-1): consider when the launch is short of waves
int split_forced_k();   // VPT_SPLIT_K (calibration): every tile as 2^k waves; unset: -1

class launch_schedule {
 public:
  int compute_units = 256;   // of the scene's device; wave slots of the chip for K1 / K2: CUs x 4 SIMDs x the kernel's waves per SIMD
  int wave_slots(bool k2) const { return compute_units * 4 * (k2 ? VPT_K2_WAVES : VPT_WAVES_PER_SIMD); }
  ~launch_schedule() {   // its events go with it (so it is neither copied nor moved)
    for (hipEvent_t e : {ev_order, ev_host0, ev_host1})
      if (e) (void)hipEventDestroy(e);
  }

  // The launch loop of K1 and K2, for one vpt_render_device call of `nsamples` samples over `grid` on `st`.  Longest-wave-first order
  // from the costs of the previous launch on the layout `key`; without them a pilot launch over 1/64 of the call's samples (1..16)
  // measures them first - same arithmetic, batching is exact (K2 in tile order: a first call ran at 216 against 302 Msamples/s on
  // 06_gridsdf).  may_split, k2: whether and for which kernel the tile-splitting policy is consulted; launch(is_pilot, grid, nsamples,
  // sch) launches the kernel instance for the part.
  template <typename Launch>
  int run(const long long (&key)[10], dim3 full_grid, int nsamples, hipStream_t st, bool may_split, bool k2, Launch&& launch) {
    host_pause = false;
    if (int rc = grow(std::max<long long>(full_grid.x, split_waves))) return rc;
    if (memcmp(key, sched_key, sizeof(sched_key)) != 0) forget(), memcpy(sched_key, key, sizeof(sched_key));   // layout / camera / shader changed
    // d_order / d_cost are written on the stream of the previous launch: a launch on another stream waits for that sort
    if (order_valid && order_stream != st) HIP_TRY(hipStreamWaitEvent(st, ev_order, 0));
    int n = nsamples, pilot = n / 64 < 1 ? 1 : n / 64 > 16 ? 16 : n / 64;
    int parts[2] = {(!order_valid && n >= 16) ? pilot : n, 0};
    parts[1] = n - parts[0];
    for (int part = 0; part < 2 && parts[part] > 0; part++) {
      const bool is_pilot = parts[1] > 0 && part == 0;
      // the costs of an unsplit launch over at least 8 samples decide, once, whether tiles are split from now on
      if (may_split && !split_decided && order_valid && full_costs) {
        // the decision waits for the stream and reads costs back on the host: that pause is bracketed by its own event pair and
        // subtracted by vpt_last_kernel_ms (a pilot launch that ran before it in this call stays counted)
        HIP_TRY(hipEventRecord(ev_host0, st));
        if (int rc = decide_split((int)full_grid.x, wave_slots(k2), st, k2 ? split_gain_k2 : split_gain)) return rc;
        HIP_TRY(hipEventRecord(ev_host1, st));
        host_pause = true;
      }
      dim3 grid = split_waves > 0 ? dim3((unsigned)split_waves) : full_grid;
      sched_cfg sch = {order_valid ? d_order.get<int>() : nullptr, d_cost.get<unsigned>(), split_waves > 0 ? d_lane_slot.get<int>() : nullptr};
      launch(is_pilot, grid, parts[part], sch);
      if (split_waves == 0) full_costs = parts[part] >= 8;   // d_cost now holds per-tile durations over enough samples (a pilot of a call with >= 512 samples counts)
      last_waves = (int)grid.x;
      if (int rc = update(grid.x, st, parts[part])) return rc;
    }
    return VPT_OK;
  }
  // the measured costs, the order made from them and the tile-splitting decision go (the buffers stay)
  void forget() { order_valid = false, split_decided = false, full_costs = false, split_waves = 0, cost_weight = 0; }
  void no_pause() { host_pause = false; }   // a timed call that does not go through run()
  int  paused_ms(float* ms) const {         // host-side pause inside the last run() (decide_split): not kernel time
    *ms = 0;
    if (host_pause) HIP_TRY(hipEventElapsedTime(ms, ev_host0, ev_host1));
    return VPT_OK;
  }
  int  last_wave_costs(unsigned* ticks, int capacity, int* count) const {   // of the last launch, once it has ended (synchronous copy)
    *count = last_waves;
    const size_t n = (size_t)std::min(last_waves, capacity);
    if (n > 0) HIP_TRY(hipMemcpy(ticks, d_cost.get(), n * 4, hipMemcpyDeviceToHost));
    return VPT_OK;
  }

 private:
  int grow(long long waves);                                                       // the buffers, for at least `waves` waves; first, the events
  int update(long long waves, hipStream_t st, int nsamples);                       // order[] for the next launch
  int decide_split(int ntiles, int slots, hipStream_t st, const double* gain);

  device_buffer d_cost, d_cost_sorted, d_cost_key;   // unsigned: per-wave cost of the last launch
  device_buffer d_cost_avg;            // float: running average of a wave's duration per sample (vpt_cost_average_kernel)
  float         cost_weight = 0;       // samples behind that average (0: none yet)
  device_buffer d_order, d_iota;       // int: waves by descending cost
  hipEvent_t    ev_order = nullptr;    // recorded after the sort that writes d_order
  hipStream_t   order_stream = nullptr;   // the stream that sort ran on
  device_buffer sort_temp;
  size_t        sort_temp_bytes = 0;
  // tile splitting: tiles whose pixels run as 2^k partly filled waves, so that a launch is not as long as its costliest tile
  device_buffer d_lane_slot;   // int
  long long     lane_cap = 0;
  int           split_waves = 0;         // waves of the split launch (0: no table)
  bool          full_costs = false;      // d_cost holds per-tile durations of an unsplit launch over >= 8 samples
  bool          split_decided = false;   // the decision for sched_key has been taken (costs of an unsplit launch were available)
  int           last_waves = 0;          // grid of the last kernel launch
  long long     sched_waves = 0;         // waves the buffers are sized for
  bool          order_valid = false;     // d_order describes the layout of sched_key
  long long     sched_key[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  hipEvent_t    ev_host0 = nullptr, ev_host1 = nullptr;   // around the host-side pause of decide_split
  bool          host_pause = false;      // the last run() recorded that pair
};
