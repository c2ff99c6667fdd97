// vpt_split_policy.h — the tile-splitting policy of K1 and K2 (vpt_split_policy.cpp): host arithmetic over the per-tile costs of an
// unsplit launch, with no device call and no HIP header.  Its callers: launch_schedule and vpt_split_plan (vpt_schedule.hip).
#pragma once
#include <vector>

extern const double split_gain[7], split_gain_k2[7];   // duration of a 64 >> k lane wave / its full wave: K1, K2

// per tile: it runs as 2^k waves.  forced_k >= 0 (VPT_SPLIT_K): every tile min(forced_k, 6), unless no tile cost anything
std::vector<int> split_factors(const std::vector<unsigned>& cost, int slots, const double* gain, int forced_k);

struct split_table {   // both empty: no table (no tile is split, or the table would pass 2^24 waves): the launch stays unsplit
  std::vector<int>      lane_slot;   // [wave][lanes] -> state slot of the lane (-1: none)
  std::vector<unsigned> wave_cost;   // predicted duration of each wave: cost * gain[k] of its tile
};
// lane table and predicted wave costs for the split factors k of tiles of `lanes` pixels
split_table make_split_table(const std::vector<int>& k, const std::vector<unsigned>& cost, const double* gain, int lanes);
