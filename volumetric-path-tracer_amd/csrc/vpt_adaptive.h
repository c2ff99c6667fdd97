// vpt_adaptive.h — the device half of adaptive sampling (csrc/vpt_adaptive.hip), called by the round loop of
// vpt_adaptive_run (vpt_capi.hip).  Rule and data flow: include/vpt.h (vpt_adaptive) and DESIGN.md §10, §23.
#pragma once
#include "vpt_device.h"
#include "vpt_error.h"

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

// n == 0: start (lum_prev from the entry image, active = slot owns a pixel and hits < cap, min / max of hits);
// n >= 1: the pixels still active have just rendered their n-th round of m samples: update and decide (vpt.h).
// Then the compaction of the active slots into b.lane_slot and their count into b.info[0].  Asynchronous on `st`.
int adaptive_update(const DParams& pr, const float4* image, const int* hits, const adaptive_buffers& b, int n, int m,
                    const vpt_adaptive& a, int cap, hipStream_t st);

// b.stats and `hits` (tile-major) as row-major width x height planes, each nullable: the squared standard error of vpt.h's rule
// with n_p = ceil(hits / step), the hits, and the Welford mean and m2 themselves.  Pixels of other ranks are left as they are.
int adaptive_noise(const DParams& pr, const adaptive_buffers& b, const int* hits, int step, float* se2, int* hits_out, float* mean_out,
                   float* m2_out, hipStream_t st);
