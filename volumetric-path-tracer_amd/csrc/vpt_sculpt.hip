// vpt_sculpt.hip — the voxel grids of a resident scene sculpted in place with analytic SDF brushes (include/vpt.h:
// vpt_scene_sculpt_volumes).  The arithmetic is csrc/vpt_sculpt_rule.h's, which the host mirror (host/vpt_sculpt.cpp)
// compiles too: this unit is built with -ffp-contract=off like it.  Here: the validation of an edit, the stamps' records, and one kernel.
#include <vector>

#include "vpt_error.h"
#include "vpt_sculpt.h"
#include "vpt_sculpt_rule.h"
#include "vpt_update_helpers.h"

namespace {

struct sculpt_grid {
  int   w, h;                  // the volume's row and slice
  int   lo_x, lo_y, lo_z;      // the region
  int   rw, rh;
  float origin[3], step[3];
};

// One lane per voxel of the region (n < 2^31 of them, x fastest: a wave's loads and stores of the grid are consecutive).  The value is
// read once and written once however many stamps there are (reads == 0: the first stamp is a REPLACE, nothing is read).  The records
// are read-only and indexed by the loop counter alone, so every lane of a wave reads the same one: uniform loads, and the switches on
// type and op are uniform branches.  Every lane evaluates every stamp.
__global__ __launch_bounds__(BLOCK) void sculpt_kernel(float* __restrict__ grid, sculpt_grid g, unsigned n, const vpt_sculpt_record* __restrict__ records,
    int num, int reads) {
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;   // the last block's lanes stay below 2^32
  if (idx >= n) return;
  const unsigned x = idx % (unsigned)g.rw, y = (idx / (unsigned)g.rw) % (unsigned)g.rh, z = idx / ((unsigned)g.rw * (unsigned)g.rh);
  const int      i = g.lo_x + (int)x, j = g.lo_y + (int)y, k = g.lo_z + (int)z;
  const size_t   at = (size_t)i + (size_t)j * (size_t)g.w + (size_t)k * (size_t)g.w * (size_t)g.h;
  const vpt_sculpt_f3 p = {vpt_sculpt_sample(g.origin[0], g.step[0], i), vpt_sculpt_sample(g.origin[1], g.step[1], j), vpt_sculpt_sample(g.origin[2], g.step[2], k)};
  float v = reads ? grid[at] : 0.0f;
  for (int s = 0; s < num; s++) v = vpt_sculpt_stamp_value(records[s], p, v);
  grid[at] = v;
}

int validate_edit(const DScene& d, const edit_mirrors& m, const vpt_sculpt_edit& e) {
  REQUIRE(e.num_entries >= 0 && (e.num_entries == 0 || e.entries), "sculpt: the entry list is null or has a negative count");
  REQUIRE(e.num_stamps >= 0 && (e.num_stamps == 0 || e.stamps), "sculpt: the stamp list is null or has a negative count");
  for (int i = 0; i < e.num_stamps; i++)
    if (const char* fault = vpt_sculpt_stamp_fault(e.stamps[i])) return vpt_set_error(VPT_ERR_INVALID_ARG, "sculpt: stamp %d: %s", i, fault);
  for (int i = 0; i < e.num_entries; i++) {
    const vpt_sculpt_entry& en = e.entries[i];
    REQUIRE(en.volume >= 0 && en.volume < d.num_volumes, "sculpt: entry %d: volume %d out of range (%d)", i, en.volume, d.num_volumes);
    bool unsupported;
    if (const char* fault = vpt_sculpt_entry_fault(en, m.volumes[(size_t)en.volume].whd, e.num_stamps, &unsupported))
      return vpt_set_error(unsupported ? VPT_ERR_UNSUPPORTED : VPT_ERR_INVALID_ARG, "sculpt: entry %d: %s", i, fault);
  }
  return VPT_OK;
}

long long region_voxels(const vpt_sculpt_entry& en) { return (long long)en.region_whd[0] * en.region_whd[1] * en.region_whd[2]; }

}  // namespace

int sculpt_apply(resident& r, const vpt_sculpt_edit& e, edit_outcome& out) {
  DScene& d = r.d;
  if (int rc = validate_edit(d, r.m, e)) return rc;
  out.changed = true;   // (an edit without entries too: it starts the counters again)
  if (int rc = begin_update(r)) return rc;
  bool any = false;
  for (int i = 0; i < e.num_entries; i++) any = any || (region_voxels(e.entries[i]) > 0 && e.entries[i].num_stamps > 0);
  device_buffer records;   // gone when the call returns (it ends with the device idle)
  if (any) {
    std::vector<vpt_sculpt_record> host((size_t)e.num_stamps);
    for (int i = 0; i < e.num_stamps; i++) host[(size_t)i] = vpt_sculpt_make_record(e.stamps[i]);
    if (int rc = send(r, records, host)) return rc;
  }
  HIP_TRY(hipEventRecord(r.upd_ev0, 0));
  for (int i = 0; i < e.num_entries; i++) {
    const vpt_sculpt_entry& en = e.entries[i];
    const long long         n  = region_voxels(en);
    if (n == 0 || en.num_stamps == 0) continue;
    const vpt_volume& v = r.m.volumes[(size_t)en.volume];
    sculpt_grid g = {v.whd[0], v.whd[1], en.region_lo[0], en.region_lo[1], en.region_lo[2], en.region_whd[0], en.region_whd[1],
        {en.origin[0], en.origin[1], en.origin[2]}, {en.step[0], en.step[1], en.step[2]}};
    LAUNCH(r, sculpt_kernel, n, mut(d.voxels) + v.offset, g, (unsigned)n, records.get<const vpt_sculpt_record>() + en.first_stamp, en.num_stamps,
        (int)(e.stamps[en.first_stamp].op != VPT_SCULPT_REPLACE));
  }
  if (int rc = mark_end(r)) return rc;
  return finish_update(r);
}
