// vpt_sculpt.cpp — sculpting a voxel grid with analytic SDF brushes on the CPU: the rule of include/vpt.h (vpt_scene_sculpt_volumes)
// through the same header as the kernel (csrc/vpt_sculpt_rule.h), one voxel after another, each through its entry's stamps in list
// order - the statement the kernel is held to bit for bit; and the brush distance and the combination alone, for the tests that pin the six functions and the ops.
#include "vpt_host.h"
#include "vpt_sculpt_rule.h"

namespace vpt {

bool sculpt_volume(volume_data& volume, const vpt_sculpt_entry& e, const vpt_sculpt_stamp* stamps, int num_stamps, string& error) {
  if (num_stamps < 0 || (num_stamps > 0 && !stamps)) return error = "sculpt: the stamp list is null or has a negative count", false;
  for (auto i = 0; i < num_stamps; i++)
    if (auto fault = vpt_sculpt_stamp_fault(stamps[i])) return error = "sculpt: stamp " + std::to_string(i) + ": " + fault, false;
  const int32_t whd[3] = {volume.whd.x, volume.whd.y, volume.whd.z};
  bool unsupported;
  if (auto fault = vpt_sculpt_entry_fault(e, whd, num_stamps, &unsupported)) return error = string{"sculpt: entry 0: "} + fault, false;
  if (volume.vol.size() < (size_t)whd[0] * (size_t)whd[1] * (size_t)whd[2]) return error = "sculpt: entry 0: the volume holds fewer voxels than its whd", false;
  if (e.num_stamps == 0) return true;
  auto records = vector<vpt_sculpt_record>((size_t)e.num_stamps);
  for (auto s = 0; s < e.num_stamps; s++) records[(size_t)s] = vpt_sculpt_make_record(stamps[e.first_stamp + s]);
  for (auto z = 0; z < e.region_whd[2]; z++)
    for (auto y = 0; y < e.region_whd[1]; y++)
      for (auto x = 0; x < e.region_whd[0]; x++) {
        const int  i = e.region_lo[0] + x, j = e.region_lo[1] + y, k = e.region_lo[2] + z;
        const auto p = vpt_sculpt_f3{vpt_sculpt_sample(e.origin[0], e.step[0], i), vpt_sculpt_sample(e.origin[1], e.step[1], j),
            vpt_sculpt_sample(e.origin[2], e.step[2], k)};
        auto& voxel = volume.vol[(size_t)i + (size_t)j * (size_t)whd[0] + (size_t)k * (size_t)whd[0] * (size_t)whd[1]];
        auto  v     = voxel;
        for (auto& r : records) v = vpt_sculpt_stamp_value(r, p, v);
        voxel = v;
      }
  return true;
}

}  // namespace vpt

extern "C" {

// the distance of `brush` (frame and material ignored) at `n` points {x, y, z} of its local frame; -1 for a null pointer or a type outside 0..5
int vpth_sculpt_eval(const vpt_sdf* brush, const float* points, int n, float* out) {
  if (!brush || n < 0 || (n > 0 && (!points || !out)) || brush->type < 0 || brush->type > VPT_SDF_TORUS) return -1;
  const auto record = vpt_sculpt_make_record(vpt_sculpt_stamp{*brush, VPT_SCULPT_REPLACE, 0.0f});
  for (auto i = 0; i < n; i++) out[i] = vpt_sculpt_brush_local(record, {points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]});
  return 0;
}
// the combination alone: out[i] = op(a[i], b[i]) with blend k, a the resident values and b the brush distances; -1 for a null pointer, an op
// outside 0..3 or a blend that is not finite and >= 0
int vpth_sculpt_combine(int op, float k, const float* a, const float* b, int n, float* out) {
  if (n < 0 || (n > 0 && (!a || !b || !out)) || op < VPT_SCULPT_REPLACE || op > VPT_SCULPT_INTERSECT || !std::isfinite(k) || !(k >= 0)) return -1;
  for (auto i = 0; i < n; i++) out[i] = vpt_sculpt_combine(op, k, a[i], b[i]);
  return 0;
}

}  // extern "C"
