// vpt_volume_set.hip — volumes, grid instances and SDFs of a resident scene added and removed (include/vpt.h:
// vpt_scene_update_volume_set).  Data movement and bookkeeping: the lists and the layout of the new voxel pool are
// decided on the host (vpt_volume_set_layout.cpp, no device call), ONE kernel fills the whole new pool from a segment table - survivors
// and copies out of the old pool, host payload out of a staging buffer, fills from a constant - and the bake kernel (vpt_bake.h) writes
// the baked volumes straight into the place the gather left for them.  The records are vpt_scene_prep.cpp's (prep_sdf_records), the
// light tables vpt_light_update.hip's.  Everything is built into buffers of the call and swapped in at the end.
#include <cstring>
#include <memory>
#include <vector>

#include "vpt_bake.h"
#include "vpt_bake_prep.h"
#include "vpt_error.h"
#include "vpt_light_update.h"
#include "vpt_update_helpers.h"
#include "vpt_volume_set.h"
#include "vpt_volume_set_layout.h"

namespace {

constexpr int GATHER_BLOCK = 256;
constexpr int GATHER_CHUNK = 16 * GATHER_BLOCK;   // voxels of the new pool one workgroup owns: 16 KiB, four 16-byte stores per lane

// The whole new pool in one launch.  `segs` tile [0, total) in order of dst, none empty (vpt_volume_set_layout.h).  A workgroup owns
// GATHER_CHUNK voxels of the destination, finds the segment that holds its first voxel by binary search and walks on until its chunk
// ends: every loop is bounded by the chunk (a segment holds at least one voxel).  The new pool is a fresh allocation, so it never
// aliases a source.  Where source and destination of a run have the same phase modulo four voxels - the allocations themselves are
// aligned far beyond 16 bytes - the run is moved as dwords up to the first 16-byte boundary of the destination, as uint4 from there
// and as dwords for what is left; a run whose phases differ (everything behind a volume of 30 voxels) is moved dword by dword.
// Values move as integers: every bit of a NaN survives.
__global__ void __launch_bounds__(GATHER_BLOCK) vol_pool_gather_kernel(unsigned* __restrict__ pool, long long total, const vol_segment* __restrict__ segs, int num_segs,
    const unsigned* __restrict__ old_pool, const unsigned* __restrict__ staging) {
  const long long c0 = (long long)blockIdx.x * GATHER_CHUNK;
  const long long c1 = c0 + GATHER_CHUNK < total ? c0 + GATHER_CHUNK : total;
  if (c0 >= c1) return;
  int first = 0, count = num_segs;   // the first segment that ends behind c0
  while (count > 0) {
    const int half = count >> 1, mid = first + half;
    if (segs[mid].dst + segs[mid].length <= c0) first = mid + 1, count -= half + 1;
    else count = half;
  }
  const int t = (int)threadIdx.x;
  for (int s = first; s < num_segs; s++) {
    const vol_segment seg = segs[s];
    if (seg.dst >= c1) break;
    const long long lo = seg.dst > c0 ? seg.dst : c0;
    const long long hi = seg.dst + seg.length < c1 ? seg.dst + seg.length : c1;
    if (seg.kind == VOL_SEG_BAKE || hi <= lo) continue;
    const int n = (int)(hi - lo);   // <= GATHER_CHUNK
    unsigned* out = pool + lo;
    if (seg.kind == VOL_SEG_CONSTANT) {
      const unsigned v = (unsigned)seg.src;
      int head = (int)((4 - (lo & 3)) & 3);
      head = head < n ? head : n;
      const int body = (n - head) >> 2, tail = n - head - 4 * body;
      if (t < head) out[t] = v;
      uint4* out4 = reinterpret_cast<uint4*>(out + head);
      for (int i = t; i < body; i += GATHER_BLOCK) out4[i] = make_uint4(v, v, v, v);
      if (t < tail) out[head + 4 * body + t] = v;
      continue;
    }
    const long long at = seg.src + (lo - seg.dst);
    const unsigned* in = (seg.kind == VOL_SEG_STAGING ? staging : old_pool) + at;
    if (((lo - at) & 3) == 0) {
      int head = (int)((4 - (lo & 3)) & 3);
      head = head < n ? head : n;
      const int body = (n - head) >> 2, tail = n - head - 4 * body;
      if (t < head) out[t] = in[t];
      uint4*       out4 = reinterpret_cast<uint4*>(out + head);
      const uint4* in4  = reinterpret_cast<const uint4*>(in + head);
      for (int i = t; i < body; i += GATHER_BLOCK) out4[i] = in4[i];
      if (t < tail) out[head + 4 * body + t] = in[head + 4 * body + t];
    } else
      for (int i = t; i < n; i += GATHER_BLOCK) out[i] = in[i];
  }
}

bool same3(const int32_t a[3], const int32_t b[3]) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }

int validate_edit(const DScene& d, const edit_mirrors& m, const vpt_volume_set_edit& e) {
  if (int rc = check_ids("volume_set remove_vol_instance", e.num_remove_vol_instances, e.remove_vol_instance_ids, d.num_vol_instances)) return rc;
  if (int rc = check_ids("volume_set remove_sdf", e.num_remove_sdfs, e.remove_sdf_ids, d.num_sdfs)) return rc;
  if (int rc = check_ids("volume_set remove_volume", e.num_remove_volumes, e.remove_volume_ids, d.num_volumes)) return rc;
  REQUIRE(e.num_add_volumes >= 0 && (e.num_add_volumes == 0 || e.add_volumes), "volume_set: add_volumes is null or has a negative count");
  REQUIRE(e.num_add_vol_instances >= 0 && (e.num_add_vol_instances == 0 || e.add_vol_instances), "volume_set: add_vol_instances is null or has a negative count");
  REQUIRE(e.num_add_sdfs >= 0 && (e.num_add_sdfs == 0 || e.add_sdfs), "volume_set: add_sdfs is null or has a negative count");
  REQUIRE(e.num_voxels >= 0 && (e.num_voxels == 0 || e.voxels), "volume_set: the voxel payload is null or has a negative count");
  std::vector<char> removed((size_t)d.num_volumes, 0), inst_removed((size_t)d.num_vol_instances, 0);
  for (int i = 0; i < e.num_remove_volumes; i++) removed[(size_t)e.remove_volume_ids[i]] = 1;
  for (int i = 0; i < e.num_remove_vol_instances; i++) inst_removed[(size_t)e.remove_vol_instance_ids[i]] = 1;
  const long long num_volumes = (long long)d.num_volumes - e.num_remove_volumes + e.num_add_volumes;
  REQUIRE(num_volumes < (1ll << 31) && (long long)d.num_vol_instances - e.num_remove_vol_instances + e.num_add_vol_instances < (1ll << 31) &&
              (long long)d.num_sdfs - e.num_remove_sdfs + e.num_add_sdfs < (1ll << 31),
      "volume_set: a list would hold 2^31 entries or more");
  for (int i = 0; i < d.num_vol_instances; i++)
    REQUIRE(inst_removed[(size_t)i] || !removed[(size_t)m.vol_instances[(size_t)i].volume], "volume_set: remove_volume: volume %d is still named by vol_instance %d",
        m.vol_instances[(size_t)i].volume, i);
  long long total = 0;
  for (int i = 0; i < d.num_volumes; i++)
    if (!removed[(size_t)i]) total += volume_voxels(m.volumes[(size_t)i].whd);
  for (int i = 0; i < e.num_add_volumes; i++) {
    const vpt_volume_new& v = e.add_volumes[i];
    REQUIRE(std::isfinite(v.res), "volume_set: add_volume entry %d: res is not finite", i);
    REQUIRE(v.whd[0] >= 0 && v.whd[1] >= 0 && v.whd[2] >= 0, "volume_set: add_volume entry %d: negative whd (%d x %d x %d)", i, v.whd[0], v.whd[1], v.whd[2]);
    REQUIRE(volume_whd_ok(v.whd), "volume_set: add_volume entry %d: 2^31 voxels or more", i);
    const long long n = volume_voxels(v.whd);
    total += n;
    REQUIRE(total < (1ll << 62), "volume_set: add_volume entry %d: the voxel pool would exceed 2^62 voxels", i);
    if (v.source == VPT_VOLUME_FROM_HOST) {
      REQUIRE(v.offset >= 0 && v.offset <= e.num_voxels - n, "volume_set: add_volume entry %d: voxels out of range of the edit's payload", i);
    } else if (v.source == VPT_VOLUME_FROM_BAKE) {
      REQUIRE(v.bake, "volume_set: add_volume entry %d: FROM_BAKE without a bake descriptor", i);
      char entry[64];
      snprintf(entry, sizeof(entry), "volume_set: add_volume entry %d: bake", i);
      if (int rc = vpt_bake_validate(v.bake, entry)) return rc;
      REQUIRE(same3(v.bake->whd, v.whd), "volume_set: add_volume entry %d: the bake's whd (%d x %d x %d) is not the entry's", i, v.bake->whd[0], v.bake->whd[1], v.bake->whd[2]);
    } else if (v.source == VPT_VOLUME_COPY) {
      REQUIRE(v.copy_of >= 0 && v.copy_of < d.num_volumes, "volume_set: add_volume entry %d: copy_of %d out of range (%d)", i, v.copy_of, d.num_volumes);
      REQUIRE(same3(v.whd, m.volumes[(size_t)v.copy_of].whd), "volume_set: add_volume entry %d: whd differs from that of volume %d, its source", i, v.copy_of);
    } else
      REQUIRE(v.source == VPT_VOLUME_FILL, "volume_set: add_volume entry %d: source %d is not one of 0..3", i, v.source);
  }
  for (int i = 0; i < e.num_add_vol_instances; i++) {
    const vpt_volume_instance& vi = e.add_vol_instances[i];
    REQUIRE(finite_all((const float*)&vi.frame, 12) && std::isfinite(vi.scalef), "volume_set: add_vol_instance entry %d: a value is not finite", i);
    REQUIRE(vi.volume >= 0 && vi.volume < num_volumes, "volume_set: add_vol_instance entry %d: volume %d out of range (%d after the edit)", i, vi.volume, (int)num_volumes);
    REQUIRE(vi.material >= 0 && vi.material < d.num_materials, "volume_set: add_vol_instance entry %d: material %d out of range (%d)", i, vi.material, d.num_materials);
  }
  for (int i = 0; i < e.num_add_sdfs; i++) {
    const vpt_sdf& f = e.add_sdfs[i];
    REQUIRE(finite_all((const float*)&f.frame, 12) && finite_all(f.whd, 3) && finite_all(f.p, 4), "volume_set: add_sdf entry %d: a value is not finite", i);
    REQUIRE(f.type >= 0 && f.type <= VPT_SDF_TORUS, "volume_set: add_sdf entry %d: type %d is not one of 0..5", i, f.type);
    REQUIRE(f.material >= 0 && f.material < d.num_materials, "volume_set: add_sdf entry %d: material %d out of range (%d)", i, f.material, d.num_materials);
  }
  return VPT_OK;
}

// erase + push_back: the survivors of `old` in order (new_id: old id -> new id, -1 removed), then `add`
template <typename T>
std::vector<T> edited_list(const std::vector<T>& old, const std::vector<int>& new_id, const T* add, int num_add) {
  std::vector<T> out;
  for (size_t i = 0; i < old.size(); i++)
    if (new_id[i] >= 0) out.push_back(old[i]);
  out.insert(out.end(), add, add + num_add);
  return out;
}

}  // namespace

int volume_set_apply(resident& r, const vpt_volume_set_edit& e, edit_outcome& out) {
  DScene&       d = r.d;
  edit_mirrors& m = r.m;
  if (int rc = validate_edit(d, m, e)) return rc;
  if (e.num_remove_vol_instances + e.num_remove_sdfs + e.num_remove_volumes == 0 && e.num_add_volumes + e.num_add_vol_instances + e.num_add_sdfs == 0) return VPT_OK;
  volume_set_plan plan;
  volume_set_plan_make(m.volumes, m.num_voxels, d.num_vol_instances, d.num_sdfs, e, plan);
  REQUIRE((plan.num_voxels + GATHER_CHUNK - 1) / GATHER_CHUNK < (1ll << 31), "volume_set: the voxel pool would exceed 2^43 voxels, the reach of one launch");
  // the bakes' host half and their uploads into buffers of their own: a tree that is too deep is refused here, the scene untouched
  std::vector<std::unique_ptr<bake_job>> bakes((size_t)e.num_add_volumes);
  for (int i = 0; i < e.num_add_volumes; i++) {
    if (e.add_volumes[i].source != VPT_VOLUME_FROM_BAKE) continue;
    char entry[64];
    snprintf(entry, sizeof(entry), "volume_set: add_volume entry %d: bake", i);
    bakes[(size_t)i] = std::make_unique<bake_job>();
    if (int rc = bake_prepare(r.device, e.add_volumes[i].bake, entry, *bakes[(size_t)i])) return rc;
  }
  if (int rc = begin_update(r)) return rc;
  out.changed = true;

  // 1. the lists as the edit leaves them: survivors in order with their volume ids renumbered, then the added entries
  std::vector<vpt_volume_instance> vol_instances = edited_list(m.vol_instances, plan.new_vol_instance, e.add_vol_instances, e.num_add_vol_instances);
  std::vector<vpt_sdf>             sdfs          = edited_list(m.sdfs, plan.new_sdf, e.add_sdfs, e.num_add_sdfs);
  const size_t kept_instances = vol_instances.size() - (size_t)e.num_add_vol_instances;
  for (size_t i = 0; i < kept_instances; i++) vol_instances[i].volume = plan.new_volume[(size_t)vol_instances[i].volume];
  std::vector<int> old_sdf(sdfs.size(), -1);   // new id -> old id
  for (size_t i = 0; i < plan.new_sdf.size(); i++)
    if (plan.new_sdf[i] >= 0) old_sdf[(size_t)plan.new_sdf[i]] = (int)i;

  // 2. the pool: one gather into a fresh allocation, then the bakes into the places it left for them
  device_buffer pool, stage, seg_table;
  if (plan.moves_pool) {
    if (int rc = pool.allocate((size_t)plan.num_voxels * sizeof(float))) return rc;
    bool staged = false;
    for (const vol_segment& s : plan.segments) staged = staged || s.kind == VOL_SEG_STAGING;
    if (staged) {   // the edit's payload, whole and once: 4 bytes per voxel of it, whatever part the FROM_HOST entries name
      if (int rc = stage.allocate((size_t)e.num_voxels * sizeof(float))) return rc;
      if (int rc = send(r, stage.get<const float>(), e.voxels, (size_t)e.num_voxels)) return rc;
    }
    if (int rc = send(r, seg_table, plan.segments)) return rc;
  }
  HIP_TRY(hipEventRecord(r.upd_ev0, 0));
  if (plan.moves_pool && plan.num_voxels > 0) {
    const unsigned blocks = (unsigned)((plan.num_voxels + GATHER_CHUNK - 1) / GATHER_CHUNK);
    hipLaunchKernelGGL(vol_pool_gather_kernel, dim3(blocks), dim3(GATHER_BLOCK), 0, 0, pool.get<unsigned>(), plan.num_voxels, seg_table.get<const vol_segment>(),
        (int)plan.segments.size(), reinterpret_cast<const unsigned*>(d.voxels), stage.get<const unsigned>());
    LAUNCHED(r);
  }
  for (int i = 0; i < e.num_add_volumes; i++) {
    if (!bakes[(size_t)i]) continue;
    const vpt_volume_new& v = e.add_volumes[i];
    const bake_region whole = {{0, 0, 0}, {v.whd[0], v.whd[1], v.whd[2]}, VPT_VOXELS_REPLACE};
    if (int rc = bake_launch(*bakes[(size_t)i], v.bake, pool.get<float>() + plan.added_offset[(size_t)i], &whole, &r.last_launches)) return rc;
    r.last_bytes += bakes[(size_t)i]->bytes;
  }
  if (int rc = mark_end(r)) return rc;

  // 3. the small tables and every record at their new lengths
  DScene nd = d;   // prep_sdf_records writes the scene's ball and the plane count
  std::vector<float4> sdf_inv, fn_rec, grid_rec;
  prep_sdf_records(sdfs.data(), (int)sdfs.size(), plan.volumes.data(), vol_instances.data(), (int)vol_instances.size(), sdf_inv, fn_rec, grid_rec, nd);
  device_buffer b_volumes, b_instances, b_sdfs, b_inv, b_fn, b_grid;
  if (int rc = send(r, b_volumes, plan.volumes)) return rc;
  if (int rc = send(r, b_instances, vol_instances)) return rc;
  if (int rc = send(r, b_sdfs, sdfs)) return rc;
  if (int rc = send(r, b_inv, sdf_inv)) return rc;
  if (int rc = send(r, b_fn, fn_rec)) return rc;
  if (int rc = send(r, b_grid, grid_rec)) return rc;
  HIP_TRY(hipDeviceSynchronize());   // the last check: the gather and the bakes have run, nothing reads the old tables

  // 4. the handle
  const void* was[7] = {d.volumes, d.vol_instances, d.sdfs, d.sdf_inv, d.sdf_fn_rec, d.sdf_grid_rec, d.voxels};
  nd.volumes = b_volumes.get<vpt_volume>(), nd.vol_instances = b_instances.get<vpt_volume_instance>(), nd.sdfs = b_sdfs.get<vpt_sdf>();
  nd.sdf_inv = b_inv.get<float4>(), nd.sdf_fn_rec = b_fn.get<float4>(), nd.sdf_grid_rec = b_grid.get<float4>();
  nd.num_volumes = (int)plan.volumes.size(), nd.num_vol_instances = (int)vol_instances.size(), nd.num_sdfs = (int)sdfs.size();
  if (plan.moves_pool) nd.voxels = pool.get<float>();
  d = nd;
  device_buffer* fresh[7] = {&b_volumes, &b_instances, &b_sdfs, &b_inv, &b_fn, &b_grid, &pool};
  for (int k = 0; k < (plan.moves_pool ? 7 : 6); k++) adopt(r.tables, was[k], std::move(*fresh[k]));
  m.volumes = plan.volumes, m.vol_instances = vol_instances, m.sdfs = sdfs, m.num_voxels = plan.num_voxels;

  // 5. the lights: only when the SDF list changed, and then only when the SDF lights are others or carry other ids (light_update_apply decides)
  if (e.num_remove_sdfs > 0 || e.num_add_sdfs > 0) {
    if (int rc = light_update_apply(r, vpt_scene_edit{}, &out.lights_rebuilt, nullptr, nullptr, nullptr, &old_sdf)) return rc;
    if (out.lights_rebuilt)
      if (int rc = mark_end(r)) return rc;   // again: the time includes the rebuild
  }
  return finish_update(r);
}
