// vpt_volume_update.hip — volumes, grid instances and SDFs of a resident scene edited in place (include/vpt.h: vpt_scene_update_volumes;
// DESIGN.md §17).  Voxels are payload: they go where vpt_scene_create would have put them (a volume that changes whd: at the end of a
// pool allocated anew), from a staging buffer through one kernel per region, or straight out of the bake kernel (vpt_bake.h).  There is
// no arithmetic here beyond op_union's select: the records are vpt_scene_prep.cpp's (prep_sdf_records, the function creation calls),
// the light tables vpt_light_update.hip's.
#include <cstring>
#include <memory>
#include <vector>

#include "vpt_bake.h"
#include "vpt_bake_prep.h"
#include "vpt_error.h"
#include "vpt_update_helpers.h"
#include "vpt_volume_update.h"

namespace {

// one lane per voxel of the region (n < 2^31 of them, x fastest): REPLACE writes the incoming value, UNION op_union(resident, incoming)
__global__ void vol_region_kernel(float* __restrict__ grid, int w, int h, int lo_x, int lo_y, int lo_z, int rw, int rh, unsigned n, int mode,
    const float* __restrict__ incoming) {
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;   // the last block's lanes stay below 2^32
  if (idx >= n) return;
  const unsigned x = idx % (unsigned)rw, y = (idx / (unsigned)rw) % (unsigned)rh, z = idx / ((unsigned)rw * (unsigned)rh);
  const size_t   at = (size_t)(lo_x + (int)x) + (size_t)(lo_y + (int)y) * (size_t)w + (size_t)(lo_z + (int)z) * (size_t)w * (size_t)h;
  float v = incoming[idx];
  if (mode == VPT_VOXELS_UNION) {   // yocto_sdfs.h:82 with a the resident value: the select, never fminf (NaN: the select decides)
    const float a = grid[at];
    v = (a < v) ? a : v;
  }
  grid[at] = v;
}

// of dimensions already known to be >= 0 and to multiply to less than 2^31 (voxel_count_ok)
long long product(const int32_t v[3]) { return (long long)v[0] * v[1] * v[2]; }
// whd >= 0 with a product below 2^31, factor by factor: every partial product stays below 2^62, so nothing overflows on the way
bool voxel_count_ok(const int32_t v[3]) {
  if (v[0] < 0 || v[1] < 0 || v[2] < 0) return false;
  if (v[0] == 0 || v[1] == 0 || v[2] == 0) return true;
  long long n = 1;
  for (int k = 0; k < 3; k++) {
    n *= v[k];
    if (n >= (1ll << 31)) return false;
  }
  return true;
}
bool same3(const int32_t a[3], const int32_t b[3]) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }

int validate_edit(const DScene& d, const edit_mirrors& m, const vpt_volume_edit& e) {
  if (int rc = check_ids("vol_instance", e.num_vol_instances, e.vol_instance_ids, e.vol_instances, d.num_vol_instances)) return rc;
  if (int rc = check_ids("sdf", e.num_sdfs, e.sdf_ids, e.sdfs, d.num_sdfs)) return rc;
  if (int rc = check_ids("volume", e.num_volumes, e.volume_ids, e.volumes, d.num_volumes)) return rc;
  REQUIRE(e.num_voxels >= 0 && (e.num_voxels == 0 || e.voxels), "edit: the voxel pool is null or has a negative count");
  for (int i = 0; i < e.num_vol_instances; i++) {
    const vpt_volume_instance& vi = e.vol_instances[i];
    REQUIRE(finite_all((const float*)&vi.frame, 12) && std::isfinite(vi.scalef), "edit: vol_instance entry %d: a value is not finite", i);
    REQUIRE(vi.volume >= 0 && vi.volume < d.num_volumes, "edit: vol_instance entry %d: volume %d out of range (%d)", i, vi.volume, d.num_volumes);
    REQUIRE(vi.material >= 0 && vi.material < d.num_materials, "edit: vol_instance entry %d: material %d out of range (%d)", i, vi.material, d.num_materials);
  }
  for (int i = 0; i < e.num_sdfs; i++) {
    const vpt_sdf& f = e.sdfs[i];
    REQUIRE(finite_all((const float*)&f.frame, 12) && finite_all(f.whd, 3) && finite_all(f.p, 4), "edit: sdf entry %d: a value is not finite", i);
    REQUIRE(f.type >= 0 && f.type <= VPT_SDF_TORUS, "edit: sdf entry %d: type %d is not one of 0..5", i, f.type);
    REQUIRE(f.material >= 0 && f.material < d.num_materials, "edit: sdf entry %d: material %d out of range (%d)", i, f.material, d.num_materials);
  }
  for (int i = 0; i < e.num_volumes; i++) {
    const vpt_volume_source& v   = e.volumes[i];
    const vpt_volume&        was = m.volumes[(size_t)e.volume_ids[i]];
    REQUIRE(std::isfinite(v.res), "edit: volume entry %d: res is not finite", i);
    REQUIRE(v.whd[0] >= 0 && v.whd[1] >= 0 && v.whd[2] >= 0, "edit: volume entry %d: negative whd (%d x %d x %d)", i, v.whd[0], v.whd[1], v.whd[2]);
    REQUIRE(voxel_count_ok(v.whd), "edit: volume entry %d: 2^31 voxels or more", i);
    for (int k = 0; k < 3; k++)
      REQUIRE(v.region_lo[k] >= 0 && v.region_whd[k] >= 0 && (long long)v.region_lo[k] + v.region_whd[k] <= v.whd[k],
          "edit: volume entry %d: the region leaves the grid on axis %d (%d + %d of %d)", i, k, v.region_lo[k], v.region_whd[k], v.whd[k]);
    REQUIRE(v.mode == VPT_VOXELS_REPLACE || v.mode == VPT_VOXELS_UNION, "edit: volume entry %d: mode %d is neither REPLACE nor UNION", i, v.mode);
    if (!same3(v.whd, was.whd))
      REQUIRE(same3(v.region_whd, v.whd) && v.mode == VPT_VOXELS_REPLACE, "edit: volume entry %d: a new whd needs the whole grid as its region, in REPLACE mode", i);
    if (v.offset == -1) {
      REQUIRE(v.bake, "edit: volume entry %d: offset -1 (baked) without a bake descriptor", i);
      char entry[64];
      snprintf(entry, sizeof(entry), "edit: volume entry %d: bake", i);
      if (int rc = vpt_bake_validate(v.bake, entry)) return rc;
      REQUIRE(same3(v.bake->whd, v.whd), "edit: volume entry %d: the bake's whd (%d x %d x %d) is not the entry's", i, v.bake->whd[0], v.bake->whd[1], v.bake->whd[2]);
    } else {
      // (the region lies inside whd: fewer than 2^31 voxels, and the comparison is written so that no offset can overflow it)
      REQUIRE(v.offset >= 0 && v.offset <= e.num_voxels - product(v.region_whd), "edit: volume entry %d: voxels out of range of the edit's pool", i);
    }
  }
  return VPT_OK;
}

}  // namespace

int volume_update_apply(resident& r, const vpt_volume_edit& e, edit_outcome& out) {
  DScene&       d = r.d;
  edit_mirrors& m = r.m;
  if (int rc = validate_edit(d, m, e)) return rc;
  // the bakes' host half and their uploads into buffers of their own: a tree that is too deep is refused here, the scene untouched
  std::vector<std::unique_ptr<bake_job>> bakes((size_t)(e.num_volumes > 0 ? e.num_volumes : 0));
  for (int i = 0; i < e.num_volumes; i++) {
    if (e.volumes[i].offset != -1) continue;
    char entry[64];
    snprintf(entry, sizeof(entry), "edit: volume entry %d: bake", i);
    bakes[(size_t)i] = std::make_unique<bake_job>();
    if (int rc = bake_prepare(r.device, e.volumes[i].bake, entry, *bakes[(size_t)i])) return rc;
  }
  out.changed = true;   // (an edit without entries too: it starts the counters again and sends every SDF record)
  if (int rc = begin_update(r)) return rc;

  // 1. volumes: in place where whd stays, else at the end of a pool that grows
  std::vector<vpt_volume> volumes = m.volumes;
  long long more = 0;
  for (int i = 0; i < e.num_volumes; i++) {
    const vpt_volume_source& src = e.volumes[i];
    vpt_volume&              v   = volumes[(size_t)e.volume_ids[i]];
    const bool regrown = !same3(src.whd, v.whd);
    memcpy(v.whd, src.whd, sizeof(v.whd)), v.res = src.res;
    if (regrown) v.offset = m.num_voxels + more, more += product(src.whd);
  }
  if (more > 0)
    if (int rc = grow_pool(r, d.voxels, m.num_voxels, more)) return rc;
  device_buffer stage;   // the edit's voxels on their way into the pool: gone when the call returns (it ends with the device idle)
  if (e.num_voxels > 0) {
    if (int rc = stage.allocate((size_t)e.num_voxels * sizeof(float))) return rc;
    HIP_TRY(hipMemcpy(stage.get(), e.voxels, (size_t)e.num_voxels * sizeof(float), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipEventRecord(r.upd_ev0, 0));
  for (int i = 0; i < e.num_volumes; i++) {
    const vpt_volume_source& src = e.volumes[i];
    const vpt_volume&        v   = volumes[(size_t)e.volume_ids[i]];
    float* grid = mut(d.voxels) + v.offset;
    if (src.offset == -1) {
      const bake_region region = {{src.region_lo[0], src.region_lo[1], src.region_lo[2]},
          {src.region_lo[0] + src.region_whd[0], src.region_lo[1] + src.region_whd[1], src.region_lo[2] + src.region_whd[2]}, src.mode};
      if (int rc = bake_launch(*bakes[(size_t)i], src.bake, grid, &region, &r.last_launches)) return rc;
      r.last_bytes += bakes[(size_t)i]->bytes;
      continue;
    }
    const long long n = product(src.region_whd);
    LAUNCH(r, vol_region_kernel, n, grid, v.whd[0], v.whd[1], src.region_lo[0], src.region_lo[1], src.region_lo[2], src.region_whd[0], src.region_whd[1], (unsigned)n,
        src.mode, stage.get<float>() + src.offset);
    r.last_bytes += n * (long long)sizeof(float);
  }
  if (int rc = mark_end(r)) return rc;

  // 2. the small tables as the edit leaves them, and every record from them
  std::vector<vpt_volume_instance> vol_instances = m.vol_instances;
  std::vector<vpt_sdf>             sdfs          = m.sdfs;
  std::vector<char>                resized((size_t)d.num_sdfs, 0);
  bool lights_differ = false;
  for (int i = 0; i < e.num_vol_instances; i++) vol_instances[(size_t)e.vol_instance_ids[i]] = e.vol_instances[i];
  for (int i = 0; i < e.num_sdfs; i++) {
    vpt_sdf& f = sdfs[(size_t)e.sdf_ids[i]];
    const bool was_lit = emissive(m.materials[(size_t)f.material]), lit = emissive(m.materials[(size_t)e.sdfs[i].material]);
    resized[(size_t)e.sdf_ids[i]] = memcmp(f.whd, e.sdfs[i].whd, 8) != 0;   // the CDF entry is whd.x * whd.y
    lights_differ = lights_differ || was_lit != lit || (lit && resized[(size_t)e.sdf_ids[i]]);
    f = e.sdfs[i];
  }
  for (int i = 0; i < e.num_volumes; i++)
    if (int rc = send(r, d.volumes + e.volume_ids[i], &volumes[(size_t)e.volume_ids[i]], 1)) return rc;
  for (int i = 0; i < e.num_vol_instances; i++)
    if (int rc = send(r, d.vol_instances + e.vol_instance_ids[i], &e.vol_instances[i], 1)) return rc;
  for (int i = 0; i < e.num_sdfs; i++)
    if (int rc = send(r, d.sdfs + e.sdf_ids[i], &e.sdfs[i], 1)) return rc;
  std::vector<float4> sdf_inv, fn_rec, grid_rec;
  prep_sdf_records(sdfs.data(), d.num_sdfs, volumes.data(), vol_instances.data(), d.num_vol_instances, sdf_inv, fn_rec, grid_rec, d);
  if (int rc = send(r, d.sdf_inv, sdf_inv.data(), sdf_inv.size())) return rc;
  if (int rc = send(r, d.sdf_fn_rec, fn_rec.data(), fn_rec.size())) return rc;
  if (int rc = send(r, d.sdf_grid_rec, grid_rec.data(), grid_rec.size())) return rc;
  m.volumes = volumes, m.vol_instances = vol_instances, m.sdfs = sdfs;

  // 3. the lights: only when the SDF lights of the edited scene are others, or one of them has another whd
  if (lights_differ) {
    if (int rc = light_update_apply(r, vpt_scene_edit{}, &out.lights_rebuilt, nullptr, &resized)) return rc;   // no vertex moved
    if (int rc = mark_end(r)) return rc;   // again: the time includes the rebuild
  }
  return finish_update(r);
}
