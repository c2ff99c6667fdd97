// vpt_instance_update.hip — the instances of a resident scene added, removed and re-pointed on the device (include/vpt.h:
// vpt_scene_update_instances).  The instance table changes length and numbering; what is keyed by an instance id
// follows: the scene BVH (built anew over the new list by K6's core, as in vpt_bvh_rebuild.hip, whose scene-level functions this
// unit calls), the enter records and slots, the light list and records (vpt_light_update.hip, with the map new id -> old id).
// Down goes the edit's own payload in ONE copy - the removed ids, the ids of the `set` entries, and one 128-byte record per set or
// added instance, made on the host by prep_instance_frames as creation makes them - then the tables that hang on the new scene
// BVH's topology; up come that BVH's nodes and primitive order.  No node or quad node of a shape crosses: the shapes' part of the
// quad-node table moves device to device, and what the traversal limits need to know of the shapes' trees the handle keeps.
// Everything is built into buffers of the call; tables, counts and mirrors are swapped after the last check.
#include <algorithm>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "vpt_bvh_build.h"
#include "vpt_error.h"
#include "vpt_instance_update.h"
#include "vpt_light_update.h"
#include "vpt_scene_update.h"
#include "vpt_update_helpers.h"

namespace {

// every old instance stays and keeps its record, until iu_mark_kernel says otherwise
__global__ void iu_fill_kernel(int n_old, int* __restrict__ keep, int* __restrict__ set_src) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_old) return;
  keep[i] = 1, set_src[i] = -1;
  if (i == 0) keep[n_old] = 0;   // the scan runs over n_old + 1 entries: its last output is the number of survivors
}
// the removal list clears keep flags, the set list names the staged record that replaces an old one (ids validated on the host)
__global__ void iu_mark_kernel(int n_old, int n_remove, const int* __restrict__ remove_ids, int n_set, const int* __restrict__ set_ids, int* __restrict__ keep,
    int* __restrict__ set_src) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n_remove) {
    const int id = remove_ids[k];
    if (id >= 0 && id < n_old) keep[id] = 0;
  } else if (k - n_remove < n_set) {
    const int id = set_ids[k - n_remove];
    if (id >= 0 && id < n_old) set_src[id] = k - n_remove;
  }
}
// The new DInstance table in one launch.  A record is 128 B = 8 float4: eight adjacent lanes move one record, one float4 each, so a
// wave reads and writes eight whole records contiguously.  Record r < n_old is an old instance: dropped when removed, else gathered
// to scan[r] - from the staged block when the edit set it, from the old table otherwise; record r >= n_old is an added one, appended
// after the n_kept survivors.  new_of_old[r] = the new id of old instance r, -1: removed.
__global__ void iu_gather_kernel(int n_old, int n_add, int n_kept, int n_set, const int* __restrict__ keep, const int* __restrict__ scan,
    const int* __restrict__ set_src, const float4* __restrict__ old_table, const float4* __restrict__ staged, float4* __restrict__ new_table,
    int* __restrict__ new_of_old) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long r = t >> 3;
  const int       part = (int)(t & 7);
  if (r >= (long long)n_old + n_add) return;
  const float4* from;
  long long     to;
  if (r < n_old) {
    const bool stays = keep[r] != 0;
    to = stays ? scan[r] : -1;
    if (part == 0) new_of_old[r] = (int)to;
    if (!stays) return;
    const int s = set_src[r];
    from = s >= 0 && s < n_set ? staged + 8 * (long long)s : old_table + 8 * r;
  } else {
    to   = (long long)n_kept + (r - n_old);
    from = staged + 8 * ((long long)n_set + (r - n_old));
  }
  if (to < 0 || to >= (long long)n_kept + n_add) return;   // (the host validated the lists: never taken)
  new_table[8 * to + part] = from[part];
}

// the record creation uploads for an instance (build_instances, vpt_scene_prep.cpp)
DInstance record_of(const vpt_instance& in, int shape_flags) {
  DInstance d = {};
  prep_instance_frames(in.frame, d.inv, d.fwd, &d.translation_only);
  d.shape = in.shape, d.material = in.material, d.shape_flags = shape_flags;
  return d;
}

int validate_edit(const resident& r, const vpt_instance_edit& e) {
  const DScene&       d = r.d;
  const edit_mirrors& m = r.m;
  if (int rc = check_ids("remove", e.num_remove, e.remove_ids, d.num_instances)) return rc;
  if (int rc = check_ids("set", e.num_set, e.set_ids, e.set, d.num_instances)) return rc;
  REQUIRE(e.num_add >= 0 && (e.num_add == 0 || e.add), "edit: add list is null or has a negative count");
  REQUIRE((long long)d.num_instances - e.num_remove + e.num_add <= 0x7fffffffLL, "edit: more than 2^31 instances");
  std::vector<char> removed((size_t)d.num_instances, 0);
  for (int i = 0; i < e.num_remove; i++) removed[(size_t)e.remove_ids[i]] = 1;
  for (int i = 0; i < e.num_set; i++) REQUIRE(!removed[(size_t)e.set_ids[i]], "edit: set entry %d: instance %d is also removed", i, e.set_ids[i]);
  auto check = [&](const vpt_instance& in, const char* list, int i) {
    REQUIRE(in.shape >= 0 && in.shape < d.num_shapes, "edit: %s entry %d: bad shape", list, i);
    REQUIRE(in.material >= 0 && in.material < d.num_materials, "edit: %s entry %d: bad material", list, i);
    REQUIRE(finite_all(in.frame.x, 12), "edit: %s entry %d: a frame value is not finite", list, i);
    return (int)VPT_OK;
  };
  for (int i = 0; i < e.num_set; i++)
    if (int rc = check(e.set[i], "set", i)) return rc;
  for (int i = 0; i < e.num_add; i++)
    if (int rc = check(e.add[i], "add", i)) return rc;
  // validate(): the texture ids of a material are range-checked once it is bound to a mesh instance
  auto bind = [&](const vpt_instance& in) { return m.textured[(size_t)in.material] ? (int)VPT_OK : prep_check_material(m.materials[(size_t)in.material], in.material, d.num_textures, true); };
  for (int i = 0; i < e.num_set; i++)
    if (int rc = bind(e.set[i])) return rc;
  for (int i = 0; i < e.num_add; i++)
    if (int rc = bind(e.add[i])) return rc;
  return VPT_OK;
}

}  // namespace

int instance_update_apply(resident& r, const vpt_instance_edit& e, edit_outcome& out) {
  DScene&       d = r.d;
  host_mirrors& h = r.h;
  edit_mirrors& m = r.m;
  if (int rc = validate_edit(r, e)) return rc;   // every refusal about the request happens here: nothing has been written
  if (e.num_remove == 0 && e.num_set == 0 && e.num_add == 0) return VPT_OK;
  if (int rc = begin_update(r)) return rc;
  const int n_old = d.num_instances, n_kept = n_old - e.num_remove, n_new = n_kept + e.num_add, n_staged = e.num_set + e.num_add;

  // the new list on the host, the same renumbering in integers: the mirrors of the new scene, and the map the lights follow
  std::vector<int> set_src((size_t)n_old, -1), inst_shape, inst_material, inst_flags, light_old_of_new;
  std::vector<char> keep((size_t)n_old, 1);
  for (int i = 0; i < e.num_remove; i++) keep[(size_t)e.remove_ids[i]] = 0;
  for (int i = 0; i < e.num_set; i++) set_src[(size_t)e.set_ids[i]] = i;
  for (int i = 0; i < n_old; i++) {
    if (!keep[(size_t)i]) continue;
    const int s = set_src[(size_t)i];
    const int shape = s >= 0 ? e.set[s].shape : h.inst_shape[(size_t)i];
    inst_shape.push_back(shape), inst_material.push_back(s >= 0 ? e.set[s].material : m.inst_material[(size_t)i]);
    inst_flags.push_back(m.shape_flags[(size_t)shape]);
    light_old_of_new.push_back(shape == h.inst_shape[(size_t)i] ? i : -1);   // another shape: its CDF is made anew
  }
  for (int i = 0; i < e.num_add; i++) {
    inst_shape.push_back(e.add[i].shape), inst_material.push_back(e.add[i].material), inst_flags.push_back(m.shape_flags[(size_t)e.add[i].shape]);
    light_old_of_new.push_back(-1);
  }

  // the payload in one copy: removed ids, set ids, the records of the set and added instances
  std::vector<DInstance> records((size_t)n_staged);
  for (int i = 0; i < e.num_set; i++) records[(size_t)i] = record_of(e.set[i], m.shape_flags[(size_t)e.set[i].shape]);
  for (int i = 0; i < e.num_add; i++) records[(size_t)e.num_set + (size_t)i] = record_of(e.add[i], m.shape_flags[(size_t)e.add[i].shape]);
  staged_block pay;
  const size_t at_remove = pay.add(e.remove_ids, 4 * (size_t)e.num_remove), at_set = pay.add(e.set_ids, 4 * (size_t)e.num_set);
  const size_t at_records = pay.add(records.data(), records.size() * sizeof(DInstance));
  device_buffer d_block, d_keep, d_scan, d_set_src, d_new_of_old, d_scan_temp, n_instances;
  if (int rc = send(r, d_block, pay.host)) return rc;
  if (int rc = d_keep.allocate(((size_t)n_old + 1) * sizeof(int))) return rc;
  if (int rc = d_scan.allocate(((size_t)n_old + 1) * sizeof(int))) return rc;
  if (int rc = d_set_src.allocate((size_t)n_old * sizeof(int))) return rc;
  if (int rc = d_new_of_old.allocate((size_t)n_old * sizeof(int))) return rc;
  if (int rc = n_instances.allocate((size_t)n_new * sizeof(DInstance))) return rc;
  bvh_build_scratch core;
  if (int rc = core.reserve(std::max(n_new, 1))) return rc;
  HIP_TRY(hipEventRecord(r.upd_ev0, 0));

  // 1. renumbering: keep flags from the removal list, their exclusive scan = the new id of every survivor
  const char* staged = d_block.get<char>();
  LAUNCH(r, iu_fill_kernel, n_old, n_old, d_keep.get<int>(), d_set_src.get<int>());
  LAUNCH(r, iu_mark_kernel, e.num_remove + e.num_set, n_old, e.num_remove, (const int*)(staged + at_remove), e.num_set, (const int*)(staged + at_set), d_keep.get<int>(),
      d_set_src.get<int>());
  if (n_old > 0) {
    size_t scan_bytes = 0;
    HIP_TRY(rocprim::exclusive_scan((void*)nullptr, scan_bytes, d_keep.get<int>(), d_scan.get<int>(), 0, (size_t)n_old + 1, rocprim::plus<int>()));
    if (int rc = d_scan_temp.allocate(scan_bytes)) return rc;
    HIP_TRY(rocprim::exclusive_scan(d_scan_temp.get(), scan_bytes, d_keep.get<int>(), d_scan.get<int>(), 0, (size_t)n_old + 1, rocprim::plus<int>()));
    r.last_launches++;
  }
  // 2. the new instance table: survivors gathered, set and added records from the staged block
  LAUNCH(r, iu_gather_kernel, 8LL * ((long long)n_old + e.num_add), n_old, e.num_add, n_kept, e.num_set, d_keep.get<int>(), d_scan.get<int>(), d_set_src.get<int>(),
      (const float4*)d.instances, (const float4*)(staged + at_records), n_instances.get<float4>(), d_new_of_old.get<int>());

  // 3. the scene BVH over ALL instances of the new list, the read-back of its nodes and primitive order, and the traversal limits by
  // creation's own function: the scene's tree is new, the shapes' are the ones the handle knows.  A tree past a limit is refused here.
  scene_level lv;
  if (int rc = scene_level_build(r, core, n_instances.get<DInstance>(), n_new, d.shapes, lv)) return rc;
  vpt_scene_desc desc = {};
  desc.num_shapes = d.num_shapes;
  desc.num_scene_bvh_nodes = lv.count, desc.scene_bvh_nodes = lv.h_nodes.data();
  scene_tables t;
  t.d = d, t.shapes = m.shapes;
  t.shape_wnodes = (size_t)r.num_shape_wnodes, t.shape_depth = most_of(r.shape_depth), t.shape_need4 = most_of(r.shape_need4);
  if (int rc = prep_quad_nodes_and_stacks(desc, t, true)) return rc;
  // the quad-node table: the scene's part from the host, the shapes' part as it is, device to device
  if (int rc = lv.wnodes.allocate((t.scene_wnodes + t.shape_wnodes) * sizeof(float4))) return rc;
  if (int rc = send(r, lv.wnodes.get<const float4>(), t.wnodes.data(), t.scene_wnodes)) return rc;
  if (t.shape_wnodes) HIP_TRY(hipMemcpy(lv.wnodes.get<float4>() + t.scene_wnodes, d.shape_wnodes, t.shape_wnodes * sizeof(float4), hipMemcpyDeviceToDevice));
  if (int rc = scene_level_enter(r, lv, t, inst_shape.data(), n_instances.get<DInstance>(), d.shapes)) return rc;

  // ---- the last check has passed: the swap of tables, counts and mirrors ------------------------------------------------------
  const void* old_instances = d.instances;
  d.instances = n_instances.get<const DInstance>(), d.num_instances = n_new;
  adopt(r.tables, old_instances, std::move(n_instances));
  scene_level_swap(r, lv, t);
  h.inst_shape = inst_shape, m.inst_material = inst_material, m.inst_flags = inst_flags;
  m.textured.assign((size_t)d.num_materials, 0);
  out.curves = false;
  for (int i = 0; i < n_new; i++) {
    m.textured[(size_t)inst_material[(size_t)i]] = 1;
    out.curves = out.curves || (inst_flags[(size_t)i] & (VPT_SHP_POINTS | VPT_SHP_LINES)) != 0;
  }
  r.varying_media = prep_media_vary(m.materials.data(), d.num_materials, m.inst_material.data(), m.inst_flags.data(), n_new);
  out.changed = out.topology = true, out.stack_cap = t.stack_cap, out.stack_lds4 = t.stack_lds4, out.stack_spill4 = t.stack_spill4;

  // 4. the lights of the new list: a survivor keeps its CDF and search structures under its new id
  const vpt_scene_edit none = {};
  if (int rc = light_update_apply(r, none, &out.lights_rebuilt, nullptr, nullptr, &light_old_of_new)) return rc;
  if (!out.lights_rebuilt)   // the same lights under the same ids: a `set` may still have moved one
    if (int rc = upd_light_records(r, d.shapes)) return rc;
  if (int rc = mark_end(r)) return rc;
  return finish_update(r);
}
