// vpt_scene_inspect.hip — a resident scene's tables as the device holds them now (include/vpt.h: vpt_scene_get_*, the three
// *_tables_hash, vpt_scene_update_stats): what the tests and the measurement tools compare an edited handle against, and the
// camera a session sizes its frame from.  Reads the `resident` part of the handle (vpt_resident.h) and nothing of its render
// side; launches nothing, writes nothing on the device.
#include <cstring>
#include <vector>

#include "vpt_error.h"
#include "vpt_resident.h"

namespace {

// launches on any stream may still write the tables an edit has just handed over
int idle(const resident& r) {
  HIP_TRY(hipSetDevice(r.device));
  HIP_TRY(hipDeviceSynchronize());
  return VPT_OK;
}
// `count` entries of a table into the caller's array, where the caller gave one
template <typename T>
int read_back(T* dst, const void* src, size_t count) {
  if (dst && count) HIP_TRY(hipMemcpy(dst, src, count * sizeof(T), hipMemcpyDeviceToHost));
  return VPT_OK;
}

// FNV-1a over tables read back from the device: every slot of `out` starts at the offset basis, and the parts of a slot continue
// its hash in the order they are listed
struct hashed_part { const void* table; size_t bytes; int slot; };
template <int Parts>
int hash_tables(const resident& r, const hashed_part (&parts)[Parts], uint64_t* out, int slots) {
  if (int rc = idle(r)) return rc;
  for (int k = 0; k < slots; k++) out[k] = 14695981039346656037ull;
  std::vector<unsigned char> host;
  for (const hashed_part& p : parts) {
    host.resize(p.bytes);
    if (int rc = read_back(host.data(), p.table, p.bytes)) return rc;
    uint64_t hash = out[p.slot];
    for (unsigned char b : host) hash = (hash ^ b) * 1099511628211ull;
    out[p.slot] = hash;
  }
  return VPT_OK;
}

}  // namespace

extern "C" {

// the resident camera, for callers that size a frame from it (vpt_session, vpt_session.hip)
int vpt_scene_get_camera(vpt_scene* s, int camera, vpt_camera* out) {
  if (!s || !out) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  const resident& r = resident_of(s);
  if (camera < 0 || camera >= r.d.num_cameras) return vpt_set_error(VPT_ERR_INVALID_ARG, "camera %d out of range", camera);
  HIP_TRY(hipSetDevice(r.device));
  return read_back(out, r.d.cameras + camera, 1);
}

// the three small tables and a volume's voxels
int vpt_scene_get_volumes(vpt_scene* s, vpt_volume* volumes, int volume_capacity, vpt_volume_instance* vol_instances, int instance_capacity, vpt_sdf* sdfs,
    int sdf_capacity) {
  if (!s) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  const DScene& d = resident_of(s).d;
  REQUIRE(!volumes || volume_capacity >= d.num_volumes, "volume_capacity %d < %d volumes", volume_capacity, d.num_volumes);
  REQUIRE(!vol_instances || instance_capacity >= d.num_vol_instances, "instance_capacity %d < %d volume instances", instance_capacity, d.num_vol_instances);
  REQUIRE(!sdfs || sdf_capacity >= d.num_sdfs, "sdf_capacity %d < %d sdfs", sdf_capacity, d.num_sdfs);
  if (int rc = idle(resident_of(s))) return rc;
  if (int rc = read_back(volumes, d.volumes, (size_t)d.num_volumes)) return rc;
  if (int rc = read_back(vol_instances, d.vol_instances, (size_t)d.num_vol_instances)) return rc;
  return read_back(sdfs, d.sdfs, (size_t)d.num_sdfs);
}
int vpt_scene_count_implicit(vpt_scene* s, int32_t counts[3]) {
  if (!s || !counts) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  const DScene& d = resident_of(s).d;
  counts[0] = d.num_volumes, counts[1] = d.num_vol_instances, counts[2] = d.num_sdfs;
  return VPT_OK;
}
int vpt_scene_get_voxels(vpt_scene* s, int volume, float* voxels, int64_t capacity) {
  if (!s || !voxels) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  const DScene& d = resident_of(s).d;
  REQUIRE(volume >= 0 && volume < d.num_volumes, "volume %d out of range (%d)", volume, d.num_volumes);
  if (int rc = idle(resident_of(s))) return rc;
  vpt_volume v;
  if (int rc = read_back(&v, d.volumes + volume, 1)) return rc;
  const long long n = (long long)v.whd[0] * v.whd[1] * v.whd[2];
  REQUIRE(capacity >= n, "capacity %lld < %lld voxels", (long long)capacity, n);
  return read_back(voxels, d.voxels + v.offset, (size_t)n);
}

// the light list and the CDF pool
int vpt_scene_get_lights(vpt_scene* s, vpt_light* lights, int light_capacity, int* num_lights, float* cdf, int64_t cdf_capacity, int64_t* num_cdf) {
  if (!s) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  const resident& r = resident_of(s);
  if (num_lights) *num_lights = r.d.num_lights;
  if (num_cdf) *num_cdf = r.m.num_cdf;
  REQUIRE(!lights || light_capacity >= r.d.num_lights, "light_capacity %d < %d lights", light_capacity, r.d.num_lights);
  REQUIRE(!cdf || cdf_capacity >= r.m.num_cdf, "cdf_capacity %lld < %lld cdf entries", (long long)cdf_capacity, r.m.num_cdf);
  if (int rc = idle(r)) return rc;
  if (int rc = read_back(lights, r.d.lights, (size_t)r.d.num_lights)) return rc;
  return read_back(cdf, r.d.light_cdf, (size_t)r.m.num_cdf);
}

// the medium records
int vpt_scene_get_media(vpt_scene* s, float* records, int capacity, int* num_materials, int* varying) {
  if (!s) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  const resident& r = resident_of(s);
  if (num_materials) *num_materials = r.d.num_materials;
  if (varying) *varying = r.varying_media ? 1 : 0;
  REQUIRE(!records || capacity >= r.d.num_materials, "capacity %d < %d materials", capacity, r.d.num_materials);
  if (int rc = idle(r)) return rc;
  return read_back((float4*)records, r.d.light_rec + 8 * (size_t)r.d.num_lights, 3 * (size_t)r.d.num_materials);
}

// the six light tables: lights, light_cdf, light_rec, light_prims, light_index + its pool, light_guide
int vpt_scene_light_tables_hash(vpt_scene* s, uint64_t out[6]) {
  if (!s || !out) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  const resident& r  = resident_of(s);
  const size_t    nl = (size_t)r.d.num_lights;
  const hashed_part parts[7] = {{r.d.lights, nl * sizeof(vpt_light), 0}, {r.d.light_cdf, (size_t)r.m.num_cdf * sizeof(float), 1},
      {r.d.light_rec, 8 * nl * sizeof(float4), 2}, {r.d.light_prims, 20 * nl * sizeof(float4), 3}, {r.d.light_index, nl * sizeof(DCdfIndex), 4},
      {r.d.light_index_pool, (size_t)r.m.num_pool * sizeof(float), 4}, {r.d.light_guide, (size_t)r.m.num_guide * sizeof(int2), 5}};
  return hash_tables(r, parts, out, 6);
}
// the tables laid out in shape order (include/vpt.h names the eight groups); group 5 is 0 for a scene without compact records
int vpt_scene_shape_tables_hash(vpt_scene* s, uint64_t out[8]) {
  if (!s || !out) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  const resident& r = resident_of(s);
  const DScene&   d = r.d;
  const size_t    slots = r.h.prim_slot.size();
  const hashed_part parts[12] = {{d.shapes, (size_t)d.num_shapes * sizeof(DShape), 0}, {d.positions, (size_t)r.num_positions * sizeof(float4), 1},
      {d.normals, (size_t)r.num_normals * sizeof(float4), 1}, {d.texcoords, (size_t)r.num_texcoords * sizeof(float2), 1},
      {d.colors, (size_t)r.num_colors * sizeof(float4), 1}, {d.elems, slots * sizeof(int4), 2}, {d.leaf_prims, (4 * slots + 8) * sizeof(float4), 3},
      {d.leaf_attrs, 6 * slots * sizeof(float4), 4}, {d.tri_prims, d.tri_prims ? (3 * slots + 8) * sizeof(float4) : 0, 5},
      {d.tri_attrs, d.tri_attrs ? 4 * slots * sizeof(float4) : 0, 5}, {d.shape_nodes, (size_t)r.num_shape_nodes * sizeof(vpt_bvh_node), 6},
      {d.shape_wnodes, (size_t)r.num_shape_wnodes * sizeof(float4), 7}};
  if (int rc = hash_tables(r, parts, out, 8)) return rc;
  if (!d.tri_prims) out[5] = 0;
  return VPT_OK;
}
// the tables keyed by instance id: instances, scene_enter, slot_of_instance, scene_prims
int vpt_scene_instance_tables_hash(vpt_scene* s, uint64_t out[4]) {
  if (!s || !out) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  const DScene& d  = resident_of(s).d;
  const size_t  ni = (size_t)d.num_instances, np = (size_t)d.num_scene_prims;
  const hashed_part parts[4] = {{d.instances, ni * sizeof(DInstance), 0}, {d.scene_enter, 6 * np * sizeof(float4), 1}, {d.slot_of_instance, ni * sizeof(int), 2},
      {d.scene_prims, np * sizeof(int), 3}};
  return hash_tables(resident_of(s), parts, out, 4);
}

int vpt_scene_get_bvh(vpt_scene* s, vpt_bvh_node* scene_nodes, int scene_capacity, vpt_bvh_node* shape_nodes, int64_t shape_capacity) {
  if (!s) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  const resident& r = resident_of(s);
  REQUIRE(!scene_nodes || scene_capacity >= r.d.num_scene_nodes, "scene_capacity %d < %d scene bvh nodes", scene_capacity, r.d.num_scene_nodes);
  REQUIRE(!shape_nodes || shape_capacity >= r.num_shape_nodes, "shape_capacity %lld < %lld shape bvh nodes", (long long)shape_capacity, r.num_shape_nodes);
  if (int rc = idle(r)) return rc;
  if (int rc = read_back(scene_nodes, r.d.scene_nodes, (size_t)r.d.num_scene_nodes)) return rc;
  return read_back(shape_nodes, r.d.shape_nodes, (size_t)r.num_shape_nodes);
}
int vpt_scene_get_bvh_counts(vpt_scene* s, int32_t* scene_nodes, int64_t* shape_nodes, int64_t* shape_node_offsets) {
  if (!s || !scene_nodes || !shape_nodes) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  const resident& r = resident_of(s);
  *scene_nodes = r.d.num_scene_nodes, *shape_nodes = r.num_shape_nodes;
  if (shape_node_offsets)
    for (int i = 0; i < r.d.num_shapes; i++) shape_node_offsets[i] = r.m.shapes[(size_t)i].node_offset;
  return VPT_OK;
}
// the shapes' order is read from the leaf records themselves (the element id in p0.w of every slot): what the traversal reports
int vpt_scene_get_bvh_prims(vpt_scene* s, int32_t* scene_prims, int capacity, int32_t* shape_prims, int64_t shape_capacity) {
  if (!s) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  const resident& r = resident_of(s);
  const long long slots = (long long)r.h.prim_slot.size();
  REQUIRE(!scene_prims || capacity >= r.d.num_scene_prims, "capacity %d < %d scene bvh primitives", capacity, r.d.num_scene_prims);
  REQUIRE(!shape_prims || shape_capacity >= slots, "shape_capacity %lld < %lld shape bvh primitives", (long long)shape_capacity, slots);
  if (int rc = idle(r)) return rc;
  if (int rc = read_back(scene_prims, r.d.scene_prims, (size_t)r.d.num_scene_prims)) return rc;
  if (shape_prims && slots)
    HIP_TRY(hipMemcpy2D(shape_prims, sizeof(int32_t), (const char*)r.d.leaf_prims + 12, 4 * sizeof(float4), sizeof(int32_t), (size_t)slots, hipMemcpyDeviceToHost));
  return VPT_OK;
}

int vpt_scene_get_instances(vpt_scene* s, vpt_instance* out, int capacity, int* num_instances) {
  if (!s) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  const resident& r = resident_of(s);
  if (num_instances) *num_instances = r.d.num_instances;
  if (!out) return VPT_OK;
  REQUIRE(capacity >= r.d.num_instances, "capacity %d < %d instances", capacity, r.d.num_instances);
  if (int rc = idle(r)) return rc;
  std::vector<DInstance> host((size_t)r.d.num_instances);
  if (int rc = read_back(host.data(), r.d.instances, host.size())) return rc;
  for (size_t i = 0; i < host.size(); i++) {
    static_assert(sizeof(vpt_frame) == 3 * sizeof(float4), "a packed frame is the frame's twelve floats in order");
    memcpy(&out[i].frame, host[i].fwd, sizeof(vpt_frame));
    out[i].shape = host[i].shape, out[i].material = host[i].material;
  }
  return VPT_OK;
}
int vpt_scene_get_shape_counts(vpt_scene* s, int32_t* num_shapes, int64_t* num_elements, int64_t* num_vertices) {
  if (!s) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  const resident& r = resident_of(s);
  if (num_shapes) *num_shapes = r.d.num_shapes;
  if (num_elements) *num_elements = (int64_t)r.h.prim_slot.size();
  if (num_vertices) *num_vertices = r.num_positions;
  return VPT_OK;
}

// what the last edit of this handle launched and sent (profiles/tools/scene_update_measure.py)
int vpt_scene_update_stats(const vpt_scene* s, int* launches, int64_t* bytes, float* device_ms) {
  if (!s || !launches || !bytes || !device_ms) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  const resident& r = resident_of(s);
  *launches = r.last_launches, *bytes = r.last_bytes, *device_ms = r.last_ms;
  return VPT_OK;
}

}  // extern "C"
