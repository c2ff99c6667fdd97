// vpt_scene_update.hip — editing a resident scene (include/vpt.h: vpt_scene_update): validation of a
// vpt_scene_edit and the kernels that rewrite the tables K1 and K2 read.  Only the edit's own payload crosses PCIe (cameras,
// materials, frames with their host-made inverses, moved vertices); leaf records, node boxes, quad nodes, root boxes, enter
// records, light records and instance boxes are derived on the device from what is resident.  The layouts are those of
// vpt_device.h as vpt_scene_prep.cpp builds them: every kernel here copies or recomputes VALUES inside records whose shape,
// order and integer fields creation decided.
// The refit rule (include/vpt.h) is the reference's refit_bvh (yocto_bvh.cpp:510-524): select-form min / max in slot order,
// children `start` then `start + 1`.  Levels run deepest first, one launch per level with stream order as the only barrier; the
// narrow top levels run in one single-workgroup launch with __syncthreads() between levels.  No float atomics, no hand-off
// between workgroups inside a launch.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vpt_error.h"
#include "vpt_launch.h"
#include "vpt_record_bounds.hip.h"
#include "vpt_scene_update.h"
#include "vpt_update_helpers.h"

namespace {

__device__ inline box3 invalid_box() {
  const float m = 3.402823466e+38f;
  return {{m, m, m}, {-m, -m, -m}};
}
__device__ inline box3 merge(box3 a, const box3& b) {
  for (int c = 0; c < 3; c++) a.lo[c] = sel_min(a.lo[c], b.lo[c]), a.hi[c] = sel_max(a.hi[c], b.hi[c]);
  return a;
}
__device__ inline box3 merge_point(box3 a, float x, float y, float z) {
  a.lo[0] = sel_min(a.lo[0], x), a.lo[1] = sel_min(a.lo[1], y), a.lo[2] = sel_min(a.lo[2], z);
  a.hi[0] = sel_max(a.hi[0], x), a.hi[1] = sel_max(a.hi[1], y), a.hi[2] = sel_max(a.hi[2], z);
  return a;
}
// a binary node is 2 x float4: {min.xyz, max.x} {max.yz, start, num | axis << 16 | internal << 24}
__device__ inline box3 node_box(const float4* nodes, long long i) {
  float4 a = nodes[2 * i], b = nodes[2 * i + 1];
  return {{a.x, a.y, a.z}, {a.w, b.x, b.y}};
}
__device__ inline void store_node_box(float4* nodes, long long i, const box3& b) {
  nodes[2 * i] = make_float4(b.lo[0], b.lo[1], b.lo[2], b.hi[0]);
  float4 t = nodes[2 * i + 1];
  t.x = b.hi[1], t.y = b.hi[2];
  nodes[2 * i + 1] = t;
}
__device__ inline int node_start(const float4* nodes, long long i) { return __float_as_int(nodes[2 * i + 1].z); }
__device__ inline int node_meta(const float4* nodes, long long i) { return __float_as_int(nodes[2 * i + 1].w); }

// ---- kernels --------------------------------------------------------------------------------------------------------------
// float3 in, the pools' float4 out (w = 0, as build_geometry leaves it)
__global__ void upd_scatter_vertices_kernel(float4* __restrict__ pool, const float* __restrict__ src, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) pool[i] = make_float4(src[3 * i], src[3 * i + 1], src[3 * i + 2], 0);
}

// One thread per leaf slot of a shape: the corners through elems and positions into every form the scene keeps of the record.
// Element id (p0.w), record kind (p3.w), radii and texcoords are creation's and stay.
__global__ void upd_leaf_records_kernel(DShape sh, const int4* __restrict__ elems, const float4* __restrict__ positions, const float4* __restrict__ normals,
    float4* __restrict__ leaf_prims, float4* __restrict__ leaf_attrs, float4* __restrict__ tri_prims, float4* __restrict__ tri_attrs) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= sh.num_elems) return;
  const long long slot = (long long)sh.leaf_offset + k;
  float4* r = leaf_prims + 4 * slot;
  const int e = __float_as_int(r[0].w), kind = __float_as_int(r[3].w);
  const int4 q = elems[(long long)sh.elem_offset + e];
  const int v[4] = {q.x, q.y, q.z, q.w};
  const float4* P = positions + sh.vertex_offset;
  const int corners = kind == VPT_LEAF_POINT ? 1 : kind == VPT_LEAF_LINE ? 2 : 4;
  for (int c = 0; c < corners; c++) {
    float4 p = P[v[c]];
    p.w = c == 0 ? __int_as_float(e) : c == 3 ? __int_as_float(kind) : 0.0f;   // faces: p3.w is the kind, 0
    r[c] = p;
  }
  float4* a = leaf_attrs + 6 * slot;
  if (sh.normal_offset >= 0)
    for (int c = 0; c < 4; c++) a[c] = normals[(long long)sh.normal_offset + v[c]];
  if (tri_prims) {   // the compact records of a scene of triangles, beside the general ones (vpt_device.h)
    for (int c = 0; c < 3; c++) tri_prims[3 * slot + c] = r[c];
    if (sh.normal_offset >= 0)
      for (int c = 0; c < 3; c++) {
        float4 t = tri_attrs[4 * slot + c], n = a[c];
        tri_attrs[4 * slot + c] = make_float4(n.x, n.y, n.z, t.w);
      }
  }
}

// DShape::root_box of every shape from its root node
__global__ void upd_shape_roots_kernel(DShape* __restrict__ shapes, int num_shapes, const float4* __restrict__ shape_nodes) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_shapes || shapes[i].num_nodes <= 0) return;
  box3 b = node_box(shape_nodes, shapes[i].node_offset);
  for (int c = 0; c < 3; c++) shapes[i].root_box[c] = b.lo[c], shapes[i].root_box[3 + c] = b.hi[c];
}

// leaves of a shape BVH: invalidb3f merged with the primitives' bounds in slot order
__global__ void upd_refit_shape_leaves_kernel(float4* __restrict__ nodes, long long base, int count, const float4* __restrict__ leaf_prims, long long leaf_offset) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int meta = node_meta(nodes, base + i);
  if ((meta >> 24) & 255) return;
  const int start = node_start(nodes, base + i), num = meta & 0xffff;
  box3 b = invalid_box();
  for (int k = 0; k < num; k++) b = merge(b, record_bounds(leaf_prims + 4 * (leaf_offset + start + k)));
  store_node_box(nodes, base + i, b);
}
// the bounds of a shape's elements in ELEMENT order, the input of a rebuild (vpt_bvh_rebuild.hip), from its leaf records: slot k holds
// element p0.w; old_slot[element] = k, the map the rebuild gathers the records through
__global__ void upd_element_boxes_kernel(const float4* __restrict__ leaf_prims, long long leaf_offset, int num_elems, float* __restrict__ boxes, int* __restrict__ old_slot) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= num_elems) return;
  const float4* r = leaf_prims + 4 * (leaf_offset + k);
  const int e = __float_as_int(r[0].w);
  if (e < 0 || e >= num_elems) return;   // (creation checked the primitive order)
  const box3 b = record_bounds(r);
  for (int c = 0; c < 3; c++) boxes[6 * (long long)e + c] = b.lo[c], boxes[6 * (long long)e + 3 + c] = b.hi[c];
  old_slot[e] = k;
}
// leaves of the scene BVH: the instances' boxes through scene_prims
__global__ void upd_refit_scene_leaves_kernel(float4* __restrict__ nodes, int count, const int* __restrict__ prims, const float4* __restrict__ inst_box) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int meta = node_meta(nodes, i);
  if ((meta >> 24) & 255) return;
  const int start = node_start(nodes, i), num = meta & 0xffff;
  box3 b = invalid_box();
  for (int k = 0; k < num; k++) b = merge(b, node_box(inst_box, prims[start + k]));
  store_node_box(nodes, i, b);
}
__device__ inline void refit_internal(float4* nodes, long long base, int i) {
  const long long c = base + node_start(nodes, base + i);
  store_node_box(nodes, base + i, merge(merge(invalid_box(), node_box(nodes, c)), node_box(nodes, c + 1)));
}
// one level of internal nodes (their children are leaves or belong to a level an earlier launch finished)
__global__ void upd_refit_level_kernel(float4* nodes, long long base, const int* __restrict__ order, int count) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < count) refit_internal(nodes, base, order[t]);
}
// The levels above `levels` (exclusive), deepest first, by ONE workgroup: first[l] .. first[l + 1] index `order`.
enum { UPD_TOP_LEVELS = 24, UPD_TOP_WIDTH = 256 };
struct top_levels { int first[UPD_TOP_LEVELS + 1]; };
__global__ void __launch_bounds__(UPD_TOP_WIDTH) upd_refit_top_kernel(float4* nodes, long long base, const int* __restrict__ order, top_levels lv, int levels) {
  for (int l = levels - 1; l >= 0; l--) {
    for (int t = lv.first[l] + (int)threadIdx.x; t < lv.first[l + 1]; t += UPD_TOP_WIDTH) refit_internal(nodes, base, order[t]);
    __syncthreads();   // the level's boxes are written before the one above reads them (one workgroup: workgroup scope is enough)
  }
}

// quad nodes (build_quad_nodes): lo.x[4], lo.y[4], lo.z[4], hi.x[4], hi.y[4], hi.z[4] gathered from the binary nodes behind the
// four slots; empty slots keep their zeros, references and axes are untouched
__global__ void upd_quad_gather_kernel(float4* __restrict__ wnodes, const int4* __restrict__ slots, int count, const float4* __restrict__ nodes, long long base) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= count) return;
  const int4 s4 = slots[n];
  const int  s[4] = {s4.x, s4.y, s4.z, s4.w};
  float v[6][4];
  for (int c = 0; c < 6; c++) {
    float4 q = wnodes[8 * (long long)n + c];
    v[c][0] = q.x, v[c][1] = q.y, v[c][2] = q.z, v[c][3] = q.w;
  }
  for (int k = 0; k < 4; k++) {
    if (s[k] < 0) continue;
    box3 b = node_box(nodes, base + s[k]);
    for (int c = 0; c < 3; c++) v[c][k] = b.lo[c], v[3 + c][k] = b.hi[c];
  }
  for (int c = 0; c < 6; c++) wnodes[8 * (long long)n + c] = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
}

struct inst_payload {   // one edited instance: the frames prep_instance_frames packs
  float4 inv[3], fwd[3];
  int    id, translation_only, pad[2];
};
__global__ void upd_scatter_instances_kernel(DInstance* __restrict__ instances, const inst_payload* __restrict__ in, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  DInstance& d = instances[in[i].id];
  for (int k = 0; k < 3; k++) d.inv[k] = in[i].inv[k], d.fwd[k] = in[i].fwd[k];
  d.translation_only = in[i].translation_only;
}
// transform_bbox(frame, root box), yocto_geometry.h:441-451: the eight corners, z fastest, each through transform_point
// (f.x * p.x + f.y * p.y + f.z * p.z + f.o, yocto_math.h:3097), merged into invalidb3f in that order
__global__ void upd_instance_boxes_kernel(const DInstance* __restrict__ instances, int n, const DShape* __restrict__ shapes, float4* __restrict__ inst_box) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const DInstance& in = instances[i];
  const DShape&    sh = shapes[in.shape];
  box3 b = invalid_box();
  if (sh.num_nodes > 0) {
    // packed frame: {x.x, x.y, x.z, y.x} {y.y, y.z, z.x, z.y} {z.z, o.x, o.y, o.z}
    const float4 f0 = in.fwd[0], f1 = in.fwd[1], f2 = in.fwd[2];
    const float fx[3] = {f0.x, f0.y, f0.z}, fy[3] = {f0.w, f1.x, f1.y}, fz[3] = {f1.z, f1.w, f2.x}, fo[3] = {f2.y, f2.z, f2.w};
    for (int cx = 0; cx < 2; cx++)
      for (int cy = 0; cy < 2; cy++)
        for (int cz = 0; cz < 2; cz++) {
          const float px = sh.root_box[cx ? 3 : 0], py = sh.root_box[cy ? 4 : 1], pz = sh.root_box[cz ? 5 : 2];
          float w[3];
          for (int c = 0; c < 3; c++) w[c] = ((fx[c] * px + fy[c] * py) + fz[c] * pz) + fo[c];
          b = merge_point(b, w[0], w[1], w[2]);
        }
  }
  inst_box[2 * i]     = make_float4(b.lo[0], b.lo[1], b.lo[2], b.hi[0]);
  inst_box[2 * i + 1] = make_float4(b.hi[1], b.hi[2], 0, 0);
}
// enter records (build_instances): e0..e2 inverse frame, e3 / e4.xy the shape's root box, e5.z translation_only; the rest is topology
__global__ void upd_enter_records_kernel(float4* __restrict__ enter, int slots, const DInstance* __restrict__ instances, const DShape* __restrict__ shapes) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= slots) return;
  float4* e = enter + 6 * (long long)k;
  const DInstance& in = instances[__float_as_int(e[5].y)];
  const DShape&    sh = shapes[in.shape];
  e[0] = in.inv[0], e[1] = in.inv[1], e[2] = in.inv[2];
  e[3] = make_float4(sh.root_box[0], sh.root_box[1], sh.root_box[2], sh.root_box[3]);
  float4 e4 = e[4], e5 = e[5];
  e4.x = sh.root_box[4], e4.y = sh.root_box[5], e5.z = __int_as_float(in.translation_only);
  e[4] = e4, e[5] = e5;
}
// light records of mesh lights (build_lights): frames of the instance, root box of its shape; area, kind and count stay
__global__ void upd_light_records_kernel(float4* __restrict__ light_rec, const vpt_light* __restrict__ lights, int n, const DInstance* __restrict__ instances,
    const DShape* __restrict__ shapes) {
  int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= n || lights[l].instance < 0) return;
  const DInstance& in = instances[lights[l].instance];
  const DShape&    sh = shapes[in.shape];
  float4* r = light_rec + 8 * (long long)l;
  for (int k = 0; k < 3; k++) r[k] = in.inv[k], r[3 + k] = in.fwd[k];
  r[6] = make_float4(sh.root_box[0], sh.root_box[1], sh.root_box[2], r[6].w);
  r[7] = make_float4(sh.root_box[3], sh.root_box[4], sh.root_box[5], r[7].w);
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// internal nodes by depth.  validate() made every child index larger than its parent's, so one forward pass gives every depth.
void make_levels(const vpt_bvh_node* nodes, int count, bvh_levels& lv, std::vector<int>& order) {
  lv.first.clear(), lv.offset = (long long)order.size();
  std::vector<int> depth((size_t)(count > 0 ? count : 0), 0);
  int deepest = -1;
  for (int i = 0; i < count; i++) {
    if (!nodes[i].internal) continue;
    for (int c = nodes[i].start; c <= nodes[i].start + 1; c++)
      if (depth[(size_t)c] < depth[(size_t)i] + 1) depth[(size_t)c] = depth[(size_t)i] + 1;
    if (depth[(size_t)i] > deepest) deepest = depth[(size_t)i];
  }
  if (deepest < 0) return;
  lv.first.assign((size_t)deepest + 2, 0);
  for (int i = 0; i < count; i++)
    if (nodes[i].internal) lv.first[(size_t)depth[(size_t)i] + 1]++;
  for (size_t l = 1; l < lv.first.size(); l++) lv.first[l] += lv.first[l - 1];
  std::vector<int> at(lv.first.begin(), lv.first.end() - 1);
  order.resize((size_t)lv.offset + (size_t)lv.first.back());
  for (int i = 0; i < count; i++)
    if (nodes[i].internal) order[(size_t)lv.offset + (size_t)at[(size_t)depth[(size_t)i]]++] = i;
}

template <typename T>
int read_back(std::vector<T>& out, const T* dev, size_t count) {
  out.resize(count);
  if (count) HIP_TRY(hipMemcpy(out.data(), dev, count * sizeof(T), hipMemcpyDeviceToHost));
  return VPT_OK;
}

// what a refit needs beyond the tables themselves, from the node arrays the device holds (once per handle, before its first refit)
int refit_tables_init(const resident& r, refit_tables& u) {
  const DScene& d = r.d;
  std::vector<vpt_bvh_node> scene_nodes, shape_nodes;
  if (int rc = read_back(scene_nodes, (const vpt_bvh_node*)d.scene_nodes, (size_t)d.num_scene_nodes)) return rc;
  if (int rc = read_back(shape_nodes, (const vpt_bvh_node*)d.shape_nodes, (size_t)r.num_shape_nodes)) return rc;
  std::vector<int> order, slots;
  make_levels(scene_nodes.data(), d.num_scene_nodes, u.scene_levels, order);
  prep_quad_slots(scene_nodes.data(), d.num_scene_nodes, slots);
  u.scene_quads = (long long)slots.size() / 4;
  if (u.scene_quads != (d.shape_wnodes - d.scene_wnodes) / 8) return vpt_set_error(VPT_ERR_HIP, "scene update: the scene's quad nodes do not match its binary nodes");
  u.shape_levels.assign((size_t)d.num_shapes, {}), u.shape_quads.assign((size_t)d.num_shapes, 0);
  for (int i = 0; i < d.num_shapes; i++) {
    const DShape& sh = r.m.shapes[(size_t)i];
    if ((long long)slots.size() / 4 != u.scene_quads + sh.wnode_offset) return vpt_set_error(VPT_ERR_HIP, "scene update: shape %d: quad nodes do not match its binary nodes", i);
    make_levels(shape_nodes.data() + sh.node_offset, sh.num_nodes, u.shape_levels[(size_t)i], order);
    prep_quad_slots(shape_nodes.data() + sh.node_offset, sh.num_nodes, slots);
    u.shape_quads[(size_t)i] = (long long)slots.size() / 4 - (u.scene_quads + sh.wnode_offset);
  }
  if (int rc = u.d_order.allocate(order.size() * sizeof(int))) return rc;
  if (int rc = u.d_quad_slots.allocate(slots.size() * sizeof(int))) return rc;
  if (int rc = u.d_inst_box.allocate((size_t)d.num_instances * 2 * sizeof(float4))) return rc;
  if (!order.empty()) HIP_TRY(hipMemcpy(u.d_order.get(), order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice));
  if (!slots.empty()) HIP_TRY(hipMemcpy(u.d_quad_slots.get(), slots.data(), slots.size() * sizeof(int), hipMemcpyHostToDevice));
  u.ready = true;
  return VPT_OK;
}

int validate_edit(const resident& r, const vpt_scene_edit& e, bool lights, const staged_vertices* on_device) {
  const DScene&       d = r.d;
  const host_mirrors& h = r.h;
  const edit_mirrors& u = r.m;
  if (int rc = check_ids("camera", e.num_cameras, e.camera_ids, e.cameras, d.num_cameras)) return rc;
  if (int rc = check_ids("instance", e.num_instances, e.instance_ids, e.instance_frames, d.num_instances)) return rc;
  if (int rc = check_ids("environment", e.num_environments, e.environment_ids, e.environment_frames, d.num_environments)) return rc;
  if (int rc = check_ids("material", e.num_materials, e.material_ids, e.materials, d.num_materials)) return rc;
  if (int rc = check_ids("shape", e.num_shapes, e.shape_ids, on_device ? (const void*)e.shape_ids : (const void*)e.shape_positions, d.num_shapes)) return rc;
  for (int i = 0; i < e.num_cameras; i++) {
    const vpt_camera& c = e.cameras[i];
    REQUIRE(finite_all(c.frame.x, 12) && finite_all(&c.lens, 5), "edit: camera entry %d: a value is not finite", i);
  }
  for (int i = 0; i < e.num_instances; i++) REQUIRE(finite_all(e.instance_frames[i].x, 12), "edit: instance entry %d: a frame value is not finite", i);
  for (int i = 0; i < e.num_environments; i++) REQUIRE(finite_all(e.environment_frames[i].x, 12), "edit: environment entry %d: a frame value is not finite", i);
  for (int i = 0; i < e.num_materials; i++) {
    const vpt_material& m = e.materials[i];
    const int id = e.material_ids[i];
    REQUIRE(finite_all(m.emission, 3) && finite_all(m.color, 3) && finite_all(&m.roughness, 3) && finite_all(m.scattering, 3) && finite_all(&m.scanisotropy, 3),
        "edit: material entry %d: a value is not finite", i);
    if (int rc = prep_check_material(m, id, d.num_textures, u.textured[(size_t)id] != 0)) return rc;
    if (!lights && emissive(m) != emissive(u.materials[(size_t)id]))
      return vpt_set_error(VPT_ERR_UNSUPPORTED, "edit: material entry %d: emission of material %d changes between zero and non-zero (the light list is fixed at creation)", i, id);
  }
  for (int i = 0; i < e.num_shapes; i++) {
    const int id = e.shape_ids[i];
    const size_t n = 3 * (size_t)h.shape_vertices[(size_t)id];
    if (on_device) {   // made on the device from input its maker has checked; the pools are the maker's to match
      REQUIRE(on_device->positions[(size_t)i] && (on_device->normals[(size_t)i] == nullptr) == (u.shapes[(size_t)id].normal_offset < 0),
          "edit: shape entry %d: staged vertices do not match the pools of shape %d", i, id);
    } else {
      REQUIRE(e.shape_positions[i], "edit: shape entry %d: null positions", i);
      REQUIRE(finite_all(e.shape_positions[i], n), "edit: shape entry %d: a position is not finite", i);
    }
    const float* nrm = !on_device && e.shape_normals ? e.shape_normals[i] : nullptr;
    if (nrm) {
      REQUIRE(u.shapes[(size_t)id].normal_offset >= 0, "edit: shape entry %d: shape %d has no normals", i, id);
      REQUIRE(finite_all(nrm, n), "edit: shape entry %d: a normal is not finite", i);
    }
    if (!lights && u.shape_lit[(size_t)id])
      return vpt_set_error(VPT_ERR_UNSUPPORTED, "edit: shape entry %d: shape %d belongs to a light's instance (its element cdf is made from the areas)", i, id);
  }
  return VPT_OK;
}

// The edit's bulk payload (moved vertices, instance frames) in its one block to the staging buffer the handle keeps: read by the
// scatter kernels that follow on stream 0 - no synchronisation in between.
int stage(resident& u, const staged_block& p) {
  if (p.host.size() > u.stage_bytes) {
    u.stage_bytes = 0;
    if (int rc = u.d_stage.allocate(p.host.size())) return rc;   // the call began with the device idle: nothing reads the buffer that goes
    u.stage_bytes = p.host.size();
  }
  if (!p.host.empty()) HIP_TRY(hipMemcpy(u.d_stage.get(), p.host.data(), p.host.size(), hipMemcpyHostToDevice));
  u.last_bytes += (long long)p.host.size();
  return VPT_OK;
}

// internal nodes of one BVH, deepest level first: a launch per level down to the narrow top, which one workgroup finishes
int refit_internal_levels(resident& u, float4* nodes, long long base, const bvh_levels& lv) {
  if (lv.first.empty()) return VPT_OK;
  const int  levels = (int)lv.first.size() - 1;
  const int* order  = u.refit.d_order.get<int>() + lv.offset;
  int top = 0;   // levels [0, top) are narrow: one launch
  const bool fuse = !getenv("VPT_UPDATE_NO_FUSE");   // A/B switch of the tests and measurements, read per call: a launch per level throughout - same bits
  while (fuse && top < levels && top < UPD_TOP_LEVELS && lv.first[(size_t)top + 1] - lv.first[(size_t)top] <= UPD_TOP_WIDTH) top++;
  for (int l = levels - 1; l >= top; l--) {
    const int count = lv.first[(size_t)l + 1] - lv.first[(size_t)l];
    LAUNCH(u, upd_refit_level_kernel, count, nodes, base, order + lv.first[(size_t)l], count);
  }
  if (top > 0) {
    top_levels t = {};
    for (int l = 0; l <= top; l++) t.first[l] = lv.first[(size_t)l];
    hipLaunchKernelGGL(upd_refit_top_kernel, dim3(1), dim3(UPD_TOP_WIDTH), 0, 0, nodes, base, order, t, top);
    LAUNCHED(u);
  }
  return VPT_OK;
}

}  // namespace

// the pieces a rebuild shares with the refit (vpt_scene_update.h), on the tables the caller names
int upd_element_boxes(resident& r, const DShape& sh, float* boxes, int* old_slot) {
  LAUNCH(r, upd_element_boxes_kernel, sh.num_elems, r.d.leaf_prims, (long long)sh.leaf_offset, sh.num_elems, boxes, old_slot);
  return VPT_OK;
}
int upd_shape_roots(resident& r, DShape* shapes, const float4* shape_nodes, int num_shapes) {
  if (num_shapes < 0) num_shapes = r.d.num_shapes;
  LAUNCH(r, upd_shape_roots_kernel, num_shapes, shapes, num_shapes, shape_nodes);
  return VPT_OK;
}
int upd_instance_boxes(resident& r, const DInstance* instances, int num_instances, const DShape* shapes, float4* inst_box) {
  LAUNCH(r, upd_instance_boxes_kernel, num_instances, instances, num_instances, shapes, inst_box);
  return VPT_OK;
}
int upd_enter_records(resident& r, float4* enter, int slots, const DInstance* instances, const DShape* shapes) {
  LAUNCH(r, upd_enter_records_kernel, slots, enter, slots, instances, shapes);
  return VPT_OK;
}
int upd_light_records(resident& r, const DShape* shapes) {
  LAUNCH(r, upd_light_records_kernel, r.d.num_lights, mut(r.d.light_rec), r.d.lights, r.d.num_lights, r.d.instances, shapes);
  return VPT_OK;
}

int scene_update_apply(resident& r, const vpt_scene_edit& e, edit_outcome& out, bool lights, const staged_vertices* on_device) {
  if (int rc = validate_edit(r, e, lights, on_device)) return rc;   // every refusal happens here: nothing has been written
  out.changed = true;   // (an edit without entries too: it starts the counters again)
  const bool refit = e.num_instances > 0 || e.num_shapes > 0;
  if (refit && !r.refit.ready)
    if (int rc = refit_tables_init(r, r.refit)) return rc;
  if (!on_device)
    if (int rc = begin_update(r)) return rc;
  DScene&             d = r.d;
  const host_mirrors& h = r.h;
  edit_mirrors&       m = r.m;

  // cameras, materials, environments: the payload itself (and the host-made inverse frame) into the tables
  for (int i = 0; i < e.num_cameras; i++)
    if (int rc = send(r, d.cameras + e.camera_ids[i], &e.cameras[i], 1)) return rc;
  for (int i = 0; i < e.num_materials; i++) {
    if (int rc = send(r, d.materials + e.material_ids[i], &e.materials[i], 1)) return rc;
    m.materials[(size_t)e.material_ids[i]] = e.materials[i];
  }
  if (e.num_materials > 0) r.varying_media = prep_media_vary(m.materials.data(), d.num_materials, m.inst_material.data(), m.inst_flags.data(), d.num_instances);
  for (int i = 0; i < e.num_environments; i++) {
    const int id = e.environment_ids[i];
    float4 inv[3], fwd[3];
    prep_environment_frames(e.environment_frames[i], inv, fwd);
    if (int rc = send(r, &d.environments[id].frame, &e.environment_frames[i], 1)) return rc;
    if (int rc = send(r, d.env_inv + 3 * (size_t)id, inv, 3)) return rc;
    m.environments[(size_t)id].frame = e.environment_frames[i];
    for (int l = 0; l < d.num_lights; l++) {   // light records of a textured environment hold both frames (build_lights); a constant one's stay zero
      const vpt_light& lt = m.lights[(size_t)l];
      if (lt.instance >= 0 || lt.sdf >= 0 || lt.environment != id) continue;
      if (m.light_kind[(size_t)l] != VPT_LIGHT_ENV_TEX) continue;
      const float4 both[6] = {inv[0], inv[1], inv[2], fwd[0], fwd[1], fwd[2]};
      if (int rc = send(r, d.light_rec + 8 * (size_t)l, both, 6)) return rc;
    }
  }
  if (!refit) return VPT_OK;

  // the bulk payload in one copy: positions / normals of the edited shapes, frames of the edited instances
  staged_block pay;
  std::vector<size_t> at_pos((size_t)e.num_shapes, 0), at_nrm((size_t)e.num_shapes, 0);
  for (int i = 0; i < e.num_shapes; i++) {
    if (on_device) break;   // the second source: the vertices are on the device already
    const size_t bytes = (size_t)h.shape_vertices[(size_t)e.shape_ids[i]] * 12;
    at_pos[(size_t)i] = pay.add(e.shape_positions[i], bytes);
    if (e.shape_normals && e.shape_normals[i]) at_nrm[(size_t)i] = pay.add(e.shape_normals[i], bytes);
  }
  std::vector<inst_payload> frames((size_t)e.num_instances);
  for (int i = 0; i < e.num_instances; i++) {
    frames[(size_t)i] = {};
    frames[(size_t)i].id = e.instance_ids[i];
    prep_instance_frames(e.instance_frames[i], frames[(size_t)i].inv, frames[(size_t)i].fwd, &frames[(size_t)i].translation_only);
  }
  const size_t at_frames = pay.add(frames.data(), frames.size() * sizeof(inst_payload));
  if (int rc = stage(r, pay)) return rc;
  const char*         staged = r.d_stage.get<char>();
  const refit_tables& u      = r.refit;
  if (!on_device) HIP_TRY(hipEventRecord(r.upd_ev0, 0));

  // 1. edited shapes: vertices, leaf records, shape BVH, its quad nodes
  float4* shape_nodes = mut(d.shape_nodes);
  for (int i = 0; i < e.num_shapes; i++) {
    const int     id = e.shape_ids[i];
    const DShape& sh = m.shapes[(size_t)id];
    const int     nv = h.shape_vertices[(size_t)id];
    const float* src_pos = on_device ? on_device->positions[(size_t)i] : (const float*)(staged + at_pos[(size_t)i]);
    const float* src_nrm = on_device ? on_device->normals[(size_t)i] : e.shape_normals && e.shape_normals[i] ? (const float*)(staged + at_nrm[(size_t)i]) : nullptr;
    LAUNCH(r, upd_scatter_vertices_kernel, nv, mut(d.positions) + sh.vertex_offset, src_pos, nv);
    if (src_nrm) LAUNCH(r, upd_scatter_vertices_kernel, nv, mut(d.normals) + sh.normal_offset, src_nrm, nv);
    LAUNCH(r, upd_leaf_records_kernel, sh.num_elems, sh, d.elems, d.positions, d.normals, mut(d.leaf_prims), mut(d.leaf_attrs), mut(d.tri_prims), mut(d.tri_attrs));
    LAUNCH(r, upd_refit_shape_leaves_kernel, sh.num_nodes, shape_nodes, (long long)sh.node_offset, sh.num_nodes, d.leaf_prims, (long long)sh.leaf_offset);
    if (int rc = refit_internal_levels(r, shape_nodes, sh.node_offset, u.shape_levels[(size_t)id])) return rc;
    const long long q0 = u.scene_quads + sh.wnode_offset, quads = u.shape_quads[(size_t)id];
    LAUNCH(r, upd_quad_gather_kernel, quads, mut(d.scene_wnodes) + 8 * q0, u.d_quad_slots.get<int4>() + q0, (int)quads, d.shape_nodes, (long long)sh.node_offset);
  }
  if (e.num_shapes > 0) LAUNCH(r, upd_shape_roots_kernel, d.num_shapes, mut(d.shapes), d.num_shapes, d.shape_nodes);

  // 2. edited instances: frames
  LAUNCH(r, upd_scatter_instances_kernel, e.num_instances, mut(d.instances), (const inst_payload*)(staged + at_frames), e.num_instances);

  // 3. the scene BVH from ALL instances, what hangs on frames and root boxes, the scene's quad nodes
  float4* scene_nodes = mut(d.scene_nodes);
  LAUNCH(r, upd_instance_boxes_kernel, d.num_instances, d.instances, d.num_instances, d.shapes, u.d_inst_box.get<float4>());
  LAUNCH(r, upd_enter_records_kernel, d.num_scene_prims, mut(d.scene_enter), d.num_scene_prims, d.instances, d.shapes);
  LAUNCH(r, upd_light_records_kernel, d.num_lights, mut(d.light_rec), d.lights, d.num_lights, d.instances, d.shapes);
  LAUNCH(r, upd_refit_scene_leaves_kernel, d.num_scene_nodes, scene_nodes, d.num_scene_nodes, d.scene_prims, u.d_inst_box.get<float4>());
  if (int rc = refit_internal_levels(r, scene_nodes, 0, u.scene_levels)) return rc;
  LAUNCH(r, upd_quad_gather_kernel, u.scene_quads, mut(d.scene_wnodes), u.d_quad_slots.get<int4>(), (int)u.scene_quads, d.scene_nodes, 0LL);
  if (int rc = mark_end(r)) return rc;
  if (d.num_scene_nodes > 0) {   // the six scene_root_* floats the kernels receive by value
    vpt_bvh_node root;
    HIP_TRY(hipMemcpy(&root, d.scene_nodes, sizeof(root), hipMemcpyDeviceToHost));
    d.scene_root_lo_x = root.bbox_min[0], d.scene_root_lo_y = root.bbox_min[1], d.scene_root_lo_z = root.bbox_min[2];
    d.scene_root_hi_x = root.bbox_max[0], d.scene_root_hi_y = root.bbox_max[1], d.scene_root_hi_z = root.bbox_max[2];
  }
  return finish_update(r);
}
