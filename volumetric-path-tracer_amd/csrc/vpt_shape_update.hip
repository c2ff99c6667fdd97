// vpt_shape_update.hip — the shapes of a resident scene added, removed and replaced on the device (include/vpt.h:
// vpt_scene_update_shapes).  The shape list changes length and numbering, and so does every pool that is laid out in
// shape order: vertices, elements, leaf records, nodes, quad nodes.  The new layout is integer work on the host (vpt_shape_layout.h);
// an untouched shape's part of every pool moves device to device, one copy per pool and run of adjacent survivors, and since every
// offset inside a shape is local to it nothing in it is rewritten.  A `set` or added shape comes down as the caller's arrays in ONE
// copy and becomes pool entries here: float3 to float4, indices to int4 with build_geometry's repeat rule, element boxes through the
// refit's record_bounds, the tree by K6's core (vpt_bvh_build.h), the leaf records in the tree's primitive order by
// su_leaf_records_kernel.  What depends on topology alone - quad nodes, root references, stack needs, the traversal limits - is made
// on the host by creation's own function from the read-back of the new shapes' nodes; the scene level is vpt_bvh_rebuild.h's.
// Everything is built into buffers of the call; tables, counts and mirrors are swapped after the last check.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "vpt_bvh_build.h"
#include "vpt_error.h"
#include "vpt_light_update.h"
#include "vpt_record_bounds.hip.h"
#include "vpt_scene_update.h"
#include "vpt_shape_layout.h"
#include "vpt_shape_update.h"
#include "vpt_subdiv_update.h"
#include "vpt_update_helpers.h"

namespace {

enum { SU_QUADS = 0, SU_TRIANGLES = 1, SU_POINTS = 2, SU_LINES = 3 };   // the form of a shape's index list

// ---- kernels --------------------------------------------------------------------------------------------------------------
// float3 in, the pools' float4 out (w = 0, as build_geometry leaves it)
__global__ void su_float3_kernel(float4* __restrict__ pool, const float* __restrict__ src, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) pool[i] = make_float4(src[3 * i], src[3 * i + 1], src[3 * i + 2], 0);
}
// the caller's index list to the int4 of the element pool: elements repeat their last vertex (build_geometry)
__global__ void su_elems_kernel(int4* __restrict__ elems, const int* __restrict__ src, int n, int form) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  int4 q;
  if (form == SU_POINTS) q.x = q.y = q.z = q.w = src[e];
  else if (form == SU_LINES) q.x = src[2 * e], q.y = q.z = q.w = src[2 * e + 1];
  else if (form == SU_TRIANGLES) q.x = src[3 * e], q.y = src[3 * e + 1], q.z = q.w = src[3 * e + 2];
  else q = make_int4(src[4 * e], src[4 * e + 1], src[4 * e + 2], src[4 * e + 3]);
  elems[e] = q;
}

// float4 `c` of the leaf record build_geometry makes of element e (vpt_device.h): a face's corner c with the element id in p0.w and
// the kind, 0, in p3.w; {p, e} {r, 0, 0, 0} {0} {0, 0, 0, kind} of a point; {p0, e} {p1, 0} {r0, r1, 0, 0} {0, 0, 0, kind} of a line
__device__ inline float4 record_part(int c, int e, int4 q, int kind, const float4* __restrict__ P, const float* __restrict__ rad) {
  float4 p = make_float4(0, 0, 0, 0);
  if (kind == 0) {
    p = P[c == 0 ? q.x : c == 1 ? q.y : c == 2 ? q.z : q.w];
    p.w = 0;
  } else if (c == 0) p = P[q.x];
  else if (c == 1) p = kind == VPT_LEAF_LINE ? P[q.y] : make_float4(rad[q.x], 0, 0, 0);
  else if (c == 2 && kind == VPT_LEAF_LINE) p = make_float4(rad[q.x], rad[q.y], 0, 0);
  if (kind != 0 && c == 1) p.w = 0;
  if (c == 0) p.w = __int_as_float(e);
  if (c == 3) p.w = __int_as_float(kind);
  return p;
}
// the bounds of every element in ELEMENT order, the input of the build: the record the element will have, through the refit's own
// record_bounds (point_bounds, line_bounds, triangle_bounds, quad_bounds in select form)
__global__ void su_element_boxes_kernel(int n, const int4* __restrict__ elems, const float4* __restrict__ P, const float* __restrict__ rad, int kind, float* __restrict__ boxes) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int4 q = elems[e];
  float4 r[4];
  for (int c = 0; c < 4; c++) r[c] = record_part(c, e, q, kind, P, rad);
  const box3 b = record_bounds(r);
  for (int c = 0; c < 3; c++) boxes[6 * (long long)e + c] = b.lo[c], boxes[6 * (long long)e + 3 + c] = b.hi[c];
}

__device__ inline float2 tex_at(const float2* __restrict__ T, int v) { return T ? T[v] : make_float2(0, 0); }   // zeros where the shape has no texcoords

struct su_shape {   // one `set` or added shape in the new pools
  int num_elems, kind;
  long long elem_offset, leaf_offset, vertex_offset, normal_offset, texcoord_offset;   // -1: the shape has no normals / texcoords
};
// Every form the scene keeps of the leaf records of one shape, from scratch: slot k holds element e = prims[k].  Four adjacent lanes
// make one slot, lane c its corner c: one float4 of leaf_prims each, so a wave writes sixteen whole 64-byte records contiguously; of
// leaf_attrs lane c writes corner c's normal and lanes 0 and 1 the two float4 of texcoords (zeros where the shape has none); of the
// compact forms (a scene of triangles, else null) lanes 0..2 write the corners and {normal, texcoord word}, lane 3 the last float4 of
// tri_attrs.  160 B a slot, 272 with the compact forms; plain stores, no hand-off between lanes.
__global__ void su_leaf_records_kernel(su_shape sh, const int* __restrict__ prims, const int4* __restrict__ elems, const float4* __restrict__ positions,
    const float4* __restrict__ normals, const float2* __restrict__ texcoords, const float* __restrict__ rad, float4* __restrict__ leaf_prims,
    float4* __restrict__ leaf_attrs, float4* __restrict__ tri_prims, float4* __restrict__ tri_attrs) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long k = t >> 2;
  const int       c = (int)(t & 3);
  if (k >= sh.num_elems) return;
  const int e = prims[k];
  if (e < 0 || e >= sh.num_elems) return;   // (the host checks the order it reads back: never taken)
  const int4      q = elems[sh.elem_offset + e];
  const long long slot = sh.leaf_offset + k;
  const float4    part = record_part(c, e, q, sh.kind, positions + sh.vertex_offset, rad);
  leaf_prims[4 * slot + c] = part;
  // (selects throughout: a corner array indexed by the lane's c would live in scratch)
  const int    vc  = c == 0 ? q.x : c == 1 ? q.y : c == 2 ? q.z : q.w;
  const float4 nrm = sh.normal_offset >= 0 ? normals[sh.normal_offset + vc] : make_float4(0, 0, 0, 0);
  leaf_attrs[6 * slot + c] = nrm;
  const float2* T = sh.texcoord_offset >= 0 ? texcoords + sh.texcoord_offset : nullptr;
  if (c < 2) {   // the texcoords of corners 0, 1 (lane 0) and 2, 3 (lane 1)
    const float2 a = tex_at(T, c == 0 ? q.x : q.z), b = tex_at(T, c == 0 ? q.y : q.w);
    leaf_attrs[6 * slot + 4 + c] = make_float4(a.x, a.y, b.x, b.y);
  }
  if (!tri_prims) return;
  // tri_attrs: {n0, t0.x} {n1, t0.y} {n2, t1.x} {t1.y, t2.x, t2.y, 0} (build_geometry)
  if (c < 3) {
    tri_prims[3 * slot + c] = part;
    const float2 t = tex_at(T, c == 2 ? q.y : q.x);
    tri_attrs[4 * slot + c] = make_float4(nrm.x, nrm.y, nrm.z, c == 1 ? t.y : t.x);
  } else {
    const float2 t1 = tex_at(T, q.y), t2 = tex_at(T, q.z);
    tri_attrs[4 * slot + 3] = make_float4(t1.y, t2.x, t2.y, 0);
  }
}
// The compact forms of slots [first, first + count) from the general records (build_geometry's last loop): a scene that was not one
// of triangles becomes one, so the survivors' compact records are made here and not uploaded.  Four lanes a slot, as above.
__global__ void su_compact_kernel(long long first, long long count, const float4* __restrict__ leaf_prims, const float4* __restrict__ leaf_attrs,
    float4* __restrict__ tri_prims, float4* __restrict__ tri_attrs) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int       c = (int)(t & 3);
  if ((t >> 2) >= count) return;
  const long long slot = first + (t >> 2);
  const float4    t01 = leaf_attrs[6 * slot + 4];
  if (c < 3) {
    tri_prims[3 * slot + c] = leaf_prims[4 * slot + c];
    const float4 n = leaf_attrs[6 * slot + c];
    tri_attrs[4 * slot + c] = make_float4(n.x, n.y, n.z, c == 0 ? t01.x : c == 1 ? t01.y : t01.z);
  } else {
    const float4 t23 = leaf_attrs[6 * slot + 5];
    tri_attrs[4 * slot + 3] = make_float4(t01.w, t23.x, t23.y, 0);
  }
}
// DInstance::shape and shape_flags through the map old shape id -> {new id, flags of the shape that has it now}
__global__ void su_instance_shapes_kernel(DInstance* __restrict__ instances, int n, const int2* __restrict__ map, int num_old_shapes) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = instances[i].shape;
  if (s < 0 || s >= num_old_shapes) return;   // (never taken: creation and every edit checked it)
  const int2 m = map[s];
  instances[i].shape = m.x, instances[i].shape_flags = m.y;
}

// ---- host -----------------------------------------------------------------------------------------------------------------
struct mesh {   // one `set` or added shape: what the edit says of it, and where its arrays sit in the staged block
  const vpt_shape_data* s = nullptr;
  int    kind = 0, form = SU_QUADS, num_elems = 0, flags = 0;
  size_t at_pos = 0, at_nrm = 0, at_tc = 0, at_col = 0, at_rad = 0, at_idx = 0;
  // its tree, on the device until the pools are laid out, and the read-back
  int                       count = 0;
  device_buffer             nodes;
  std::vector<vpt_bvh_node> h_nodes;
  std::vector<int>          prims;
};


// validate()'s rules for one shape of the edit
int check_mesh(const vpt_shape_data& s, const char* list, int i, mesh& m) {
  REQUIRE(s.num_vertices >= 0 && s.num_triangles >= 0 && s.num_quads >= 0 && s.num_points >= 0 && s.num_lines >= 0, "edit: %s entry %d: a negative count", list, i);
  REQUIRE(s.num_vertices == 0 || s.positions, "edit: %s entry %d: null positions", list, i);
  REQUIRE((s.num_triangles == 0 || s.triangles) && (s.num_quads == 0 || s.quads) && (s.num_points == 0 || s.points) && (s.num_lines == 0 || s.lines),
      "edit: %s entry %d: a null element list with a non-zero count", list, i);
  if (int rc = prep_check_shape_elements(i, s.num_vertices, s.triangles, s.num_triangles, s.quads, s.num_quads, s.points, s.num_points, s.lines, s.num_lines)) return rc;
  const bool curves = s.num_points || s.num_lines;
  REQUIRE(!curves || s.radius || s.num_vertices == 0, "edit: %s entry %d: a shape of points or lines needs one radius per vertex", list, i);
  const size_t nv = (size_t)s.num_vertices;
  REQUIRE(finite_all(s.positions, 3 * nv) && (!s.normals || finite_all(s.normals, 3 * nv)) && (!s.texcoords || finite_all(s.texcoords, 2 * nv)) &&
              (!s.colors || finite_all(s.colors, 4 * nv)) && (!curves || finite_all(s.radius, nv)),
      "edit: %s entry %d: a value is not finite", list, i);
  m.s = &s;
  m.kind = s.num_points ? VPT_LEAF_POINT : s.num_lines ? VPT_LEAF_LINE : 0;
  m.form = s.num_points ? SU_POINTS : s.num_lines ? SU_LINES : s.num_triangles ? SU_TRIANGLES : SU_QUADS;
  m.num_elems = s.num_points ? s.num_points : s.num_lines ? s.num_lines : s.num_triangles ? s.num_triangles : s.num_quads;
  const bool some = s.num_vertices > 0;   // an attribute of no vertices is an absent one, as an empty vector is to the host flattening
  m.flags = (s.num_triangles ? VPT_SHP_TRIANGLES : 0) | (s.normals && some ? VPT_SHP_NORMALS : 0) | (s.texcoords && some ? VPT_SHP_TEXCOORDS : 0) | (s.colors && some ? VPT_SHP_COLORS : 0) |
            (s.num_points ? VPT_SHP_POINTS : 0) | (s.num_lines ? VPT_SHP_LINES : 0);
  return VPT_OK;
}

// the pools that are laid out in shape order, and what a shape takes of each
enum { P_POSITIONS, P_NORMALS, P_TEXCOORDS, P_COLORS, P_ELEMS, P_NODES, P_QUADS, P_COUNT };
struct shape_sizes { long long len[P_COUNT]; };

int validate_edit(const resident& r, const vpt_shape_edit& e, std::vector<mesh>& meshes) {
  const DScene&       d = r.d;
  const host_mirrors& h = r.h;
  if (int rc = check_ids("remove", e.num_remove, e.remove_ids, d.num_shapes)) return rc;
  if (int rc = check_ids("set", e.num_set, e.set_ids, e.set, d.num_shapes)) return rc;
  REQUIRE(e.num_add >= 0 && (e.num_add == 0 || e.add), "edit: add list is null or has a negative count");
  REQUIRE((long long)d.num_shapes - e.num_remove + e.num_add <= 0x7fffffffLL, "edit: more than 2^31 shapes");
  std::vector<char> removed((size_t)d.num_shapes, 0);
  for (int i = 0; i < e.num_remove; i++) removed[(size_t)e.remove_ids[i]] = 1;
  for (int i = 0; i < e.num_set; i++) REQUIRE(!removed[(size_t)e.set_ids[i]], "edit: set entry %d: shape %d is also removed", i, e.set_ids[i]);
  for (int i = 0; i < d.num_instances; i++)
    REQUIRE(!removed[(size_t)h.inst_shape[(size_t)i]], "edit: shape %d is removed but instance %d names it (remove or re-point its instances first)", h.inst_shape[(size_t)i], i);
  meshes.resize((size_t)e.num_set + (size_t)e.num_add);
  for (int i = 0; i < e.num_set; i++)
    if (int rc = check_mesh(e.set[i], "set", i, meshes[(size_t)i])) return rc;
  for (int i = 0; i < e.num_add; i++)
    if (int rc = check_mesh(e.add[i], "add", i, meshes[(size_t)e.num_set + (size_t)i])) return rc;
  return VPT_OK;
}

}  // namespace

int shape_update_apply(resident& r, const vpt_shape_edit& e, edit_outcome& out) {
  DScene&       d = r.d;
  host_mirrors& h = r.h;
  edit_mirrors& m = r.m;
  std::vector<mesh> meshes;
  if (int rc = validate_edit(r, e, meshes)) return rc;   // every refusal about the request happens here: nothing has been written
  if (e.num_remove == 0 && e.num_set == 0 && e.num_add == 0) return VPT_OK;
  const int n_old = d.num_shapes, ninst = d.num_instances;

  // ---- the layout: the new list, and per pool the offset of every shape in the old pools and in the new ones ---------------------
  std::vector<shape_slot> list;
  std::vector<int>        new_of_old;
  shape_list_of_edit(n_old, e.remove_ids, e.num_remove, e.set_ids, e.num_set, e.num_add, list, new_of_old);
  const int n_new = (int)list.size();
  std::vector<shape_sizes> was((size_t)n_old), now((size_t)n_new);
  for (int i = 0; i < n_old; i++) {
    const DShape&   sh = m.shapes[(size_t)i];
    const long long nv = h.shape_vertices[(size_t)i];
    was[(size_t)i] = {{nv, sh.normal_offset >= 0 ? nv : 0, sh.texcoord_offset >= 0 ? nv : 0, sh.color_offset >= 0 ? nv : 0, sh.num_elems, sh.num_nodes, r.shape_quads[(size_t)i]}};
  }
  auto offsets_of = [](const std::vector<shape_sizes>& sizes, int pool) {
    std::vector<long long> len(sizes.size());
    for (size_t i = 0; i < sizes.size(); i++) len[i] = sizes[i].len[pool];
    return pool_offsets(len);
  };
  std::vector<long long> old_at[P_COUNT], new_at[P_COUNT];
  for (int p = 0; p < P_COUNT; p++) old_at[p] = offsets_of(was, p);
  // the resident pools must be the ones this layout describes: contiguous in shape order (a descriptor made by other means may not be)
  bool contiguous = old_at[P_POSITIONS][(size_t)n_old] == r.num_positions && old_at[P_NORMALS][(size_t)n_old] == r.num_normals &&
                    old_at[P_TEXCOORDS][(size_t)n_old] == r.num_texcoords && old_at[P_COLORS][(size_t)n_old] == r.num_colors &&
                    old_at[P_NODES][(size_t)n_old] == r.num_shape_nodes && 8 * old_at[P_QUADS][(size_t)n_old] == r.num_shape_wnodes;
  for (int i = 0; i < n_old && contiguous; i++) {
    const DShape& sh = m.shapes[(size_t)i];
    contiguous = sh.vertex_offset == old_at[P_POSITIONS][(size_t)i] && (sh.normal_offset < 0 || sh.normal_offset == old_at[P_NORMALS][(size_t)i]) &&
                 (sh.texcoord_offset < 0 || sh.texcoord_offset == old_at[P_TEXCOORDS][(size_t)i]) && (sh.color_offset < 0 || sh.color_offset == old_at[P_COLORS][(size_t)i]) &&
                 sh.elem_offset == old_at[P_ELEMS][(size_t)i] && sh.leaf_offset == old_at[P_ELEMS][(size_t)i] && sh.node_offset == old_at[P_NODES][(size_t)i] &&
                 sh.wnode_offset == old_at[P_QUADS][(size_t)i];
  }
  if (!contiguous) return vpt_set_error(VPT_ERR_UNSUPPORTED, "edit: the scene's pools are not contiguous in shape order (the layout of the host flattening)");
  std::vector<int> flags((size_t)n_new);
  for (int j = 0; j < n_new; j++) {
    const shape_slot& sl = list[(size_t)j];
    if (sl.payload < 0) {
      now[(size_t)j] = was[(size_t)sl.old_id], flags[(size_t)j] = m.shape_flags[(size_t)sl.old_id];
      continue;
    }
    const mesh&     ms = meshes[(size_t)sl.payload];
    const long long nv = ms.s->num_vertices;
    now[(size_t)j] = {{nv, ms.flags & VPT_SHP_NORMALS ? nv : 0, ms.flags & VPT_SHP_TEXCOORDS ? nv : 0, ms.flags & VPT_SHP_COLORS ? nv : 0, ms.num_elems, 0, 0}};   // nodes and quad nodes: after the build
    flags[(size_t)j] = ms.flags;
  }
  for (int p = P_POSITIONS; p <= P_ELEMS; p++) {
    new_at[p] = offsets_of(now, p);
    REQUIRE(new_at[p][(size_t)n_new] <= 0x7fffffffLL, "edit: a pool of the new scene has more than 2^31 entries");
  }
  const std::vector<shape_run> runs = survivor_runs(list);
  const long long n_pos = new_at[P_POSITIONS][(size_t)n_new], n_nrm = new_at[P_NORMALS][(size_t)n_new], n_tc = new_at[P_TEXCOORDS][(size_t)n_new],
                  n_col = new_at[P_COLORS][(size_t)n_new], n_elem = new_at[P_ELEMS][(size_t)n_new];
  // the new shape records: counts and the offsets known so far; the mirrors of the new list
  std::vector<DShape> shapes((size_t)n_new);
  bool compact = n_new > 0 && !getenv("VPT_NO_COMPACT_TRIANGLES");   // build_geometry: every shape holds triangles
  for (int j = 0; j < n_new; j++) {
    DShape& o = shapes[(size_t)j];
    o = {};
    const shape_slot& sl = list[(size_t)j];
    if (sl.payload < 0) o = m.shapes[(size_t)sl.old_id];
    else o.is_triangles = meshes[(size_t)sl.payload].form == SU_TRIANGLES, o.num_elems = meshes[(size_t)sl.payload].num_elems;
    o.elem_offset = o.leaf_offset = (int)new_at[P_ELEMS][(size_t)j], o.vertex_offset = (int)new_at[P_POSITIONS][(size_t)j];
    o.normal_offset   = flags[(size_t)j] & VPT_SHP_NORMALS ? (int)new_at[P_NORMALS][(size_t)j] : -1;
    o.texcoord_offset = flags[(size_t)j] & VPT_SHP_TEXCOORDS ? (int)new_at[P_TEXCOORDS][(size_t)j] : -1;
    o.color_offset    = flags[(size_t)j] & VPT_SHP_COLORS ? (int)new_at[P_COLORS][(size_t)j] : -1;
    compact = compact && o.is_triangles && o.num_elems > 0;
  }

  // ---- the payload of the `set` and added shapes in one copy ------------------------------------------------------------------------
  staged_block pay;
  int   most_elems = 0;
  for (mesh& ms : meshes) {
    const vpt_shape_data& s  = *ms.s;
    const size_t          nv = (size_t)s.num_vertices;
    ms.at_pos = pay.add(s.positions, 12 * nv);
    if (ms.flags & VPT_SHP_NORMALS) ms.at_nrm = pay.add(s.normals, 12 * nv);
    if (ms.flags & VPT_SHP_TEXCOORDS) ms.at_tc = pay.add(s.texcoords, 8 * nv);
    if (ms.flags & VPT_SHP_COLORS) ms.at_col = pay.add(s.colors, 16 * nv);
    if (ms.kind) ms.at_rad = pay.add(s.radius, 4 * nv);
    const void*  idx   = ms.form == SU_POINTS ? s.points : ms.form == SU_LINES ? s.lines : ms.form == SU_TRIANGLES ? s.triangles : s.quads;
    const size_t width = ms.form == SU_POINTS ? 4 : ms.form == SU_LINES ? 8 : ms.form == SU_TRIANGLES ? 12 : 16;
    ms.at_idx  = pay.add(idx, width * (size_t)ms.num_elems);
    most_elems = std::max(most_elems, ms.num_elems);
  }
  if (int rc = begin_update(r)) return rc;
  device_buffer d_block, d_boxes, n_positions, n_normals, n_texcoords, n_colors, n_elems, n_leaf_prims, n_leaf_attrs, n_tri_prims, n_tri_attrs;
  if (int rc = send(r, d_block, pay.host)) return rc;
  if (int rc = d_boxes.allocate(6 * (size_t)most_elems * sizeof(float))) return rc;
  if (int rc = n_positions.allocate((size_t)n_pos * sizeof(float4))) return rc;
  if (int rc = n_normals.allocate((size_t)n_nrm * sizeof(float4))) return rc;
  if (int rc = n_texcoords.allocate((size_t)n_tc * sizeof(float2))) return rc;
  if (int rc = n_colors.allocate((size_t)n_col * sizeof(float4))) return rc;
  if (int rc = n_elems.allocate((size_t)n_elem * sizeof(int4))) return rc;
  if (int rc = n_leaf_prims.allocate((4 * (size_t)n_elem + 8) * sizeof(float4))) return rc;   // + 8: phase B fetches one record ahead (build_geometry)
  if (int rc = n_leaf_attrs.allocate(6 * (size_t)n_elem * sizeof(float4))) return rc;
  HIP_TRY(hipMemset(n_leaf_prims.get<float4>() + 4 * (size_t)n_elem, 0, 8 * sizeof(float4)));
  if (compact) {
    if (int rc = n_tri_prims.allocate((3 * (size_t)n_elem + 8) * sizeof(float4))) return rc;
    if (int rc = n_tri_attrs.allocate(4 * (size_t)n_elem * sizeof(float4))) return rc;
    HIP_TRY(hipMemset(n_tri_prims.get<float4>() + 3 * (size_t)n_elem, 0, 8 * sizeof(float4)));
  }
  bvh_build_scratch core;
  if (int rc = core.reserve(std::max(std::max(most_elems, e.num_set > 0 ? ninst : 0), 1))) return rc;
  HIP_TRY(hipEventRecord(r.upd_ev0, 0));

  // ---- 1. untouched shapes: their part of the vertex, element and leaf pools, one copy per pool and run of adjacent survivors ------
  const bool compact_kept = compact && d.tri_prims;   // the survivors' compact records exist: they move; else (3.) they are made
  for (const shape_run& run : runs) {
    auto part = [&](int pool, void* to, const void* from, size_t entry) {   // entries [first_old, first_old + count) of a pool to their new place
      const long long a = old_at[pool][(size_t)run.first_old], b = old_at[pool][(size_t)run.first_old + (size_t)run.count];
      return copy_on_device((char*)to + (size_t)new_at[pool][(size_t)run.first_new] * entry, (const char*)from + (size_t)a * entry, (size_t)(b - a) * entry);
    };
    if (int rc = part(P_POSITIONS, n_positions.get(), d.positions, sizeof(float4))) return rc;
    if (int rc = part(P_NORMALS, n_normals.get(), d.normals, sizeof(float4))) return rc;
    if (int rc = part(P_TEXCOORDS, n_texcoords.get(), d.texcoords, sizeof(float2))) return rc;
    if (int rc = part(P_COLORS, n_colors.get(), d.colors, sizeof(float4))) return rc;
    if (int rc = part(P_ELEMS, n_elems.get(), d.elems, sizeof(int4))) return rc;
    if (int rc = part(P_ELEMS, n_leaf_prims.get(), d.leaf_prims, 4 * sizeof(float4))) return rc;
    if (int rc = part(P_ELEMS, n_leaf_attrs.get(), d.leaf_attrs, 6 * sizeof(float4))) return rc;
    if (compact_kept) {
      if (int rc = part(P_ELEMS, n_tri_prims.get(), d.tri_prims, 3 * sizeof(float4))) return rc;
      if (int rc = part(P_ELEMS, n_tri_attrs.get(), d.tri_attrs, 4 * sizeof(float4))) return rc;
    }
  }

  // ---- 2. `set` and added shapes: pool entries, element boxes, the tree, the leaf records in its order; nodes and order read back ----
  const char* staged = d_block.get<char>();
  for (int j = 0; j < n_new; j++) {
    if (list[(size_t)j].payload < 0) continue;
    mesh&                 ms = meshes[(size_t)list[(size_t)j].payload];
    const vpt_shape_data& s  = *ms.s;
    const DShape&         o  = shapes[(size_t)j];
    const int             nv = s.num_vertices, n = ms.num_elems;
    LAUNCH(r, su_float3_kernel, nv, n_positions.get<float4>() + o.vertex_offset, (const float*)(staged + ms.at_pos), nv);
    if (ms.flags & VPT_SHP_NORMALS) LAUNCH(r, su_float3_kernel, nv, n_normals.get<float4>() + o.normal_offset, (const float*)(staged + ms.at_nrm), nv);
    if (ms.flags & VPT_SHP_TEXCOORDS)
      if (int rc = copy_on_device(n_texcoords.get<float2>() + o.texcoord_offset, staged + ms.at_tc, 8 * (size_t)nv)) return rc;
    if (ms.flags & VPT_SHP_COLORS)
      if (int rc = copy_on_device(n_colors.get<float4>() + o.color_offset, staged + ms.at_col, 16 * (size_t)nv)) return rc;
    const float* rad = ms.kind ? (const float*)(staged + ms.at_rad) : nullptr;
    LAUNCH(r, su_elems_kernel, n, n_elems.get<int4>() + o.elem_offset, (const int*)(staged + ms.at_idx), n, ms.form);
    LAUNCH(r, su_element_boxes_kernel, n, n, n_elems.get<int4>() + o.elem_offset, n_positions.get<float4>() + o.vertex_offset, rad, ms.kind, d_boxes.get<float>());
    if (int rc = bvh_build_core(core, d_boxes.get<float>(), 6, n, &ms.count, &r.last_launches)) return rc;
    if (int rc = ms.nodes.allocate((size_t)ms.count * sizeof(vpt_bvh_node))) return rc;
    if (int rc = copy_on_device(ms.nodes.get(), core.nodes(), (size_t)ms.count * sizeof(vpt_bvh_node))) return rc;
    const su_shape on_device = {n, ms.kind, o.elem_offset, o.leaf_offset, o.vertex_offset, o.normal_offset, o.texcoord_offset};
    LAUNCH(r, su_leaf_records_kernel, 4LL * n, on_device, core.primitives(), n_elems.get<int4>(), n_positions.get<float4>(), n_normals.get<float4>(),
        n_texcoords.get<float2>(), rad, n_leaf_prims.get<float4>(), n_leaf_attrs.get<float4>(), compact ? n_tri_prims.get<float4>() : nullptr,
        compact ? n_tri_attrs.get<float4>() : nullptr);
    if (int rc = fetch(r, ms.h_nodes, ms.nodes.get(), (size_t)ms.count)) return rc;
    if (int rc = fetch(r, ms.prims, core.primitives(), (size_t)n)) return rc;   // (after the launch above in stream order)
    std::vector<char> seen((size_t)n, 0);
    for (int k : ms.prims) {
      if (k < 0 || k >= n || seen[(size_t)k]) return vpt_set_error(VPT_ERR_HIP, "shape update: new shape %d: the primitive order is not a permutation", j);
      seen[(size_t)k] = 1;
    }
    now[(size_t)j].len[P_NODES] = ms.count;
  }
  // ---- 3. a scene that becomes one of triangles: the survivors' compact records from their general ones ----------------------------
  if (compact && !compact_kept)
    for (const shape_run& run : runs) {
      const long long first = new_at[P_ELEMS][(size_t)run.first_new], count = new_at[P_ELEMS][(size_t)run.first_new + (size_t)run.count] - first;
      LAUNCH(r, su_compact_kernel, 4 * count, first, count, n_leaf_prims.get<float4>(), n_leaf_attrs.get<float4>(), n_tri_prims.get<float4>(), n_tri_attrs.get<float4>());
    }

  // ---- 4. the node pool at its new size: new trees and, device to device, the untouched ones ---------------------------------------
  new_at[P_NODES] = offsets_of(now, P_NODES);
  const long long n_nodes = new_at[P_NODES][(size_t)n_new];
  if (n_nodes > 0x7fffffffLL) return vpt_set_error(VPT_ERR_UNSUPPORTED, "more than 2^31 shape bvh nodes");
  device_buffer n_shape_nodes, n_shapes;
  if (int rc = n_shape_nodes.allocate((size_t)n_nodes * sizeof(vpt_bvh_node))) return rc;
  for (const shape_run& run : runs) {
    const long long a = old_at[P_NODES][(size_t)run.first_old], b = old_at[P_NODES][(size_t)run.first_old + (size_t)run.count];
    if (int rc = copy_on_device(n_shape_nodes.get<vpt_bvh_node>() + new_at[P_NODES][(size_t)run.first_new], (const vpt_bvh_node*)d.shape_nodes + a, (size_t)(b - a) * sizeof(vpt_bvh_node))) return rc;
  }
  std::vector<vpt_bvh_node> made_nodes;   // of the new shapes alone, in shape order: what the quad nodes are made from
  std::vector<vpt_shape>    desc_shapes((size_t)n_new);
  std::vector<char>         made((size_t)n_new, 0);
  for (int j = 0; j < n_new; j++) {
    DShape& o = shapes[(size_t)j];
    o.node_offset = (int)new_at[P_NODES][(size_t)j], o.num_nodes = (int)now[(size_t)j].len[P_NODES];
    desc_shapes[(size_t)j] = {};
    if (list[(size_t)j].payload < 0) continue;
    const mesh& ms = meshes[(size_t)list[(size_t)j].payload];
    if (int rc = copy_on_device(n_shape_nodes.get<vpt_bvh_node>() + o.node_offset, ms.nodes.get(), (size_t)ms.count * sizeof(vpt_bvh_node))) return rc;
    made[(size_t)j] = 1;
    desc_shapes[(size_t)j].bvh_node_offset = (int)made_nodes.size(), desc_shapes[(size_t)j].num_bvh_nodes = ms.count;
    made_nodes.insert(made_nodes.end(), ms.h_nodes.begin(), ms.h_nodes.end());
  }

  // ---- 5. instances under the new numbering; the scene BVH when a shape was replaced; the traversal limits ------------------------
  std::vector<int>  inst_shape((size_t)ninst), inst_flags((size_t)ninst), light_old_of_new((size_t)ninst);
  std::vector<int2> shape_map((size_t)n_old);
  std::vector<char> is_set((size_t)n_old, 0);
  for (int i = 0; i < e.num_set; i++) is_set[(size_t)e.set_ids[i]] = 1;
  for (int i = 0; i < n_old; i++) shape_map[(size_t)i] = make_int2(new_of_old[(size_t)i], new_of_old[(size_t)i] >= 0 ? flags[(size_t)new_of_old[(size_t)i]] : 0);
  for (int i = 0; i < ninst; i++) {
    const int was_shape = h.inst_shape[(size_t)i];
    inst_shape[(size_t)i] = shape_map[(size_t)was_shape].x, inst_flags[(size_t)i] = shape_map[(size_t)was_shape].y;
    light_old_of_new[(size_t)i] = is_set[(size_t)was_shape] ? -1 : i;   // a replaced shape: its light's CDF is made anew
  }
  device_buffer n_instances, d_map;
  if (int rc = n_instances.allocate((size_t)ninst * sizeof(DInstance))) return rc;
  if (int rc = copy_on_device(n_instances.get(), d.instances, (size_t)ninst * sizeof(DInstance))) return rc;
  if (int rc = send(r, d_map, shape_map)) return rc;
  LAUNCH(r, su_instance_shapes_kernel, ninst, n_instances.get<DInstance>(), ninst, d_map.get<int2>(), n_old);

  const bool  scene_built = e.num_set > 0;
  scene_level lv;
  lv.num_instances = ninst;
  if (scene_built) {   // the shape records as far as they are known, their root boxes from the new pool: what the instance boxes are made from
    if (int rc = send(r, n_shapes, shapes)) return rc;
    if (int rc = upd_shape_roots(r, n_shapes.get<DShape>(), n_shape_nodes.get<float4>(), n_new)) return rc;
    if (int rc = scene_level_build(r, core, n_instances.get<DInstance>(), ninst, n_shapes.get<DShape>(), lv)) return rc;
  } else {   // the scene BVH stays: its primitive order from the slots the handle knows
    if (d.num_scene_prims != ninst) return vpt_set_error(VPT_ERR_UNSUPPORTED, "edit: the scene bvh does not hold every instance once");
    lv.h_prims.assign((size_t)d.num_scene_prims, -1);
    for (int i = 0; i < ninst; i++)
      if (h.slot_of[(size_t)i] >= 0) lv.h_prims[(size_t)h.slot_of[(size_t)i]] = i;
    for (int id : lv.h_prims)
      if (id < 0) return vpt_set_error(VPT_ERR_UNSUPPORTED, "edit: the scene bvh does not hold every instance once");
  }
  vpt_scene_desc desc = {};
  desc.num_shapes = n_new, desc.shapes = desc_shapes.data();
  desc.num_shape_bvh_nodes = (int64_t)made_nodes.size(), desc.shape_bvh_nodes = made_nodes.data();
  desc.num_scene_bvh_nodes = scene_built ? lv.count : 0, desc.scene_bvh_nodes = scene_built ? lv.h_nodes.data() : nullptr;
  scene_tables t;
  t.d = d, t.shapes = shapes;
  t.shape_depths.assign((size_t)n_new, 0), t.shape_need4s.assign((size_t)n_new, 0), t.shape_quads.assign((size_t)n_new, 0);
  for (int j = 0; j < n_new; j++)
    if (!made[(size_t)j]) {
      const int i = list[(size_t)j].old_id;
      t.shape_depths[(size_t)j] = r.shape_depth[(size_t)i], t.shape_need4s[(size_t)j] = r.shape_need4[(size_t)i], t.shape_quads[(size_t)j] = r.shape_quads[(size_t)i];
    }
  t.scene_depth = r.scene_depth, t.scene_need4 = r.scene_need4, t.scene_wnodes = (size_t)(d.shape_wnodes - d.scene_wnodes);
  if (int rc = prep_quad_nodes_and_stacks(desc, t, false, made.data(), !scene_built)) return rc;   // a tree past a limit is refused here, the scene untouched
  // the quad-node table: the scene's part (new, or as it is), the new shapes' from the host, the untouched ones' device to device
  for (int j = 0; j < n_new; j++) now[(size_t)j].len[P_QUADS] = t.shape_quads[(size_t)j];
  new_at[P_QUADS] = offsets_of(now, P_QUADS);
  if (int rc = lv.wnodes.allocate((t.scene_wnodes + t.shape_wnodes) * sizeof(float4))) return rc;
  float4*       n_shape_wnodes = lv.wnodes.get<float4>() + t.scene_wnodes;
  const float4* host_quads     = t.wnodes.data();
  if (scene_built) {
    if (int rc = send(r, lv.wnodes.get<const float4>(), host_quads, t.scene_wnodes)) return rc;
    host_quads += t.scene_wnodes;
  } else if (int rc = copy_on_device(lv.wnodes.get(), d.scene_wnodes, t.scene_wnodes * sizeof(float4))) return rc;
  for (int j = 0; j < n_new; j++) {
    if (!made[(size_t)j]) continue;
    const size_t count = 8 * (size_t)t.shape_quads[(size_t)j];
    if (int rc = send(r, (const float4*)(n_shape_wnodes + 8 * new_at[P_QUADS][(size_t)j]), host_quads, count)) return rc;
    host_quads += count;
  }
  for (const shape_run& run : runs) {
    const long long a = old_at[P_QUADS][(size_t)run.first_old], b = old_at[P_QUADS][(size_t)run.first_old + (size_t)run.count];
    if (int rc = copy_on_device(n_shape_wnodes + 8 * new_at[P_QUADS][(size_t)run.first_new], d.shape_wnodes + 8 * a, (size_t)(b - a) * 8 * sizeof(float4))) return rc;
  }
  // the shape records whole, with wnode_offset, root_ref and stack_need; every root box from the new node pool (the host's copy of an
  // untouched shape's is creation's: the device may have refitted it)
  if (scene_built) {
    if (int rc = send(r, n_shapes.get<const DShape>(), t.shapes.data(), t.shapes.size())) return rc;
  } else if (int rc = send(r, n_shapes, t.shapes)) return rc;
  if (int rc = upd_shape_roots(r, n_shapes.get<DShape>(), n_shape_nodes.get<float4>(), n_new)) return rc;
  if (int rc = scene_level_enter(r, lv, t, inst_shape.data(), n_instances.get<DInstance>(), n_shapes.get<DShape>())) return rc;

  // ---- the last check has passed: the swap of tables, counts and mirrors ------------------------------------------------------
  {
    auto take = [&](auto*& table, device_buffer& fresh) {   // `fresh` becomes the scene's table
      const void* old = table;
      table = fresh.get<std::remove_reference_t<decltype(*table)>>();
      adopt(r.tables, old, std::move(fresh));
    };
    take(d.positions, n_positions), take(d.normals, n_normals), take(d.texcoords, n_texcoords), take(d.colors, n_colors), take(d.elems, n_elems);
    take(d.leaf_prims, n_leaf_prims), take(d.leaf_attrs, n_leaf_attrs), take(d.shape_nodes, n_shape_nodes), take(d.shapes, n_shapes), take(d.instances, n_instances);
    const void *old_tp = d.tri_prims, *old_ta = d.tri_attrs;
    d.tri_prims = compact ? n_tri_prims.get<const float4>() : nullptr, d.tri_attrs = compact ? n_tri_attrs.get<const float4>() : nullptr;
    if (old_tp || compact) adopt(r.tables, old_tp, std::move(n_tri_prims));   // (an empty buffer takes the place of records that go)
    if (old_ta || compact) adopt(r.tables, old_ta, std::move(n_tri_attrs));
  }
  if (scene_built) scene_level_swap(r, lv, t);
  else {   // the scene's nodes and primitive order stay: the quad-node table, the enter records and the slots are new
    const struct { const void* old; device_buffer* fresh; } swaps[3] = {{d.scene_wnodes, &lv.wnodes}, {d.scene_enter, &lv.enter}, {d.slot_of_instance, &lv.d_slot_of}};
    d.scene_wnodes = lv.wnodes.get<const float4>(), d.shape_wnodes = d.scene_wnodes + t.scene_wnodes;
    d.scene_enter = lv.enter.get<const float4>(), d.slot_of_instance = lv.d_slot_of.get<const int>();
    for (const auto& s : swaps) adopt(r.tables, s.old, std::move(*s.fresh));
    h.slot_of = lv.slot_of;
    r.refit.ready = false;   // levels and quad slots are numbered by the old shape list
  }
  d.num_shapes = n_new;
  r.num_positions = n_pos, r.num_normals = n_nrm, r.num_texcoords = n_tc, r.num_colors = n_col;
  r.num_shape_nodes = n_nodes, r.num_shape_wnodes = (long long)t.shape_wnodes;
  r.shape_depth = t.shape_depths, r.shape_need4 = t.shape_need4s, r.shape_quads = t.shape_quads;
  // prim_slot: a survivor's slots move with its leaf offset, a new shape's come from its primitive order
  std::vector<int> prim_slot((size_t)n_elem, -1), shape_elems((size_t)n_new), shape_elem_offset((size_t)n_new), shape_vertices((size_t)n_new);
  for (int j = 0; j < n_new; j++) {
    const DShape& o = t.shapes[(size_t)j];
    shape_elems[(size_t)j] = o.num_elems, shape_elem_offset[(size_t)j] = o.elem_offset, shape_vertices[(size_t)j] = (int)now[(size_t)j].len[P_POSITIONS];
    if (made[(size_t)j]) {
      const mesh& ms = meshes[(size_t)list[(size_t)j].payload];
      for (int k = 0; k < o.num_elems; k++) prim_slot[(size_t)o.elem_offset + (size_t)ms.prims[(size_t)k]] = o.leaf_offset + k;
    } else {
      const DShape& was_shape = m.shapes[(size_t)list[(size_t)j].old_id];
      for (int k = 0; k < o.num_elems; k++) prim_slot[(size_t)o.elem_offset + (size_t)k] = h.prim_slot[(size_t)was_shape.elem_offset + (size_t)k] - was_shape.leaf_offset + o.leaf_offset;
    }
  }
  h.prim_slot = std::move(prim_slot), h.shape_elems = std::move(shape_elems), h.shape_elem_offset = std::move(shape_elem_offset), h.shape_vertices = std::move(shape_vertices);
  h.inst_shape = inst_shape, m.inst_flags = inst_flags, m.shapes = t.shapes, m.shape_flags = flags;
  subdiv_plans_follow_shapes(r, new_of_old, is_set);   // a replaced or removed shape drops its tesselation plan, the others are renumbered
  out.curves = false;
  for (int i = 0; i < ninst; i++) out.curves = out.curves || (inst_flags[(size_t)i] & (VPT_SHP_POINTS | VPT_SHP_LINES)) != 0;
  r.varying_media = prep_media_vary(m.materials.data(), d.num_materials, m.inst_material.data(), m.inst_flags.data(), ninst);
  out.changed = out.topology = true, out.stack_cap = t.stack_cap, out.stack_lds4 = t.stack_lds4, out.stack_spill4 = t.stack_spill4;

  // ---- 6. the lights of the new scene: a light on a replaced shape gets a CDF of the new length and the kind of its new tree --------
  const vpt_scene_edit none = {};
  if (int rc = light_update_apply(r, none, &out.lights_rebuilt, nullptr, nullptr, &light_old_of_new)) return rc;
  if (!out.lights_rebuilt) {   // the same lights: their records name shapes, whose table is new
    if (int rc = upd_light_records(r, d.shapes)) return rc;
    m.shape_lit.assign((size_t)n_new, 0);
    for (const vpt_light& l : m.lights)
      if (l.instance >= 0) m.shape_lit[(size_t)h.inst_shape[(size_t)l.instance]] = 1;
  }
  if (int rc = mark_end(r)) return rc;
  return finish_update(r);
}
