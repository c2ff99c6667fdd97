// vpt_scene_prep.cpp — the host half of vpt_scene_create (vpt_scene_prep.h): validation of a vpt_scene_desc and the tables
// of the device layout (vpt_device.h) built from it.  Host arithmetic only: no kernel, no device call, so every refusal
// happens before a device is touched and the figures can be checked on a machine without one.
#include "vpt_scene_prep.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "vpt_error.h"

namespace {

// host-side float3 helpers for the load-time precomputation (same formulas as the reference)
struct h3 { float x, y, z; };
h3 hcross(h3 a, h3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
float hdot(h3 a, h3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
h3 hmul(h3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
h3 hadd(h3 a, h3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
struct hframe { h3 x, y, z, o; };
hframe to_h(const vpt_frame& f) { return {{f.x[0], f.x[1], f.x[2]}, {f.y[0], f.y[1], f.y[2]}, {f.z[0], f.z[1], f.z[2]}, {f.o[0], f.o[1], f.o[2]}}; }
// inverse(frame3f, non_rigid), yocto_math.h:2948-2956 with inverse(mat3f) = adjoint * (1/det), :2802-2808
hframe hinverse(const hframe& a, bool non_rigid) {
  h3 mx, my, mz;
  if (non_rigid) {
    h3 c0 = hcross(a.y, a.z), c1 = hcross(a.z, a.x), c2 = hcross(a.x, a.y);   // adjoint = transpose{c0,c1,c2}
    float s = 1 / hdot(a.x, hcross(a.y, a.z));
    mx = hmul({c0.x, c1.x, c2.x}, s), my = hmul({c0.y, c1.y, c2.y}, s), mz = hmul({c0.z, c1.z, c2.z}, s);
  } else {
    mx = {a.x.x, a.y.x, a.z.x}, my = {a.x.y, a.y.y, a.z.y}, mz = {a.x.z, a.y.z, a.z.z};
  }
  h3 mo = hadd(hadd(hmul(mx, a.o.x), hmul(my, a.o.y)), hmul(mz, a.o.z));
  return {mx, my, mz, {-mo.x, -mo.y, -mo.z}};
}
void pack_frame(const hframe& f, float4* out) {
  out[0] = make_float4(f.x.x, f.x.y, f.x.z, f.y.x);
  out[1] = make_float4(f.y.y, f.y.z, f.z.x, f.z.y);
  out[2] = make_float4(f.z.z, f.o.x, f.o.y, f.o.z);
}

// Quad nodes (vpt_device.h): one 128-byte record per internal node at even depth, holding the boxes and
// references of its (up to) four grandchildren in the binary BVH: slots 0,1 = children of child 0 (or
// child 0 itself when it is a leaf, slot 1 empty), slots 2,3 likewise for child 1.  Layout: lo.x[4],
// lo.y[4], lo.z[4], hi.x[4], hi.y[4], hi.z[4], ref[4], meta[4].  Low 16 bits of meta[0]: axis | axis0 << 2 | axis1 << 4, of
// meta[1 .. 3]: 0.  High 16 bits of meta[j]: the visit rank of slot j in the reference's order, two bits for each of the 8 sign
// octants of a ray's direction (bits 16 + 2 s, s = sign_bits): a function of the three axes, tabulated here so that the group form
// of the node step reads it with the word it loads anyway (this function is the row's only writer: edits rewrite rows 0 .. 5).
// ref >= 0: quad node (relative to this BVH), ~ref = start << 4 | count: leaf, VPT_NONE_REF: empty slot.
// Returns the reference of the root and its box, appends to `out`; *need = worst-case number of stack
// entries a traversal of this BVH holds at once (three pending siblings per quad level).
constexpr int VPT_NONE_REF = -2147483647 - 1;
// the (up to) four binary nodes behind the slots of the quad node made from internal binary node i (-1: empty slot), and the split axes
void quad_slots_of(const vpt_bvh_node* nodes, int i, int slot[4], int axes[3]) {
  axes[0] = nodes[i].axis, axes[1] = axes[2] = 0;
  for (int side = 0; side < 2; side++) {
    int c = nodes[i].start + side;
    if (nodes[c].internal) slot[2 * side] = nodes[c].start, slot[2 * side + 1] = nodes[c].start + 1, axes[1 + side] = nodes[c].axis;
    else slot[2 * side] = c, slot[2 * side + 1] = -1;
  }
}
// binary nodes that become quad nodes, in depth-first preorder (a node's subtree stays close to it): order[n] = the binary node of
// quad node n, quad_of[i] = the quad node of binary node i (-1: none).  A BVH without nodes or whose root is a leaf has no quad nodes.
void quad_order(const vpt_bvh_node* nodes, int count, std::vector<int>& order, std::vector<int>& quad_of) {
  order.clear(), quad_of.assign((size_t)(count > 0 ? count : 0), -1);
  if (count <= 0 || !nodes[0].internal) return;
  std::vector<int> todo{0};
  while (!todo.empty()) {
    int i = todo.back();
    todo.pop_back();
    quad_of[(size_t)i] = (int)order.size();
    order.push_back(i);
    int slot[4], axes[3];
    quad_slots_of(nodes, i, slot, axes);
    for (int k = 3; k >= 0; k--)
      if (slot[k] >= 0 && nodes[slot[k]].internal) todo.push_back(slot[k]);
  }
}
int build_quad_nodes(const vpt_bvh_node* nodes, int count, std::vector<float4>& out, float root_box[6], int* need) {
  for (int k = 0; k < 6; k++) root_box[k] = 0;
  *need = 0;
  if (count <= 0) return ~0;   // empty leaf
  for (int k = 0; k < 3; k++) root_box[k] = nodes[0].bbox_min[k], root_box[3 + k] = nodes[0].bbox_max[k];
  auto leaf_code = [&](int i) { return ~((nodes[i].start << 4) | (nodes[i].num & 15)); };
  if (!nodes[0].internal) return leaf_code(0);
  std::vector<int> quad_of, order;
  quad_order(nodes, count, order, quad_of);
  auto slots_of = [&](int i, int slot[4], int axes[3]) { quad_slots_of(nodes, i, slot, axes); };
  size_t base = out.size();
  out.resize(base + 8 * order.size());
  std::vector<int> node_need(order.size(), 0);
  for (size_t n = order.size(); n-- > 0;) {   // children come after their parent in preorder: fill bottom-up
    int i = order[n], slot[4], axes[3];
    slots_of(i, slot, axes);
    float box[6][4];
    int   ref[4], present = 0, deepest = 0;
    for (int k = 0; k < 4; k++) {
      for (int c = 0; c < 6; c++) box[c][k] = 0;
      ref[k] = VPT_NONE_REF;
      if (slot[k] < 0) continue;
      const vpt_bvh_node& ch = nodes[slot[k]];
      for (int c = 0; c < 3; c++) box[c][k] = ch.bbox_min[c], box[3 + c][k] = ch.bbox_max[c];
      ref[k] = ch.internal ? quad_of[(size_t)slot[k]] : leaf_code(slot[k]);
      present++;
      if (ch.internal && node_need[(size_t)quad_of[(size_t)slot[k]]] > deepest) deepest = node_need[(size_t)quad_of[(size_t)slot[k]]];
    }
    node_need[n] = present - 1 + deepest;
    float4* q = &out[base + 8 * n];
    for (int c = 0; c < 6; c++) q[c] = make_float4(box[c][0], box[c][1], box[c][2], box[c][3]);
    memcpy(&q[6], ref, 16);
    // visit ranks: for octant s of a ray's direction (bit a set: negative along axis a) the reference reaches the child on the far
    // side of the node's axis last, and likewise one level down; a leaf child counts as axis 0 (its second slot is empty)
    unsigned meta[4] = {(unsigned)(axes[0] | (axes[1] << 2) | (axes[2] << 4)), 0, 0, 0};
    for (int j = 0; j < 4; j++)
      for (int s = 0; s < 8; s++) {
        const int gn = (s >> axes[0]) & 1, g0 = (s >> axes[1]) & 1, g1 = (s >> axes[2]) & 1, grp = j >> 1;
        const unsigned k = (unsigned)(((grp ^ gn) << 1) | ((j & 1) ^ (grp ? g1 : g0)));
        meta[j] |= k << (16 + 2 * s);
      }
    memcpy(&q[7], meta, 16);
  }
  *need = node_need[0];
  return 0;
}

int bvh_depth(const vpt_bvh_node* nodes, int count, int root, int depth, int limit) {
  if (depth > limit) return depth;
  const vpt_bvh_node& n = nodes[root];
  if (!n.internal) return depth;
  int a = bvh_depth(nodes, count, n.start, depth + 1, limit), b = bvh_depth(nodes, count, n.start + 1, depth + 1, limit);
  return a > b ? a : b;
}

int check_nodes(const vpt_bvh_node* nodes, long long count, long long nprims, const char* what) {
  for (long long i = 0; i < count; i++) {
    const vpt_bvh_node& n = nodes[i];
    if (n.internal) REQUIRE(n.start > i && (long long)n.start + 1 < count, "%s bvh node %lld: bad children", what, i);
    else REQUIRE(n.start >= 0 && n.num >= 0 && n.num <= 15 && n.start < (1 << 27) && (long long)n.start + n.num <= nprims, "%s bvh node %lld: bad leaf range", what, i);
    REQUIRE(n.axis >= 0 && n.axis <= 2, "%s bvh node %lld: bad axis", what, i);
  }
  return VPT_OK;
}

// the points / lines entry of shape i (all zero when the descriptor has no side array)
vpt_shape_curves curves_of(const vpt_scene_curves& cs, int i) {
  vpt_shape_curves c = {0, 0, 0, 0, -1};
  if (cs.shape_curves) c = cs.shape_curves[i];
  return c;
}
bool has_curves(const vpt_scene_curves& cs, int i) {
  vpt_shape_curves c = curves_of(cs, i);
  return c.num_points != 0 || c.num_lines != 0;
}

int validate(const vpt_scene_desc& d, const vpt_scene_curves& cs) {
  REQUIRE(d.num_cameras > 0 && d.cameras, "scene has no cameras");
#define TABLE(n, p) REQUIRE((n) >= 0 && ((n) == 0 || (p) != nullptr), "table %s is null", #p)
  TABLE(d.num_instances, d.instances); TABLE(d.num_shapes, d.shapes); TABLE(d.num_materials, d.materials);
  TABLE(d.num_textures, d.textures); TABLE(d.num_environments, d.environments); TABLE(d.num_volumes, d.volumes);
  TABLE(d.num_vol_instances, d.vol_instances); TABLE(d.num_sdfs, d.sdfs); TABLE(d.num_lights, d.lights);
  TABLE(d.num_positions, d.positions); TABLE(d.num_normals, d.normals); TABLE(d.num_texcoords, d.texcoords);
  TABLE(d.num_colors, d.colors); TABLE(d.num_triangles, d.triangles); TABLE(d.num_quads, d.quads);
  TABLE(d.num_texels_f, d.texels_f); TABLE(d.num_texels_b, d.texels_b); TABLE(d.num_voxels, d.voxels);
  TABLE(d.num_light_cdf, d.light_cdf); TABLE(d.num_scene_bvh_nodes, d.scene_bvh_nodes);
  TABLE(d.num_scene_bvh_prims, d.scene_bvh_prims); TABLE(d.num_shape_bvh_nodes, d.shape_bvh_nodes);
  TABLE(d.num_shape_bvh_prims, d.shape_bvh_prims);
  TABLE(cs.num_points, cs.points); TABLE(cs.num_lines, cs.lines); TABLE(cs.num_radius, cs.radius);
#undef TABLE
  auto tex_ok = [&](int t) { return t >= -1 && t < d.num_textures; };
  for (int i = 0; i < d.num_shapes; i++) {
    const vpt_shape& s = d.shapes[i];
    REQUIRE(s.num_vertices >= 0 && s.position_offset >= 0 && (long long)s.position_offset + s.num_vertices <= d.num_positions, "shape %d: positions out of range", i);
    REQUIRE(s.normal_offset == -1 || (s.normal_offset >= 0 && (long long)s.normal_offset + s.num_vertices <= d.num_normals), "shape %d: normals out of range", i);
    REQUIRE(s.texcoord_offset == -1 || (s.texcoord_offset >= 0 && (long long)s.texcoord_offset + s.num_vertices <= d.num_texcoords), "shape %d: texcoords out of range", i);
    REQUIRE(s.color_offset == -1 || (s.color_offset >= 0 && (long long)s.color_offset + s.num_vertices <= d.num_colors), "shape %d: colors out of range", i);
    REQUIRE(s.num_triangles >= 0 && s.triangle_offset >= 0 && (long long)s.triangle_offset + s.num_triangles <= d.num_triangles, "shape %d: triangles out of range", i);
    REQUIRE(s.num_quads >= 0 && s.quad_offset >= 0 && (long long)s.quad_offset + s.num_quads <= d.num_quads, "shape %d: quads out of range", i);
    long long nel = s.num_triangles ? s.num_triangles : s.num_quads;
    const vpt_shape_curves c = curves_of(cs, i);
    REQUIRE(c.num_points >= 0 && c.point_offset >= 0 && (long long)c.point_offset + c.num_points <= cs.num_points, "shape %d: points out of range", i);
    REQUIRE(c.num_lines >= 0 && c.line_offset >= 0 && (long long)c.line_offset + c.num_lines <= cs.num_lines, "shape %d: lines out of range", i);
    if (c.num_points || c.num_lines) {
      REQUIRE((c.num_points != 0) + (c.num_lines != 0) + (nel != 0) > 1 || (c.radius_offset >= 0 && (long long)c.radius_offset + s.num_vertices <= cs.num_radius),
          "shape %d: radius out of range", i);
      nel = c.num_points ? c.num_points : c.num_lines;
    }
    if (int rc = prep_check_shape_elements(i, s.num_vertices, s.num_triangles ? d.triangles + 3LL * s.triangle_offset : nullptr, s.num_triangles,
            s.num_quads ? d.quads + 4LL * s.quad_offset : nullptr, s.num_quads, c.num_points ? cs.points + c.point_offset : nullptr, c.num_points,
            c.num_lines ? cs.lines + 2LL * c.line_offset : nullptr, c.num_lines))
      return rc;
    REQUIRE(s.num_bvh_nodes >= 0 && s.bvh_node_offset >= 0 && (long long)s.bvh_node_offset + s.num_bvh_nodes <= d.num_shape_bvh_nodes, "shape %d: bvh nodes out of range", i);
    REQUIRE(s.bvh_prim_offset >= 0 && (long long)s.bvh_prim_offset + nel <= d.num_shape_bvh_prims, "shape %d: bvh prims out of range", i);
    if (int rc = check_nodes(d.shape_bvh_nodes + s.bvh_node_offset, s.num_bvh_nodes, nel, "shape")) return rc;
    for (long long k = 0; k < nel; k++) {
      int e = d.shape_bvh_prims[s.bvh_prim_offset + k];
      REQUIRE(e >= 0 && e < nel, "shape %d: bvh primitive id out of range", i);
    }
  }
  for (int i = 0; i < d.num_instances; i++) {
    REQUIRE(d.instances[i].shape >= 0 && d.instances[i].shape < d.num_shapes, "instance %d: bad shape", i);
    REQUIRE(d.instances[i].material >= 0 && d.instances[i].material < d.num_materials, "instance %d: bad material", i);
  }
  // Texture ids are only dereferenced for materials bound to mesh instances (eval_material with
  // texcoords, yocto_scene.cpp:529); materials used only by SDFs / voxel grids go through the
  // texture-free eval_material(scene,int) (:581) and the reference tolerates dangling ids there
  // (tests/06_gridsdf ships some), so range-check only what the device can read.
  std::vector<char> textured((size_t)d.num_materials, 0);
  for (int i = 0; i < d.num_instances; i++) textured[(size_t)d.instances[i].material] = 1;
  for (int i = 0; i < d.num_materials; i++) {
    const vpt_material& m = d.materials[i];
    if (int rc = prep_check_material(m, i, d.num_textures, textured[(size_t)i] != 0)) return rc;
  }
  for (int i = 0; i < d.num_textures; i++) {
    const vpt_texture& t = d.textures[i];
    long long n = (long long)t.width * t.height;
    REQUIRE(t.width >= 0 && t.height >= 0 && t.offset >= 0 && t.offset + n <= (t.is_float ? d.num_texels_f : d.num_texels_b), "texture %d: texels out of range", i);
  }
  for (int i = 0; i < d.num_environments; i++) REQUIRE(tex_ok(d.environments[i].emission_tex), "environment %d: bad texture", i);
  for (int i = 0; i < d.num_volumes; i++) {
    const vpt_volume& v = d.volumes[i];
    REQUIRE(v.whd[0] >= 0 && v.whd[1] >= 0 && v.whd[2] >= 0 && v.offset >= 0 && v.offset + (long long)v.whd[0] * v.whd[1] * v.whd[2] <= d.num_voxels, "volume %d: voxels out of range", i);
    REQUIRE((long long)v.whd[0] * v.whd[1] * v.whd[2] < (1ll << 31), "volume %d: 2^31 voxels or more", i);   // eval_volume indexes a volume with 32-bit arithmetic
  }
  for (int i = 0; i < d.num_vol_instances; i++) {
    REQUIRE(d.vol_instances[i].volume >= 0 && d.vol_instances[i].volume < d.num_volumes, "vol_instance %d: bad volume", i);
    REQUIRE(d.vol_instances[i].material >= 0 && d.vol_instances[i].material < d.num_materials, "vol_instance %d: bad material", i);
  }
  for (int i = 0; i < d.num_sdfs; i++) {
    REQUIRE(d.sdfs[i].type >= 0 && d.sdfs[i].type <= VPT_SDF_TORUS, "sdf %d: bad type", i);
    REQUIRE(d.sdfs[i].material >= 0 && d.sdfs[i].material < d.num_materials, "sdf %d: bad material", i);
  }
  for (int i = 0; i < d.num_lights; i++) {
    const vpt_light& l = d.lights[i];
    REQUIRE(l.instance >= -1 && l.instance < d.num_instances && l.environment >= -1 && l.environment < d.num_environments && l.sdf >= -1 && l.sdf < d.num_sdfs, "light %d: bad reference", i);
    REQUIRE(l.cdf_len >= 0 && l.cdf_offset >= 0 && l.cdf_offset + l.cdf_len <= d.num_light_cdf, "light %d: cdf out of range", i);
    if (l.instance >= 0) {
      const vpt_shape& s = d.shapes[d.instances[l.instance].shape];
      REQUIRE(l.cdf_len == (s.num_triangles ? s.num_triangles : s.num_quads) && l.cdf_len > 0, "light %d: cdf length != element count", i);
    } else if (l.sdf >= 0) {
      REQUIRE(l.cdf_len == 1, "light %d: sdf light needs a 1-entry cdf", i);
    } else if (l.environment >= 0 && d.environments[l.environment].emission_tex >= 0) {
      const vpt_texture& t = d.textures[d.environments[l.environment].emission_tex];
      REQUIRE(l.cdf_len == t.width * t.height && l.cdf_len > 0, "light %d: cdf length != texel count", i);
    }
  }
  if (int rc = check_nodes(d.scene_bvh_nodes, d.num_scene_bvh_nodes, d.num_scene_bvh_prims, "scene")) return rc;
  for (int i = 0; i < d.num_scene_bvh_prims; i++) REQUIRE(d.scene_bvh_prims[i] >= 0 && d.scene_bvh_prims[i] < d.num_instances, "scene bvh: bad instance id");
  {   // the single-instance query of the mesh-light pdf walk enters an instance through its scene-BVH slot
    std::vector<char> in_bvh((size_t)d.num_instances, 0);
    for (int i = 0; i < d.num_scene_bvh_prims; i++) in_bvh[(size_t)d.scene_bvh_prims[i]] = 1;
    for (int i = 0; i < d.num_lights; i++)
      if (d.lights[i].instance >= 0) REQUIRE(in_bvh[(size_t)d.lights[i].instance], "light %d: its instance is not in the scene bvh", i);
  }
  return VPT_OK;
}

// vertex pools, shapes and elements, leaf records and their vertex attributes, the compact records of a scene of triangles
void build_geometry(const vpt_scene_desc& d, const vpt_scene_curves& cs, scene_tables& t) {
  t.positions.resize((size_t)d.num_positions), t.normals.resize((size_t)d.num_normals), t.colors.resize((size_t)d.num_colors);
  t.texcoords.resize((size_t)d.num_texcoords);
  for (long long i = 0; i < d.num_positions; i++) t.positions[i] = make_float4(d.positions[3 * i], d.positions[3 * i + 1], d.positions[3 * i + 2], 0);
  for (long long i = 0; i < d.num_normals; i++) t.normals[i] = make_float4(d.normals[3 * i], d.normals[3 * i + 1], d.normals[3 * i + 2], 0);
  for (long long i = 0; i < d.num_colors; i++) t.colors[i] = make_float4(d.colors[4 * i], d.colors[4 * i + 1], d.colors[4 * i + 2], d.colors[4 * i + 3]);
  for (long long i = 0; i < d.num_texcoords; i++) t.texcoords[i] = make_float2(d.texcoords[2 * i], d.texcoords[2 * i + 1]);

  std::vector<float4>& leafs = t.leaf_prims;
  t.shapes.resize((size_t)d.num_shapes);
  for (int i = 0; i < d.num_shapes; i++) {
    const vpt_shape& sh = d.shapes[i];
    DShape& o = t.shapes[i];
    o = {};
    o.num_nodes = sh.num_bvh_nodes, o.node_offset = sh.bvh_node_offset;
    o.is_triangles = sh.num_triangles != 0;
    o.num_elems = o.is_triangles ? sh.num_triangles : sh.num_quads;
    const vpt_shape_curves cv = curves_of(cs, i);
    const int kind = cv.num_points ? VPT_LEAF_POINT : cv.num_lines ? VPT_LEAF_LINE : 0;
    if (kind) o.num_elems = kind == VPT_LEAF_POINT ? cv.num_points : cv.num_lines;
    o.elem_offset = (int)t.elems.size(), o.leaf_offset = (int)(leafs.size() / 4);
    o.vertex_offset = sh.position_offset, o.normal_offset = sh.normal_offset;
    o.texcoord_offset = sh.texcoord_offset, o.color_offset = sh.color_offset;
    for (int e = 0; e < o.num_elems; e++) {
      if (kind == VPT_LEAF_POINT) {   // elements of points and lines repeat their last vertex, like a triangle's
        int p = cs.points[(long long)cv.point_offset + e];
        t.elems.push_back(make_int4(p, p, p, p));
      } else if (kind == VPT_LEAF_LINE) {
        const int32_t* l = cs.lines + 2LL * (cv.line_offset + e);
        t.elems.push_back(make_int4(l[0], l[1], l[1], l[1]));
      } else if (o.is_triangles) {
        const int32_t* tr = d.triangles + 3LL * (sh.triangle_offset + e);
        t.elems.push_back(make_int4(tr[0], tr[1], tr[2], tr[2]));
      } else {
        const int32_t* q = d.quads + 4LL * (sh.quad_offset + e);
        t.elems.push_back(make_int4(q[0], q[1], q[2], q[3]));
      }
    }
    t.h.shape_elems.push_back(o.num_elems), t.h.shape_elem_offset.push_back(o.elem_offset), t.h.shape_vertices.push_back(sh.num_vertices);
    t.h.prim_slot.resize(t.elems.size(), -1);
    // leaf records in BVH primitive order: slot k holds element prims[k]'s corners
    for (int k = 0; k < o.num_elems; k++) {
      int  e = d.shape_bvh_prims[sh.bvh_prim_offset + k];
      t.h.prim_slot[(size_t)o.elem_offset + e] = o.leaf_offset + k;
      int4 q = t.elems[(size_t)o.elem_offset + e];
      if (kind) {   // vpt_device.h: VPT_LEAF_POINT / VPT_LEAF_LINE
        const float* rad = cs.radius + cv.radius_offset;
        float4 p0 = t.positions[(size_t)sh.position_offset + q.x], p1 = t.positions[(size_t)sh.position_offset + q.y];
        float4 r[4] = {p0, kind == VPT_LEAF_LINE ? p1 : make_float4(rad[q.x], 0, 0, 0), make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0)};
        if (kind == VPT_LEAF_LINE) r[1].w = 0, r[2] = make_float4(rad[q.x], rad[q.y], 0, 0);
        memcpy(&r[0].w, &e, 4), memcpy(&r[3].w, &kind, 4);
        for (int c = 0; c < 4; c++) leafs.push_back(r[c]);
      } else {
        for (int c = 0; c < 4; c++) {
          int    v = c == 0 ? q.x : c == 1 ? q.y : c == 2 ? q.z : q.w;
          float4 p = t.positions[(size_t)sh.position_offset + v];
          int    tag = c == 0 ? e : 0;
          memcpy(&p.w, &tag, 4);
          leafs.push_back(p);
        }
      }
      // the corners' normals, then their texcoords (zeros where the shape has none: never read then)
      float tc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int c = 0; c < 4; c++) {
        int v = c == 0 ? q.x : c == 1 ? q.y : c == 2 ? q.z : q.w;
        t.leaf_attrs.push_back(sh.normal_offset >= 0 ? t.normals[(size_t)sh.normal_offset + v] : make_float4(0, 0, 0, 0));
        if (sh.texcoord_offset >= 0) tc[2 * c] = t.texcoords[(size_t)sh.texcoord_offset + v].x, tc[2 * c + 1] = t.texcoords[(size_t)sh.texcoord_offset + v].y;
      }
      t.leaf_attrs.push_back(make_float4(tc[0], tc[1], tc[2], tc[3]));
      t.leaf_attrs.push_back(make_float4(tc[4], tc[5], tc[6], tc[7]));
    }
  }
  leafs.resize(leafs.size() + 8, make_float4(0, 0, 0, 0));   // phase B fetches one record ahead of the one it tests
  // every shape holds triangles: the compact records beside the general ones (vpt_device.h: tri_prims / tri_attrs)
  bool all_triangles = d.num_shapes > 0 && !getenv("VPT_NO_COMPACT_TRIANGLES");
  for (int i = 0; i < d.num_shapes; i++) all_triangles = all_triangles && t.shapes[i].is_triangles && t.shapes[i].num_elems > 0;
  if (all_triangles) {
    const size_t slots = t.leaf_attrs.size() / 6;
    std::vector<float4>&tp = t.tri_prims, &ta = t.tri_attrs;
    tp.assign(3 * slots + 8, make_float4(0, 0, 0, 0)), ta.resize(4 * slots);   // (+ 8: phase B fetches one record ahead, as above)
    for (size_t k = 0; k < slots; k++) {
      const float4 *p = &leafs[4 * k], *a = &t.leaf_attrs[6 * k];
      for (int c = 0; c < 3; c++) tp[3 * k + c] = p[c], ta[4 * k + c] = a[c];
      ta[4 * k + 0].w = a[4].x, ta[4 * k + 1].w = a[4].y, ta[4 * k + 2].w = a[4].z;
      ta[4 * k + 3] = make_float4(a[4].w, a[5].x, a[5].y, 0);
    }
  }
}

// instance records, the enter records of the scene-BVH slots, and the inverse frames of environments
void build_instances(const vpt_scene_desc& d, const vpt_scene_curves& cs, scene_tables& t) {
  t.instances.resize((size_t)d.num_instances);
  t.m.shape_flags.resize((size_t)d.num_shapes);   // of every shape, instanced or not: vpt_scene_update_instances may bind it later
  for (int i = 0; i < d.num_shapes; i++) {
    const vpt_shape& sh = d.shapes[i];
    t.m.shape_flags[(size_t)i] = (sh.num_triangles != 0 ? VPT_SHP_TRIANGLES : 0) | (sh.normal_offset >= 0 ? VPT_SHP_NORMALS : 0) |
                                 (sh.texcoord_offset >= 0 ? VPT_SHP_TEXCOORDS : 0) | (sh.color_offset >= 0 ? VPT_SHP_COLORS : 0) |
                                 (curves_of(cs, i).num_points ? VPT_SHP_POINTS : 0) | (curves_of(cs, i).num_lines ? VPT_SHP_LINES : 0);
  }
  for (int i = 0; i < d.num_instances; i++) {
    DInstance& in = t.instances[i];
    in = {};
    prep_instance_frames(d.instances[i].frame, in.inv, in.fwd, &in.translation_only);
    in.shape = d.instances[i].shape, in.material = d.instances[i].material;
    in.shape_flags = t.m.shape_flags[(size_t)in.shape];
    t.curves = t.curves || has_curves(cs, in.shape);
    t.h.inst_shape.push_back(d.instances[i].shape);
  }
  t.enter.resize((size_t)d.num_scene_bvh_prims * 6);
  t.h.slot_of.assign((size_t)d.num_instances, -1);
  for (int k = 0; k < d.num_scene_bvh_prims; k++) {
    int id = d.scene_bvh_prims[k];
    const DInstance& in = t.instances[(size_t)id];
    const DShape&    sh = t.shapes[(size_t)in.shape];
    float4* e = &t.enter[6 * (size_t)k];
    // (vpt_scene_update.hip rewrites e0..e2, the root box and translation_only of a resident scene in place: keep the two in step)
    e[0] = in.inv[0], e[1] = in.inv[1], e[2] = in.inv[2];
    e[3] = make_float4(sh.root_box[0], sh.root_box[1], sh.root_box[2], sh.root_box[3]);
    e[4] = make_float4(sh.root_box[4], sh.root_box[5], 0, 0);
    prep_enter_tail(e, sh, (int)(t.scene_wnodes / 8), id, in.translation_only);
    t.h.slot_of[(size_t)id] = k;
  }
  t.env_inv.resize((size_t)d.num_environments * 3);
  for (int i = 0; i < d.num_environments; i++) {
    float4 fwd[3];
    prep_environment_frames(d.environments[i].frame, &t.env_inv[3 * (size_t)i], fwd);
  }
}

// the features the lights need, the 16-ary search index and guide table over each light's CDF (vpt_device.h: DCdfIndex), light records
void build_lights(const vpt_scene_desc& d, scene_tables& t) {
  for (int i = 0; i < d.num_lights; i++)
    if (d.lights[i].instance >= 0) {
      int ref = t.shapes[(size_t)d.instances[d.lights[i].instance].shape].root_ref;
      t.light_features |= (ref >= 0 || ((~ref) & 15) > 4) ? VPT_FEAT_LARGE_LIGHTS : VPT_FEAT_SMALL_LIGHTS;
    } else if (d.lights[i].sdf >= 0) t.light_features |= VPT_FEAT_SDF_LIGHTS;

  const float inf = std::numeric_limits<float>::infinity();
  std::vector<float>& pool = t.light_index_pool;
  t.light_index.resize((size_t)d.num_lights);
  for (int i = 0; i < d.num_lights; i++) {
    DCdfIndex& ix = t.light_index[(size_t)i];
    ix = {};
    const float* c = d.light_cdf + d.lights[i].cdf_offset;
    long long    n = d.lights[i].cdf_len;
    bool sorted = n > 64;
    for (long long k = 1; sorted && k < n; k++) sorted = c[k - 1] <= c[k];   // false for NaN too
    if (!sorted) continue;
    std::vector<float> level(c, c + n);
    size_t mark = pool.size();
    while (true) {
      if (ix.levels == 8) { ix.levels = 0; break; }   // > 16^8 entries: keep the binary search
      ix.offset[ix.levels++] = (int)pool.size();
      ix.top_count = (int)level.size();
      pool.insert(pool.end(), level.begin(), level.end());
      pool.resize((pool.size() + 15) / 16 * 16 + (ix.levels == 1 ? 16 : 0), inf);   // level 0 is also read 16-wide from any index
      if (level.size() <= 16) break;
      std::vector<float> up((level.size() + 15) / 16);
      for (size_t g = 0; g < up.size(); g++) up[g] = level[std::min(level.size() - 1, 16 * g + 15)];
      level.swap(up);
    }
    if (ix.levels == 0) { pool.resize(mark); continue; }
    // guide table: n/4 buckets over [0, back); bracket = upper_bound of a lower / an upper bound of the bucket's r
    float back = c[n - 1];
    long long M = n / 4;
    float scale = (float)M / back;
    if (!(back > 0) || !std::isfinite(scale) || M < 16) continue;
    ix.guide_offset = (int)t.light_guide.size(), ix.guide_buckets = (int)M, ix.guide_scale = scale;
    for (long long b = 0; b < M; b++) {
      // fl(r * scale) in [b, b+1)  =>  r in [b (1 - 2^-24) / scale, (b+1) (1 + 2^-23) / scale]; widened further
      double lo_r = (double)b * (1.0 - 1.0 / 8388608.0) / (double)scale, hi_r = (double)(b + 1) * (1.0 + 1.0 / 4194304.0) / (double)scale;
      float  lf = std::nextafter((float)lo_r, -inf), hf = std::nextafter((float)hi_r, inf);
      int lo = b == 0 ? 0 : (int)(std::upper_bound(c, c + n, lf) - c);
      int hi = b == M - 1 ? (int)n : (int)(std::upper_bound(c, c + n, hf) - c);
      t.light_guide.push_back(make_int2(lo, hi));
    }
  }

  t.light_rec.assign(8 * (size_t)d.num_lights + 3 * (size_t)d.num_materials, make_float4(0, 0, 0, 0));   // + the medium records, filled on the device
  for (int i = 0; i < d.num_lights; i++) {
    const vpt_light& l = d.lights[i];
    float4* r = &t.light_rec[8 * (size_t)i];
    float   total = l.cdf_len > 0 ? d.light_cdf[l.cdf_offset + l.cdf_len - 1] : 0.0f;
    int     kind = VPT_LIGHT_NONE, count = 0;
    if (l.instance != VPT_INVALID) {
      const DInstance& in = t.instances[(size_t)l.instance];
      const DShape&    sh = t.shapes[(size_t)in.shape];
      // a shape whose BVH is one leaf of <= 4 primitives (the reference's bvh_max_prims) is walked inline from the light's own
      // copy of them (light_prims holds four); anything else goes through the traversal
      bool small = sh.root_ref < 0 && ((~sh.root_ref) & 15) <= 4;
      kind  = small ? VPT_LIGHT_SMALL_MESH : VPT_LIGHT_LARGE_MESH;
      count = small ? ((~sh.root_ref) & 15) : 0;
      for (int k = 0; k < 3; k++) r[k] = in.inv[k], r[3 + k] = in.fwd[k];
      r[6] = make_float4(sh.root_box[0], sh.root_box[1], sh.root_box[2], total);
      r[7] = make_float4(sh.root_box[3], sh.root_box[4], sh.root_box[5], 0);
    } else if (l.sdf != VPT_INVALID) {
      kind = VPT_LIGHT_SDF;
    } else if (l.environment != VPT_INVALID && d.environments[l.environment].emission_tex == VPT_INVALID) {
      kind = VPT_LIGHT_ENV_CONST;
    } else if (l.environment != VPT_INVALID) {
      kind = VPT_LIGHT_ENV_TEX;
      const vpt_texture& tx = d.textures[d.environments[l.environment].emission_tex];
      prep_environment_frames(d.environments[l.environment].frame, &r[0], &r[3]);
      int dims[2] = {tx.width, tx.height};
      memcpy(&r[6].x, dims, 8);
      r[6].z = total;
    }
    int tag = kind | (count << 8);
    memcpy(&r[7].w, &tag, 4);
  }
}

// what the edits of the resident scene keep on the host (edit_mirrors): the descriptor's small tables and what the tables above say
// about them, while both are at hand
void build_edit_mirrors(const vpt_scene_desc& d, scene_tables& t) {
  edit_mirrors& m = t.m;
  m.materials.assign(d.materials, d.materials + d.num_materials), m.environments.assign(d.environments, d.environments + d.num_environments);
  m.textures.assign(d.textures, d.textures + d.num_textures), m.lights.assign(d.lights, d.lights + d.num_lights);
  m.sdfs.assign(d.sdfs, d.sdfs + d.num_sdfs), m.volumes.assign(d.volumes, d.volumes + d.num_volumes);
  m.vol_instances.assign(d.vol_instances, d.vol_instances + d.num_vol_instances);
  m.shapes = t.shapes, m.light_index = t.light_index;
  m.textured.assign((size_t)d.num_materials, 0), m.shape_lit.assign((size_t)d.num_shapes, 0);
  for (const DInstance& in : t.instances) m.textured[(size_t)in.material] = 1, m.inst_material.push_back(in.material), m.inst_flags.push_back(in.shape_flags);
  for (int l = 0; l < d.num_lights; l++) {
    int tag;
    memcpy(&tag, &t.light_rec[8 * (size_t)l + 7].w, 4);
    m.light_kind.push_back(tag & 255);
    if (d.lights[l].instance >= 0) m.shape_lit[(size_t)t.instances[(size_t)d.lights[l].instance].shape] = 1;
  }
  m.num_cdf = d.num_light_cdf, m.num_pool = (long long)t.light_index_pool.size(), m.num_guide = (long long)t.light_guide.size();
  m.num_texels_f = d.num_texels_f, m.num_texels_b = d.num_texels_b, m.num_voxels = d.num_voxels;
}

}  // namespace

void prep_instance_frames(const vpt_frame& frame, float4 inv[3], float4 fwd[3], int* translation_only) {
  hframe f = to_h(frame);
  pack_frame(hinverse(f, true), inv);
  pack_frame(f, fwd);
  *translation_only = f.x.x == 1 && f.x.y == 0 && f.x.z == 0 && f.y.x == 0 && f.y.y == 1 && f.y.z == 0 &&
                      f.z.x == 0 && f.z.y == 0 && f.z.z == 1;
}
void prep_environment_frames(const vpt_frame& frame, float4 inv[3], float4 fwd[3]) {
  pack_frame(hinverse(to_h(frame), false), inv);
  pack_frame(to_h(frame), fwd);
}
int prep_check_material(const vpt_material& m, int i, int num_textures, bool textured) {
  auto tex_ok = [&](int t) { return t >= -1 && t < num_textures; };
  REQUIRE(m.type >= 0 && m.type <= VPT_MAT_GLTFPBR, "material %d: bad type", i);
  if (!textured) return VPT_OK;
  REQUIRE(tex_ok(m.emission_tex) && tex_ok(m.color_tex) && tex_ok(m.roughness_tex) && tex_ok(m.scattering_tex) && tex_ok(m.normal_tex), "material %d: texture id out of range", i);
  return VPT_OK;
}
int prep_check_shape_elements(int i, int num_vertices, const int32_t* triangles, int num_triangles, const int32_t* quads, int num_quads, const int32_t* points,
    int num_points, const int32_t* lines, int num_lines) {
  REQUIRE(num_triangles == 0 || num_quads == 0, "shape %d: both triangles and quads", i);
  // the reference's BVH tests points, then lines, then faces; its eval_* functions faces first: a mixed shape has no single behaviour
  if ((num_points || num_lines) && (num_points != 0) + (num_lines != 0) + (num_triangles != 0 || num_quads != 0) > 1)
    return vpt_set_error(VPT_ERR_UNSUPPORTED, "shape %d mixes points, lines and faces", i);
  const struct { const int32_t* v; long long n; const char* what; } lists[4] = {{points, num_points, "point"}, {lines, 2LL * num_lines, "line"},
      {triangles, 3LL * num_triangles, "triangle"}, {quads, 4LL * num_quads, "quad"}};
  for (const auto& l : lists)
    for (long long k = 0; k < l.n; k++) REQUIRE(l.v[k] >= 0 && l.v[k] < num_vertices, "shape %d: %s vertex index out of range", i, l.what);
  return VPT_OK;
}
bool prep_media_vary(const vpt_material* materials, int num_materials, const int* inst_material, const int* inst_flags, int num_instances) {
  if (num_materials > 65534) return true;
  for (int i = 0; i < num_instances; i++) {
    const vpt_material& m = materials[inst_material[i]];
    if (m.type != VPT_MAT_REFRACTIVE && m.type != VPT_MAT_VOLUMETRIC && m.type != VPT_MAT_SUBSURFACE) continue;   // is_volumetric_type
    if (m.color_tex != VPT_INVALID || m.emission_tex != VPT_INVALID || m.scattering_tex != VPT_INVALID || (inst_flags[i] & VPT_SHP_COLORS)) return true;
  }
  return false;
}

// SDF evaluation records (vpt_scene.hip.h "SDF records") and the balls the escaping-ray early-out needs.  The
// constants are folded with the reference's own float operations (yocto_sdfs.cpp:33-38, yocto_sceneio.cpp:3697);
// the balls are test-independent geometry, computed in double with a 5 % margin.  Only rigid frames get a ball
// (a scaling frame turns SDF values into something other than world distances): radius -1 switches the early-out off.
// The inverse frames of the SDFs (rigid) come with them.  vpt_scene_create and vpt_scene_update_volumes both call this, for all
// records of a scene at once (the scene's ball depends on every one), so the two cannot drift apart.
void prep_sdf_records(const vpt_sdf* sdfs, int num_sdfs, const vpt_volume* volumes, const vpt_volume_instance* vol_instances, int num_vol_instances,
    std::vector<float4>& sdf_inv, std::vector<float4>& sdf_fn_rec, std::vector<float4>& sdf_grid_rec, DScene& D) {
  auto rigid = [](const vpt_frame& f) {
    double c[3][3] = {{f.x[0], f.x[1], f.x[2]}, {f.y[0], f.y[1], f.y[2]}, {f.z[0], f.z[1], f.z[2]}};
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        double dp = c[i][0] * c[j][0] + c[i][1] * c[j][1] + c[i][2] * c[j][2];
        if (std::fabs(dp - (i == j ? 1.0 : 0.0)) > 1e-5) return false;
      }
    return true;
  };
  auto identity3 = [](const vpt_frame& f) {
    return f.x[0] == 1 && f.x[1] == 0 && f.x[2] == 0 && f.y[0] == 0 && f.y[1] == 1 && f.y[2] == 0 && f.z[0] == 0 && f.z[1] == 0 && f.z[2] == 1;
  };
  // world position of a local point: the SDFs apply the FORWARD frame to world points (yocto_sdfs.cpp:13), so world = R^T (local - o)
  auto to_world = [](const vpt_frame& f, const double l[3], double w[3]) {
    double v[3] = {l[0] - f.o[0], l[1] - f.o[1], l[2] - f.o[2]};
    w[0] = f.x[0] * v[0] + f.y[0] * v[1] + f.z[0] * v[2];   // rows of R^T = the frame's x, y, z taken component-wise
    w[1] = f.x[1] * v[0] + f.y[1] * v[1] + f.z[1] * v[2];
    w[2] = f.x[2] * v[0] + f.y[2] * v[1] + f.z[2] * v[2];
  };
  struct ball { double c[3], r; };
  std::vector<ball> balls;
  bool all_bounded_rigid = true;
  int  planes = 0;
  sdf_fn_rec.assign(6 * (size_t)num_sdfs, make_float4(0, 0, 0, 0)), sdf_grid_rec.assign(7 * (size_t)num_vol_instances, make_float4(0, 0, 0, 0));
  sdf_inv.resize(3 * (size_t)num_sdfs);
  for (int i = 0; i < num_sdfs; i++) pack_frame(hinverse(to_h(sdfs[i].frame), false), &sdf_inv[3 * (size_t)i]);
  for (int i = 0; i < num_sdfs; i++) {
    const vpt_sdf& f = sdfs[i];
    float4* r = &sdf_fn_rec[6 * (size_t)i];
    pack_frame(to_h(f.frame), r);
    r[3] = make_float4(f.p[0], f.p[1], f.p[2], f.p[3]);
    r[4] = make_float4(f.whd[0] * 0.5f, f.whd[1] * 0.5f, f.whd[2] * 0.5f, 0);
    int tag = f.type | ((identity3(f.frame) ? 1 : 0) << 8);
    memcpy(&r[4].w, &tag, 4);
    double lc[3] = {0, 0, 0}, lr = -1;   // local centre / radius of a ball around the shape
    switch (f.type) {
      case VPT_SDF_BOX: lc[0] = f.whd[0] * 0.5, lc[1] = f.whd[1] * 0.5, lc[2] = f.whd[2] * 0.5, lr = std::sqrt(lc[0] * lc[0] + lc[1] * lc[1] + lc[2] * lc[2]); break;
      case VPT_SDF_BBOX: lr = std::sqrt((double)f.p[1] * f.p[1] + (double)f.p[2] * f.p[2] + (double)f.p[3] * f.p[3]) + 2.0 * std::fabs((double)f.p[0]); break;
      case VPT_SDF_SPHERE: lr = std::fabs((double)f.p[0]); break;
      case VPT_SDF_TORUS: lr = std::fabs((double)f.p[0]) + std::fabs((double)f.p[1]); break;
      case VPT_SDF_CAPPED_CONE: lr = std::sqrt((double)f.p[0] * f.p[0] + std::max((double)f.p[1] * f.p[1], (double)f.p[2] * f.p[2])); break;
      default: break;   // plane: unbounded
    }
    r[5] = make_float4(0, 0, 0, -1);
    if (f.type == VPT_SDF_PLANE) planes++;
    else if (lr > 0 && std::isfinite(lr) && rigid(f.frame)) {
      ball b;
      to_world(f.frame, lc, b.c);
      b.r = lr * 1.05 + 1e-6;
      balls.push_back(b);
      r[5] = make_float4((float)b.c[0], (float)b.c[1], (float)b.c[2], (float)b.r);
    } else all_bounded_rigid = false;
  }
  for (int i = 0; i < num_vol_instances; i++) {
    const vpt_volume_instance& vi = vol_instances[i];
    const vpt_volume&          vol = volumes[vi.volume];
    float4* r = &sdf_grid_rec[7 * (size_t)i];
    pack_frame(to_h(vi.frame), r);
    // bbox_max = origin + (vol.res * grid_res) * scalef; bbox_size = bbox_max - origin   (yocto_sdfs.cpp:33-36, float)
    float size[3];
    for (int k = 0; k < 3; k++) {
      float origin = vi.frame.o[k], grid_res = (float)vol.whd[k];
      float bbox_max = origin + (vol.res * grid_res) * vi.scalef;
      size[k] = bbox_max - origin;
    }
    r[3] = make_float4(size[0], size[1], size[2], vi.scalef);
    r[4] = make_float4(size[0] * 0.5f, size[1] * 0.5f, size[2] * 0.5f, 0);
    int tr = identity3(vi.frame) ? 1 : 0;
    memcpy(&r[4].w, &tr, 4);
    int dims[3] = {vol.whd[0], vol.whd[1], vol.whd[2]};
    memcpy(&r[5], dims, 12);
    r[5].w = vol.res;
    int off[2] = {(int)(vol.offset & 0xffffffffll), (int)(vol.offset >> 32)};
    memcpy(&r[6], off, 8);
    double lc[3] = {size[0] * 0.5, size[1] * 0.5, size[2] * 0.5}, lr = std::sqrt(lc[0] * lc[0] + lc[1] * lc[1] + lc[2] * lc[2]);
    if (lr > 0 && std::isfinite(lr) && rigid(vi.frame)) {
      ball b;
      to_world(vi.frame, lc, b.c);
      b.r = lr * 1.05 + 1e-6;
      balls.push_back(b);
    } else all_bounded_rigid = false;
  }
  D.sdf_bound_cx = D.sdf_bound_cy = D.sdf_bound_cz = 0, D.sdf_bound_r = -1, D.sdf_num_planes = planes;
  if (all_bounded_rigid && !balls.empty()) {
    double c[3] = {0, 0, 0}, rr = 0;
    for (const ball& b : balls)
      for (int k = 0; k < 3; k++) c[k] += b.c[k] / (double)balls.size();
    for (const ball& b : balls) {
      double dist = std::sqrt((b.c[0] - c[0]) * (b.c[0] - c[0]) + (b.c[1] - c[1]) * (b.c[1] - c[1]) + (b.c[2] - c[2]) * (b.c[2] - c[2]));
      rr = std::max(rr, dist + b.r);
    }
    D.sdf_bound_cx = (float)c[0], D.sdf_bound_cy = (float)c[1], D.sdf_bound_cz = (float)c[2], D.sdf_bound_r = (float)(rr * 1.01);
  }
}

void prep_enter_tail(float4* e, const DShape& sh, int scene_quads, int instance, int translation_only) {
  // the quad nodes of all BVHs live in one array, the scene's first: a level is named by the index of its first node
  int tail[6] = {sh.root_ref, scene_quads + sh.wnode_offset, sh.leaf_offset, instance, translation_only, sh.num_nodes};
  memcpy(&e[4].z, &tail[0], 8);
  memcpy(&e[5], &tail[2], 16);
}

// quad nodes of every BVH, the shapes' roots and stack needs, and the traversal stacks sized from them.  The stack sizes and the
// VPT_FLOOR_SHIFT check depend on the trees' topology only: vpt_scene_update refits boxes and keeps topology, so they stay valid;
// vpt_scene_rebuild_bvh (vpt_bvh_rebuild.hip) changes topology and calls this again, on the node arrays it built (vpt_scene_prep.h).
int prep_quad_nodes_and_stacks(const vpt_scene_desc& d, scene_tables& t, bool shapes_kept, const char* shape_made, bool scene_kept) {
  std::vector<float4> shape_wnodes;
  int max_shape_depth = shapes_kept ? t.shape_depth : 0, max_shape_need4 = shapes_kept ? t.shape_need4 : 0;
  long long shape_quads = 0;   // quad nodes of all shapes, the kept ones of a partial call included
  if (!shapes_kept && !shape_made) t.shape_depths.assign((size_t)d.num_shapes, 0), t.shape_need4s.assign((size_t)d.num_shapes, 0), t.shape_quads.assign((size_t)d.num_shapes, 0);
  for (int i = 0; i < d.num_shapes && !shapes_kept; i++) {
    DShape& o = t.shapes[i];
    if (shape_quads > 0x7fffffffLL) return vpt_set_error(VPT_ERR_UNSUPPORTED, "more than 2^27 quad nodes");
    o.wnode_offset = (int)shape_quads;
    if (!shape_made || shape_made[i]) {
      const vpt_shape& sh = d.shapes[i];
      const size_t before = shape_wnodes.size();
      int need4 = 0;
      o.root_ref     = build_quad_nodes(d.shape_bvh_nodes + sh.bvh_node_offset, sh.num_bvh_nodes, shape_wnodes, o.root_box, &need4);
      int depth = o.num_nodes ? bvh_depth(d.shape_bvh_nodes + sh.bvh_node_offset, sh.num_bvh_nodes, 0, 0, 4096) : 0;
      o.stack_need = depth + 2;
      t.shape_depths[(size_t)i] = depth, t.shape_need4s[(size_t)i] = need4, t.shape_quads[(size_t)i] = (int)((shape_wnodes.size() - before) / 8);
    }
    shape_quads += t.shape_quads[(size_t)i];
    if (t.shape_depths[(size_t)i] > max_shape_depth) max_shape_depth = t.shape_depths[(size_t)i];
    if (t.shape_need4s[(size_t)i] > max_shape_need4) max_shape_need4 = t.shape_need4s[(size_t)i];
  }
  DScene& D = t.d;
  if (!scene_kept) {
    t.scene_depth = d.num_scene_bvh_nodes ? bvh_depth(d.scene_bvh_nodes, d.num_scene_bvh_nodes, 0, 0, 4096) : 0;
    float scene_box[6];
    D.scene_root_ref = build_quad_nodes(d.scene_bvh_nodes, d.num_scene_bvh_nodes, t.wnodes, scene_box, &t.scene_need4);
    D.scene_root_lo_x = scene_box[0], D.scene_root_lo_y = scene_box[1], D.scene_root_lo_z = scene_box[2];
    D.scene_root_hi_x = scene_box[3], D.scene_root_hi_y = scene_box[4], D.scene_root_hi_z = scene_box[5];
  }
  const int scene_depth = t.scene_depth, scene_need4 = t.scene_need4;
  // stack entries alive at once: one pending sibling per level (+ the two just pushed), scene level
  // entries stay below the entries of the instance being traversed
  int need = (scene_depth + 2) + (max_shape_depth + 2);
  t.stack_cap = ((need > 8 ? need : 8) + 3) & ~3;
  const int max_stack_cap = 64 * 1024 / (VPT_BLOCK * (int)sizeof(int));   // 256 entries with VPT_BLOCK = 64
  if (t.stack_cap > max_stack_cap)
    return vpt_set_error(VPT_ERR_UNSUPPORTED, "BVH depth %d (scene %d + shapes %d) needs a %d-entry traversal stack; the LDS stack holds %d",
                need, scene_depth, max_shape_depth, t.stack_cap, max_stack_cap);
  // quad-node traversal: worst case = three pending siblings per quad level of the scene BVH plus of the
  // deepest shape BVH, plus one free entry above the top (the branch-free push stores rejected candidates
  // there).  24 entries per lane = 12 KB per wave keep twelve waves on a CU (144 of 160 KB); whatever the
  // worst case needs beyond that lives in HBM (lane_stack2<true>).
  int need4 = scene_need4 + max_shape_need4 + 1;
  // the group form of the node phase (vpt_mesh_kernel.hip.h: group_nodes) hands a ray's pop floor - the stack depth at instance entry, at
  // most scene_need4 - to its helper lanes in the bits above VPT_FLOOR_SHIFT of one word: every stack position has to fit there
  if ((long long)need4 > (0x7fffffffLL >> VPT_FLOOR_SHIFT))
    return vpt_set_error(VPT_ERR_UNSUPPORTED, "quad stack need %d does not fit the traversal's packed pop floor", need4);
  // With the mesh kernel's five parked words per lane (vpt_mesh_kernel.hip.h) a wave takes need4 * 512 + 1280 + 8 bytes of LDS,
  // granted in 1 280-byte steps: up to 22 entries twelve waves fit a CU's 160 KB, with 23 or 24 eleven do - still better than the
  // checked push / pop of the HBM-overflow variant (-7 %), which is for deeper trees only (22 entries in LDS, the rest in HBM).
  t.stack_lds4 = need4 < 8 ? 8 : need4 > 24 ? 22 : need4;
  if (const char* e = getenv("VPT_STACK_LDS")) {   // tuning experiments: force a smaller LDS part (the rest spills to HBM)
    int v = atoi(e);
    if (v >= 4 && v < t.stack_lds4) t.stack_lds4 = v;
  }
  t.stack_spill4 = need4 > t.stack_lds4 ? need4 - t.stack_lds4 : 0;
  if (getenv("VPT_DEBUG"))
    fprintf(stderr, "[vpt] binary depth scene %d shape %d; quad stack need scene %d + shape %d + 1 -> %d in LDS + %d in HBM\n",
        scene_depth, max_shape_depth, scene_need4, max_shape_need4, t.stack_lds4, t.stack_spill4);
  // one table: [scene quad nodes][shape quad nodes]
  if (!scene_kept) t.scene_wnodes = t.wnodes.size();
  if (!shapes_kept) t.shape_wnodes = 8 * (size_t)shape_quads, t.shape_depth = max_shape_depth, t.shape_need4 = max_shape_need4;
  if ((t.scene_wnodes + t.shape_wnodes) / 8 >= (1ull << 27)) return vpt_set_error(VPT_ERR_UNSUPPORTED, "more than 2^27 quad nodes");
  t.wnodes.insert(t.wnodes.end(), shape_wnodes.begin(), shape_wnodes.end());
  return VPT_OK;
}

void prep_quad_slots(const vpt_bvh_node* nodes, int count, std::vector<int>& slots) {
  std::vector<int> order, quad_of;
  quad_order(nodes, count, order, quad_of);
  for (int i : order) {
    int slot[4], axes[3];
    quad_slots_of(nodes, i, slot, axes);
    slots.insert(slots.end(), slot, slot + 4);
  }
}

int prepare_scene(const vpt_scene_desc& d, const vpt_scene_curves* curves, scene_tables& t) {
  const vpt_scene_curves none = {};
  const vpt_scene_curves& cs = curves ? *curves : none;
  if (int rc = validate(d, cs)) return rc;
  DScene& D = t.d;
  D.num_cameras = d.num_cameras, D.num_instances = d.num_instances, D.num_shapes = d.num_shapes;
  D.num_materials = d.num_materials, D.num_textures = d.num_textures, D.num_environments = d.num_environments;
  D.num_volumes = d.num_volumes, D.num_vol_instances = d.num_vol_instances, D.num_sdfs = d.num_sdfs;
  D.num_lights = d.num_lights, D.num_scene_nodes = d.num_scene_bvh_nodes, D.num_scene_prims = d.num_scene_bvh_prims;
  D.group_forms = getenv("VPT_NO_GROUP_FORMS") ? 0 : 1;   // A/B switch of the tests: the two forms of a phase must give the same bits
  build_geometry(d, cs, t);
  if (int rc = prep_quad_nodes_and_stacks(d, t)) return rc;
  build_instances(d, cs, t);
  // sRGB decode LUT: byte_to_float then srgb_to_rgb, yocto_color.h:212-227, evaluated with the host powf
  t.srgb_lut.resize(256);
  for (int b = 0; b < 256; b++) {
    float srgb    = b / 255.0f;
    t.srgb_lut[b] = (srgb <= 0.04045) ? srgb / 12.92f : std::pow((srgb + 0.055f) / (1.0f + 0.055f), 2.4f);
  }
  build_lights(d, t);
  prep_sdf_records(d.sdfs, d.num_sdfs, d.volumes, d.vol_instances, d.num_vol_instances, t.sdf_inv, t.sdf_fn_rec, t.sdf_grid_rec, t.d);
  build_edit_mirrors(d, t);
  t.varying_media = prep_media_vary(d.materials, d.num_materials, t.m.inst_material.data(), t.m.inst_flags.data(), d.num_instances);
  return VPT_OK;
}
