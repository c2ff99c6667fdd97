// vpt_host_capi.cpp — C entry points over the host library for the Python harness
// (tests/, bench.py): load a scene.json, build bvh + lights, hand out the flattened
// vpt_scene_desc, seed a pathtrace_state, quantise/encode output.  Host-only; no GPU calls.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <set>

#include "vpt_host.h"

using namespace vpt;

namespace {
struct host_scene {
  scene_data       scene;
  bvh_scene        bvh;
  pathtrace_lights lights;
  std::unique_ptr<flat_scene> flat = std::make_unique<flat_scene>();
  std::set<int> edited_instances, edited_shapes;   // since the last vpth_scene_update_bvh
  vector<std::unique_ptr<subdiv_plan_host>> plans;   // per subdiv, made when first asked for (vpth_scene_subdiv_plan_item)
};
void set_error(char* err, int errlen, const string& msg) {
  if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", msg.c_str());
}
uint64_t fnv1a(const void* data, size_t nbytes) {
  auto p = (const unsigned char*)data;
  auto h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < nbytes; i++) h = (h ^ p[i]) * 0x100000001b3ull;
  return h;
}
template <typename T>
uint64_t fnv1a(const vector<T>& v) { return fnv1a(v.data(), v.size() * sizeof(T)); }
}  // namespace

extern "C" {

// tess_device >= 0: the vertex arithmetic of tesselate_surfaces on that GPU (tesselate_surfaces_device: same mesh)
void* vpth_scene_load_ex(const char* filename, int tess_device, char* err, int errlen) {
  try {
    auto h     = std::make_unique<host_scene>();
    auto error = string{};
    if (!load_scene(filename, h->scene, error)) return set_error(err, errlen, error), nullptr;
    if (tess_device >= 0) tesselate_surfaces_device(h->scene, tess_device);
    else tesselate_surfaces(h->scene);
    auto params = pathtrace_params{};
    h->bvh      = make_bvh(h->scene, params);
    h->lights   = make_lights(h->scene, params);
    flatten_scene(*h->flat, h->scene, h->bvh, h->lights);
    return h.release();
  } catch (const std::exception& e) {
    return set_error(err, errlen, e.what()), nullptr;
  }
}
void* vpth_scene_load(const char* filename, char* err, int errlen) { return vpth_scene_load_ex(filename, -1, err, errlen); }
// one level of tesselate_catmullclark on a quad mesh with `dim` floats per vertex (host arithmetic, or GPU `device` >= 0 for the
// vertex half): quads_out has room for 4 * nquads entries, verts_out for (nverts + 4 * nquads + nquads) * dim floats (edges <= 4 per face)
int vpth_catmullclark(const int32_t* quads, int nquads, const float* verts, int nverts, int dim, int lock_boundary, int device, int32_t* quads_out,
    int* nquads_out, float* verts_out, int* nverts_out, char* err, int errlen) {
  try {
    auto q = vector<vec4i>((size_t)nquads);
    memcpy((void*)q.data(), quads, (size_t)nquads * 16);
    for (auto& f : q)
      for (auto v : {f.x, f.y, f.z, f.w})
        if (v < 0 || v >= nverts) throw std::invalid_argument{"face index out of range"};
    auto v = vector<float>(verts, verts + (size_t)nverts * dim);
    if (device < 0) tesselate_catmullclark(q, v, dim, lock_boundary != 0);
    else {
      auto L = subdiv_level{};
      catmullclark_topology(q, nverts, lock_boundary != 0, L);
      auto next = vector<float>((size_t)(L.nv + L.ne + L.nf) * dim);
      auto desc = vpt_subdiv_level{dim, L.nv, L.ne, L.nf, (int)L.tquads.size(), L.edges.data(), &L.faces.data()->x, &L.tquads.data()->x,
          L.valence.data(), L.offsets.data(), L.items.data(), (int64_t)L.items.size()};
      if (vpt_subdivide_vertices(device, &desc, v.data(), next.data()) != VPT_OK) throw std::runtime_error{vpt_last_error()};
      v = std::move(next), q = std::move(L.tquads);
    }
    memcpy(quads_out, q.data(), q.size() * 16), memcpy(verts_out, v.data(), v.size() * 4);
    *nquads_out = (int)q.size(), *nverts_out = (int)(v.size() / (size_t)dim);
    return 0;
  } catch (const std::exception& e) {
    return set_error(err, errlen, e.what()), -1;
  }
}
// quads_normals (corners = 4) / triangles_normals (3) over float3 positions: host loops (device < 0) or vpt_vertex_normals on that GPU
int vpth_vertex_normals(const float* positions, int nverts, const int32_t* faces, int nfaces, int corners, int device, float* normals, char* err, int errlen) {
  try {
    if (corners != 3 && corners != 4) throw std::invalid_argument{"corners must be 3 or 4"};
    for (long long i = 0; i < (long long)nfaces * corners; i++)
      if (faces[i] < 0 || faces[i] >= nverts) throw std::invalid_argument{"face index out of range"};
    auto pos = vector<vec3f>((size_t)nverts);
    memcpy((void*)pos.data(), positions, (size_t)nverts * 12);
    auto out = vertex_normals(pos, faces, nfaces, corners, device);
    memcpy(normals, out.data(), (size_t)nverts * 12);
    return 0;
  } catch (const std::exception& e) {
    return set_error(err, errlen, e.what()), -1;
  }
}
// the displacement step of tesselate_surface over float3 positions / normals and float2 texcoords; texels: uchar4 or float4 by is_float
int vpth_displace_vertices(const void* texels, int width, int height, int is_float, int linear, float displacement, const float* positions,
    const float* normals, const float* texcoords, int nverts, int device, float* out_positions, char* err, int errlen) {
  try {
    auto tex = texture_data{};
    tex.width = width, tex.height = height, tex.linear = linear != 0;
    if (is_float) tex.pixelsf.assign((const vec4f*)texels, (const vec4f*)texels + (size_t)width * height);
    else tex.pixelsb.assign((const vec4b*)texels, (const vec4b*)texels + (size_t)width * height);
    auto pos = vector<vec3f>((size_t)nverts), nrm = vector<vec3f>((size_t)nverts);
    auto uv  = vector<vec2f>((size_t)nverts);
    memcpy((void*)pos.data(), positions, (size_t)nverts * 12), memcpy((void*)nrm.data(), normals, (size_t)nverts * 12);
    memcpy((void*)uv.data(), texcoords, (size_t)nverts * 8);
    auto out = displace_vertices(tex, displacement, pos, nrm, uv, device);
    memcpy(out_positions, out.data(), (size_t)nverts * 12);
    return 0;
  } catch (const std::exception& e) {
    return set_error(err, errlen, e.what()), -1;
  }
}
// rebuild the scene's BVHs on GPU `device` (make_bvh_device) and flatten again; 0 on success
// (quality: VPT_BVH_MIDDLE or VPT_BVH_SAH for every tree; another value is refused, the scene untouched)
int vpth_scene_rebuild_bvh_device_quality(void* hh, int device, int quality, char* err, int errlen) {
  try {
    auto& h = *(host_scene*)hh;
    h.bvh   = make_bvh_device(h.scene, pathtrace_params{}, device, quality);
    auto flat = std::make_unique<flat_scene>();
    flatten_scene(*flat, h.scene, h.bvh, h.lights);
    h.flat = std::move(flat);   // the address vpth_scene_desc handed out before is gone: callers fetch it again
    return 0;
  } catch (const std::exception& e) {
    return set_error(err, errlen, e.what()), -1;
  }
}
int vpth_scene_rebuild_bvh_device(void* hh, int device, char* err, int errlen) { return vpth_scene_rebuild_bvh_device_quality(hh, device, VPT_BVH_MIDDLE, err, errlen); }
// build_bvh over n boxes on the host (the checker of vpt_build_bvh_quality in tests): nodes has room for max(1, 2 n) entries; -1 for
// an unknown quality or a bad pointer, nothing written
int vpth_build_bvh_host_quality(const float* bboxes, int n, int quality, vpt_bvh_node* nodes, int* num_nodes, int32_t* primitives) {
  if (n < 0 || !nodes || !num_nodes || (n > 0 && (!bboxes || !primitives))) return -1;
  if (quality != VPT_BVH_MIDDLE && quality != VPT_BVH_SAH) return -1;
  auto bvh = build_bvh_host(bboxes, n, quality);
  memcpy(nodes, bvh.nodes.data(), bvh.nodes.size() * sizeof(vpt_bvh_node));
  if (n > 0) memcpy(primitives, bvh.primitives.data(), (size_t)n * sizeof(int32_t));
  *num_nodes = (int)bvh.nodes.size();
  return 0;
}
int vpth_build_bvh_host(const float* bboxes, int n, vpt_bvh_node* nodes, int* num_nodes, int32_t* primitives) {
  auto bvh = build_bvh_host(bboxes, n);
  memcpy(nodes, bvh.nodes.data(), bvh.nodes.size() * sizeof(vpt_bvh_node));
  if (n > 0) memcpy(primitives, bvh.primitives.data(), (size_t)n * sizeof(int32_t));
  *num_nodes = (int)bvh.nodes.size();
  return 0;
}
// ---- editing a loaded scene (the host side of vpt_scene_update, include/vpt.h) -----------------------------------------------
// kinds of item: 0 camera (vpt_camera), 1 instance frame (vpt_frame), 2 environment frame (vpt_frame), 3 material (vpt_material),
// 4 positions / 5 normals of a shape (float3 per vertex), 6 {shape, material} of an instance (two int32, read only);
// read only, of a shape: 7 texcoords (float2), 8 colors (float4), 9 radius (float), 10 triangles (int3), 11 quads (int4), 12 points (int), 13 lines (int2)
int vpth_scene_count(void* hh, int kind) {
  auto& sc = ((host_scene*)hh)->scene;
  switch (kind) {
    case 0: return (int)sc.cameras.size();
    case 1: return (int)sc.instances.size();
    case 2: return (int)sc.environments.size();
    case 3: return (int)sc.materials.size();
    case 4: case 5: case 7: case 8: case 9: case 10: case 11: case 12: case 13: return (int)sc.shapes.size();
    case 6: return (int)sc.instances.size();
    default: return -1;
  }
}
// copies item `id` to `out` when it fits `capacity` bytes; returns its size in bytes, -1 for a bad kind or id
int64_t vpth_scene_get_item(void* hh, int kind, int id, void* out, int64_t capacity) {
  auto& h = *(host_scene*)hh;
  if (id < 0 || id >= vpth_scene_count(hh, kind)) return -1;
  auto& flat = *h.flat;   // the flattened forms are the ABI's structs
  const void* src = nullptr;
  int64_t     n   = 0;
  switch (kind) {
    case 0: src = &flat.cameras[id], n = sizeof(vpt_camera); break;
    case 1: src = &flat.instances[id].frame, n = sizeof(vpt_frame); break;
    case 2: src = &flat.environments[id].frame, n = sizeof(vpt_frame); break;
    case 3: src = &flat.materials[id], n = sizeof(vpt_material); break;
    case 4: src = h.scene.shapes[id].positions.data(), n = (int64_t)h.scene.shapes[id].positions.size() * 12; break;
    case 5: src = h.scene.shapes[id].normals.data(), n = (int64_t)h.scene.shapes[id].normals.size() * 12; break;
    case 6: src = &flat.instances[id].shape, n = 8; break;
    case 7: src = h.scene.shapes[id].texcoords.data(), n = (int64_t)h.scene.shapes[id].texcoords.size() * 8; break;
    case 8: src = h.scene.shapes[id].colors.data(), n = (int64_t)h.scene.shapes[id].colors.size() * 16; break;
    case 9: src = h.scene.shapes[id].radius.data(), n = (int64_t)h.scene.shapes[id].radius.size() * 4; break;
    case 10: src = h.scene.shapes[id].triangles.data(), n = (int64_t)h.scene.shapes[id].triangles.size() * 12; break;
    case 11: src = h.scene.shapes[id].quads.data(), n = (int64_t)h.scene.shapes[id].quads.size() * 16; break;
    case 12: src = h.scene.shapes[id].points.data(), n = (int64_t)h.scene.shapes[id].points.size() * 4; break;
    case 13: src = h.scene.shapes[id].lines.data(), n = (int64_t)h.scene.shapes[id].lines.size() * 8; break;
  }
  if (out && capacity >= n && n > 0) memcpy(out, src, (size_t)n);
  return n;
}
// Replaces item `id` in the scene containers and in the flattened descriptor; the BVHs follow at vpth_scene_update_bvh.
int vpth_scene_set_item(void* hh, int kind, int id, const void* in, int64_t bytes, char* err, int errlen) {
  auto& h = *(host_scene*)hh;
  if (kind > 5 || id < 0 || id >= vpth_scene_count(hh, kind) || !in) return set_error(err, errlen, "bad item kind, id or pointer"), -1;
  if (bytes != vpth_scene_get_item(hh, kind, id, nullptr, 0)) return set_error(err, errlen, "item size does not match (counts cannot change)"), -1;
  auto frame_of = [](const vpt_frame& f) {
    auto r = frame3f{};
    memcpy((void*)&r, &f, sizeof(f));
    return r;
  };
  switch (kind) {
    case 0: {
      auto& c = h.scene.cameras[id];
      auto& d = *(const vpt_camera*)in;
      c.frame = frame_of(d.frame), c.orthographic = d.orthographic != 0, c.lens = d.lens, c.film = d.film, c.aspect = d.aspect, c.focus = d.focus, c.aperture = d.aperture;
    } break;
    case 1: h.scene.instances[id].frame = frame_of(*(const vpt_frame*)in), h.edited_instances.insert(id); break;
    case 2: h.scene.environments[id].frame = frame_of(*(const vpt_frame*)in); break;
    case 3: {
      auto& m = h.scene.materials[id];
      auto& d = *(const vpt_material*)in;
      if (d.type < 0 || d.type > VPT_MAT_GLTFPBR) return set_error(err, errlen, "bad material type"), -1;
      m.type = (material_type)d.type;
      memcpy((void*)&m.emission, d.emission, 12), memcpy((void*)&m.color, d.color, 12), memcpy((void*)&m.scattering, d.scattering, 12);
      m.roughness = d.roughness, m.metallic = d.metallic, m.ior = d.ior, m.scanisotropy = d.scanisotropy, m.trdepth = d.trdepth, m.opacity = d.opacity;
      m.emission_tex = d.emission_tex, m.color_tex = d.color_tex, m.roughness_tex = d.roughness_tex, m.scattering_tex = d.scattering_tex, m.normal_tex = d.normal_tex;
    } break;
    case 4: memcpy((void*)h.scene.shapes[id].positions.data(), in, (size_t)bytes), h.edited_shapes.insert(id); break;
    case 5: memcpy((void*)h.scene.shapes[id].normals.data(), in, (size_t)bytes); break;
  }
  auto& flat = *h.flat;   // the descriptor's own copy of the item, so that it reads back at once; the BVH arrays wait for update_bvh
  switch (kind) {
    case 0: flat.cameras[id] = *(const vpt_camera*)in; break;
    case 1: flat.instances[id].frame = *(const vpt_frame*)in; break;
    case 2: flat.environments[id].frame = *(const vpt_frame*)in; break;
    case 3: flat.materials[id] = *(const vpt_material*)in; break;
    case 4: memcpy((void*)(flat.positions.data() + flat.shapes[id].position_offset), in, (size_t)bytes); break;
    case 5: memcpy((void*)(flat.normals.data() + flat.shapes[id].normal_offset), in, (size_t)bytes); break;
  }
  return 0;
}
// update_bvh over the instances and shapes edited since the last call, then the flattened descriptor again (its address changes)
int vpth_scene_update_bvh(void* hh, char* err, int errlen) {
  try {
    auto& h = *(host_scene*)hh;
    update_bvh(h.bvh, h.scene, {h.edited_instances.begin(), h.edited_instances.end()}, {h.edited_shapes.begin(), h.edited_shapes.end()});
    h.edited_instances.clear(), h.edited_shapes.clear();
    auto flat = std::make_unique<flat_scene>();
    flatten_scene(*flat, h.scene, h.bvh, h.lights);
    h.flat = std::move(flat);
    return 0;
  } catch (const std::exception& e) {
    return set_error(err, errlen, e.what()), -1;
  }
}
// rebuild_bvh (make_bvh again for the named shapes and, `scene` non-zero or a shape named, for the scene level) on the CURRENT host
// scene, then the flattened descriptor again (its address changes): the host side of vpt_scene_rebuild_bvh
int vpth_scene_rebuild_bvh_quality(void* hh, const int32_t* shape_ids, int n, int scene, int quality, char* err, int errlen);
int vpth_scene_rebuild_bvh(void* hh, const int32_t* shape_ids, int n, int scene, char* err, int errlen) {
  return vpth_scene_rebuild_bvh_quality(hh, shape_ids, n, scene, VPT_BVH_MIDDLE, err, errlen);
}
// (every tree the call builds at `quality`: VPT_BVH_MIDDLE or VPT_BVH_SAH; another value is refused, the scene untouched)
int vpth_scene_rebuild_bvh_quality(void* hh, const int32_t* shape_ids, int n, int scene, int quality, char* err, int errlen) {
  try {
    auto& h = *(host_scene*)hh;
    if (n < 0 || (n > 0 && !shape_ids)) return set_error(err, errlen, "null or negative shape list"), -1;
    rebuild_bvh(h.bvh, h.scene, vector<int>(shape_ids, shape_ids + n), scene != 0, quality);
    for (auto i = 0; i < n; i++) h.edited_shapes.erase(shape_ids[i]);   // their boxes are current
    auto flat = std::make_unique<flat_scene>();
    flatten_scene(*flat, h.scene, h.bvh, h.lights);
    h.flat = std::move(flat);
    return 0;
  } catch (const std::exception& e) {
    return set_error(err, errlen, e.what()), -1;
  }
}
// edit_instances (set on current ids, then remove, then add; the scene BVH built anew, make_lights) and the flattened descriptor again
// (its address changes): the host side of vpt_scene_update_instances.  Refused while a frame or vertex edit waits for update_bvh: its
// ids name the old list.
int vpth_scene_edit_instances(void* hh, const int32_t* remove_ids, int num_remove, const int32_t* set_ids, const vpt_instance* set, int num_set,
    const vpt_instance* add, int num_add, char* err, int errlen) {
  try {
    auto& h = *(host_scene*)hh;
    if (num_remove < 0 || num_set < 0 || num_add < 0 || (num_remove > 0 && !remove_ids) || (num_set > 0 && (!set_ids || !set)) || (num_add > 0 && !add))
      return set_error(err, errlen, "null or negative instance list"), -1;
    if (!h.edited_instances.empty() || !h.edited_shapes.empty()) return set_error(err, errlen, "an edit of frames or vertices is pending: update_bvh first"), -1;
    auto convert = [](const vpt_instance* in, int n) {
      auto out = vector<instance_data>((size_t)n);
      for (auto i = 0; i < n; i++) {
        memcpy((void*)&out[(size_t)i].frame, &in[i].frame, sizeof(vpt_frame));
        out[(size_t)i].shape = in[i].shape, out[(size_t)i].material = in[i].material;
      }
      return out;
    };
    edit_instances(h.scene, h.bvh, h.lights, vector<int>(remove_ids, remove_ids + num_remove), vector<int>(set_ids, set_ids + num_set), convert(set, num_set),
        convert(add, num_add));
    auto flat = std::make_unique<flat_scene>();
    flatten_scene(*flat, h.scene, h.bvh, h.lights);
    h.flat = std::move(flat);
    return 0;
  } catch (const std::exception& e) {
    return set_error(err, errlen, e.what()), -1;
  }
}
// edit_shapes (set on current ids, then remove, then add; make_bvh of the new shapes, the scene BVH when a shape was replaced,
// make_lights) and the flattened descriptor again (its address changes): the host side of vpt_scene_update_shapes.  Refused while a
// frame or vertex edit waits for update_bvh: its ids name the old list.
int vpth_scene_edit_shapes(void* hh, const int32_t* remove_ids, int num_remove, const int32_t* set_ids, const vpt_shape_data* set, int num_set,
    const vpt_shape_data* add, int num_add, char* err, int errlen) {
  try {
    auto& h = *(host_scene*)hh;
    if (num_remove < 0 || num_set < 0 || num_add < 0 || (num_remove > 0 && !remove_ids) || (num_set > 0 && (!set_ids || !set)) || (num_add > 0 && !add))
      return set_error(err, errlen, "null or negative shape list"), -1;
    if (!h.edited_instances.empty() || !h.edited_shapes.empty()) return set_error(err, errlen, "an edit of frames or vertices is pending: update_bvh first"), -1;
    auto convert = [](const vpt_shape_data* in, int n) {
      auto out = vector<shape_data>((size_t)n);
      for (auto i = 0; i < n; i++) {
        auto& s  = in[i];
        auto& o  = out[(size_t)i];
        if (s.num_vertices < 0 || s.num_triangles < 0 || s.num_quads < 0 || s.num_points < 0 || s.num_lines < 0) throw std::invalid_argument{"negative count in a shape"};
        if ((s.num_vertices > 0 && !s.positions) || (s.num_triangles > 0 && !s.triangles) || (s.num_quads > 0 && !s.quads) || (s.num_points > 0 && !s.points) ||
            (s.num_lines > 0 && !s.lines))
          throw std::invalid_argument{"null array with a non-zero count in a shape"};
        auto nv  = (size_t)s.num_vertices;
        auto all = [](const float* p, size_t n) {
          for (size_t k = 0; k < n; k++)
            if (!std::isfinite(p[k])) throw std::invalid_argument{"a value of a shape is not finite"};
        };
        auto fill = [&](auto& to, const float* from, size_t width) {
          if (!from || nv == 0) return;
          all(from, width * nv);
          to.resize(nv);
          memcpy((void*)to.data(), from, 4 * width * nv);
        };
        fill(o.positions, s.positions, 3), fill(o.normals, s.normals, 3), fill(o.texcoords, s.texcoords, 2), fill(o.colors, s.colors, 4);
        if (s.num_points || s.num_lines) fill(o.radius, s.radius, 1);
        o.triangles.resize((size_t)s.num_triangles), o.quads.resize((size_t)s.num_quads), o.points.resize((size_t)s.num_points), o.lines.resize((size_t)s.num_lines);
        if (s.num_triangles) memcpy((void*)o.triangles.data(), s.triangles, 12 * (size_t)s.num_triangles);
        if (s.num_quads) memcpy((void*)o.quads.data(), s.quads, 16 * (size_t)s.num_quads);
        if (s.num_points) memcpy((void*)o.points.data(), s.points, 4 * (size_t)s.num_points);
        if (s.num_lines) memcpy((void*)o.lines.data(), s.lines, 8 * (size_t)s.num_lines);
      }
      return out;
    };
    edit_shapes(h.scene, h.bvh, h.lights, vector<int>(remove_ids, remove_ids + num_remove), vector<int>(set_ids, set_ids + num_set), convert(set, num_set),
        convert(add, num_add));
    auto flat = std::make_unique<flat_scene>();
    flatten_scene(*flat, h.scene, h.bvh, h.lights);
    h.flat = std::move(flat);
    return 0;
  } catch (const std::exception& e) {
    return set_error(err, errlen, e.what()), -1;
  }
}
// make_lights of the scene as the setters left it (an emission switched on or off, an emitter's vertices moved), then the flattened
// descriptor again: the host side of vpt_scene_update_lights.  The BVHs are vpth_scene_update_bvh's business.
int vpth_scene_update_lights(void* hh, char* err, int errlen) {
  try {
    auto& h  = *(host_scene*)hh;
    h.lights = make_lights(h.scene, pathtrace_params{});
    auto flat = std::make_unique<flat_scene>();
    flatten_scene(*flat, h.scene, h.bvh, h.lights);
    h.flat = std::move(flat);
    return 0;
  } catch (const std::exception& e) {
    return set_error(err, errlen, e.what()), -1;
  }
}
// ---- subdivision surfaces (the host side of vpt_scene_attach_subdiv / vpt_scene_update_subdivs, include/vpt.h) ------------------
int vpth_scene_subdiv_count(void* hh) { return (int)((host_scene*)hh)->scene.subdivs.size(); }
// settings: {shape, subdivisions, smooth, catmullclark, displacement_tex}; -1 for a bad id
int vpth_scene_get_subdiv(void* hh, int id, int32_t* settings, float* displacement) {
  auto& sc = ((host_scene*)hh)->scene;
  if (id < 0 || id >= (int)sc.subdivs.size() || !settings || !displacement) return -1;
  auto& s = sc.subdivs[id];
  settings[0] = s.shape, settings[1] = s.subdivisions, settings[2] = s.smooth, settings[3] = s.catmullclark, settings[4] = s.displacement_tex;
  *displacement = s.displacement;
  return 0;
}
// One array of subdiv `id`, copied to `out` when it fits `capacity` bytes; returns its size in bytes, -1 for a bad id or kind.
// The cage: 0 positions (float3), 1 normals (float3), 2 texcoords (float2), 3 quadspos, 4 quadsnorm, 5 quadstexcoord (int4).
// The plan (made by tesselate_subdiv on first use, kept until subdivisions or smooth change): 6 verts (int3 per shape vertex), 7 the
// quads after the last level (int4); of level L = 0 .. subdivisions - 1, kind 16 + 8 L + k: k = 0 sizes {num_vertices, num_edges,
// num_faces, num_new_faces, num_items} (int32), 1 edges, 2 faces, 3 new_faces, 4 valence, 5 offsets, 6 items.
int64_t vpth_scene_subdiv_plan_item(void* hh, int id, int kind, void* out, int64_t capacity) {
  try {
    auto& h = *(host_scene*)hh;
    if (id < 0 || id >= (int)h.scene.subdivs.size() || kind < 0) return -1;
    auto& s = h.scene.subdivs[id];
    if (kind > 5 && s.shape < 0) return -1;   // its shape was removed: there is nothing to plan
    const void* src = nullptr;
    int64_t     n   = 0;
    int32_t     sizes[5];
    auto        of = [&](const auto& v) { src = v.data(), n = (int64_t)(v.size() * sizeof(v[0])); };
    if (kind <= 5) {
      switch (kind) {
        case 0: of(s.positions); break;
        case 1: of(s.normals); break;
        case 2: of(s.texcoords); break;
        case 3: of(s.quadspos); break;
        case 4: of(s.quadsnorm); break;
        case 5: of(s.quadstexcoord); break;
      }
    } else {
      if (h.plans.size() != h.scene.subdivs.size()) h.plans.clear(), h.plans.resize(h.scene.subdivs.size());
      if (!h.plans[id]) {   // into a copy of the shape: asking for the plan changes nothing of the scene
        auto plan = std::make_unique<subdiv_plan_host>();
        auto copy = h.scene.shapes.at((size_t)s.shape);
        tesselate_subdiv(h.scene, id, copy, plan.get());
        h.plans[id] = std::move(plan);
      }
      auto& plan = *h.plans[id];
      if (kind == 6) of(plan.verts);
      else if (kind == 7) of(plan.quads);
      else if (kind >= 16 && (kind - 16) / 8 < (int)plan.levels.size() && (kind - 16) % 8 <= 6) {
        auto& L = plan.levels[(size_t)(kind - 16) / 8];
        switch ((kind - 16) % 8) {
          case 0:
            sizes[0] = L.nv, sizes[1] = L.ne, sizes[2] = L.nf, sizes[3] = (int32_t)L.tquads.size(), sizes[4] = (int32_t)L.items.size();
            src = sizes, n = sizeof(sizes);
            break;
          case 1: of(L.edges); break;
          case 2: of(L.faces); break;
          case 3: of(L.tquads); break;
          case 4: of(L.valence); break;
          case 5: of(L.offsets); break;
          case 6: of(L.items); break;
        }
      } else return -1;
    }
    if (out && capacity >= n && n > 0) memcpy(out, src, (size_t)n);
    return n;
  } catch (const std::exception&) {
    return -1;
  }
}
// The kept cage edited - positions (float3 x the cage's count) unless null, displacement unless NaN, subdivisions / smooth unless < 0 -
// and the mirror's tesselate_surface run on it: the shape holds the new mesh.  *resized: 0 when the shape kept its vertex and triangle
// counts and its pools - the descriptor's copy of positions and normals is current and the shape waits for vpth_scene_update_bvh
// (and _update_lights) like any vertex edit; 1 when it did not: the descriptor and the BVH wait for vpth_scene_edit_shapes with the
// shape's arrays as a `set` entry.  A refused call leaves the scene as it was.
int vpth_scene_set_subdiv(void* hh, int id, const float* positions, float displacement, int subdivisions, int smooth, int* resized, char* err, int errlen) {
  try {
    auto& h = *(host_scene*)hh;
    if (id < 0 || id >= (int)h.scene.subdivs.size() || !resized) return set_error(err, errlen, "subdiv id out of range or null pointer"), -1;
    auto& s = h.scene.subdivs[id];
    if (s.shape < 0) return set_error(err, errlen, "the subdiv's shape was removed"), -1;
    if (positions)
      for (size_t k = 0; k < 3 * s.positions.size(); k++)
        if (!std::isfinite(positions[k])) return set_error(err, errlen, "a cage position is not finite"), -1;
    if (std::isinf(displacement)) return set_error(err, errlen, "the displacement is not finite"), -1;
    if (subdivisions > 10) return set_error(err, errlen, "more than 10 subdivisions"), -1;
    auto was = s;
    if (positions) memcpy((void*)s.positions.data(), positions, 12 * s.positions.size());
    if (!std::isnan(displacement)) s.displacement = displacement;
    if (subdivisions >= 0) s.subdivisions = subdivisions;
    if (smooth >= 0) s.smooth = smooth != 0;
    auto  topology = s.subdivisions != was.subdivisions || s.smooth != was.smooth;
    auto& shape    = h.scene.shapes.at((size_t)s.shape);
    auto  made     = shape;
    try {
      tesselate_subdiv(h.scene, id, made);
    } catch (...) {
      s = was;
      throw;
    }
    *resized = made.positions.size() != shape.positions.size() || made.normals.size() != shape.normals.size() || made.triangles.size() != shape.triangles.size() ||
               made.texcoords.size() != shape.texcoords.size() || topology;
    shape = std::move(made);
    if (topology && h.plans.size() == h.scene.subdivs.size()) h.plans[id] = nullptr;
    if (!*resized) {
      auto& flat = *h.flat;
      memcpy((void*)(flat.positions.data() + flat.shapes[s.shape].position_offset), shape.positions.data(), 12 * shape.positions.size());
      if (!shape.normals.empty()) memcpy((void*)(flat.normals.data() + flat.shapes[s.shape].normal_offset), shape.normals.data(), 12 * shape.normals.size());
      h.edited_shapes.insert(s.shape);
    }
    return 0;
  } catch (const std::exception& e) {
    return set_error(err, errlen, e.what()), -1;
  }
}
// ---- environments and textures (the host side of vpt_scene_update_textures, include/vpt.h) ------------------------------------
int vpth_scene_get_environment(void* hh, int id, vpt_environment* out) {
  auto& sc = ((host_scene*)hh)->scene;
  if (id < 0 || id >= (int)sc.environments.size() || !out) return -1;
  auto& e = sc.environments[id];
  memcpy(&out->frame, &e.frame, sizeof(vpt_frame)), memcpy(out->emission, &e.emission, 12);
  out->emission_tex = e.emission_tex;
  return 0;
}
// frame, emission and emission_tex of an environment; desc and stats() follow at vpth_scene_update_textures
int vpth_scene_set_environment(void* hh, int id, const vpt_environment* in, char* err, int errlen) {
  auto& sc = ((host_scene*)hh)->scene;
  if (id < 0 || id >= (int)sc.environments.size() || !in) return set_error(err, errlen, "environment id out of range or null pointer"), -1;
  auto frame = (const float*)&in->frame;
  for (auto k = 0; k < 12; k++)
    if (!std::isfinite(frame[k])) return set_error(err, errlen, "a frame value is not finite"), -1;
  for (auto v : in->emission)
    if (!std::isfinite(v)) return set_error(err, errlen, "an emission value is not finite"), -1;
  if (in->emission_tex < -1 || in->emission_tex >= (int)sc.textures.size()) return set_error(err, errlen, "emission_tex is neither -1 nor a texture"), -1;
  // an emissive environment's texture holds texels: vpt_scene_create and vpt_scene_update_textures refuse the scene otherwise
  auto lit = !(in->emission[0] == 0 && in->emission[1] == 0 && in->emission[2] == 0);
  if (lit && in->emission_tex >= 0 && (int64_t)sc.textures[in->emission_tex].width * sc.textures[in->emission_tex].height == 0)
    return set_error(err, errlen, "the emission texture of an emissive environment has no texels"), -1;
  auto& e = sc.environments[id];
  memcpy((void*)&e.frame, &in->frame, sizeof(vpt_frame)), memcpy((void*)&e.emission, in->emission, 12);
  e.emission_tex = in->emission_tex;
  return 0;
}
// width, height, linear, is_float of a texture, and its texels (float4 or uchar4) when they fit `capacity` bytes
int vpth_scene_get_texture(void* hh, int id, int* width, int* height, int* linear, int* is_float, void* texels, int64_t capacity) {
  auto& sc = ((host_scene*)hh)->scene;
  if (id < 0 || id >= (int)sc.textures.size()) return -1;
  auto& t = sc.textures[id];
  *width = t.width, *height = t.height, *linear = t.linear, *is_float = !t.pixelsf.empty();
  auto bytes = (int64_t)(*is_float ? t.pixelsf.size() * 16 : t.pixelsb.size() * 4);
  if (texels && capacity >= bytes && bytes > 0) memcpy(texels, *is_float ? (const void*)t.pixelsf.data() : (const void*)t.pixelsb.data(), (size_t)bytes);
  return 0;
}
// all texels of a texture replaced (any size, either format); desc and stats() follow at vpth_scene_update_textures
int vpth_scene_set_texture(void* hh, int id, int width, int height, int linear, int is_float, const void* texels, char* err, int errlen) {
  auto& sc = ((host_scene*)hh)->scene;
  if (id < 0 || id >= (int)sc.textures.size()) return set_error(err, errlen, "texture id out of range"), -1;
  if (width < 0 || height < 0 || (int64_t)width * height >= (1ll << 31)) return set_error(err, errlen, "bad texture size"), -1;
  auto n = (size_t)width * (size_t)height;
  if (n > 0 && !texels) return set_error(err, errlen, "null texels"), -1;
  if (is_float && n == 0) return set_error(err, errlen, "a float texture needs at least one texel (an empty one reads as bytes)"), -1;
  for (auto& e : sc.environments)
    if (n == 0 && e.emission_tex == id && !(e.emission.x == 0 && e.emission.y == 0 && e.emission.z == 0))
      return set_error(err, errlen, "an emissive environment names this texture: it needs at least one texel"), -1;
  auto& t = sc.textures[id];
  t.width = width, t.height = height, t.linear = linear != 0;
  t.pixelsf.clear(), t.pixelsb.clear();
  if (is_float) t.pixelsf.assign((const vec4f*)texels, (const vec4f*)texels + n);
  else t.pixelsb.assign((const vec4b*)texels, (const vec4b*)texels + n);
  return 0;
}
// make_lights of the scene as the setters above left it, then the flattened descriptor again (its address changes)
int vpth_scene_update_textures(void* hh, char* err, int errlen) { return vpth_scene_update_lights(hh, err, errlen); }
// ---- volumes, grid instances and SDFs (the host side of vpt_scene_update_volumes, include/vpt.h) ------------------------------
// kind: 0 volumes, 1 volume instances, 2 SDFs
int vpth_scene_count_implicit(void* hh, int kind) {
  auto& sc = ((host_scene*)hh)->scene;
  return kind == 0 ? (int)sc.volumes.size() : kind == 1 ? (int)sc.vol_instances.size() : kind == 2 ? (int)sc.sdfs.size() : -1;
}
int vpth_scene_get_vol_instance(void* hh, int id, vpt_volume_instance* out) {
  auto& sc = ((host_scene*)hh)->scene;
  if (id < 0 || id >= (int)sc.vol_instances.size() || !out) return -1;
  auto& i = sc.vol_instances[id];
  memcpy(&out->frame, &i.frame, sizeof(vpt_frame));
  out->volume = i.volume, out->material = i.material, out->scalef = i.scalef;
  return 0;
}
// frame, volume, material and scalef of a grid instance; desc and stats() follow at vpth_scene_update_volumes
int vpth_scene_set_vol_instance(void* hh, int id, const vpt_volume_instance* in, char* err, int errlen) {
  auto& sc = ((host_scene*)hh)->scene;
  if (id < 0 || id >= (int)sc.vol_instances.size() || !in) return set_error(err, errlen, "volume instance id out of range or null pointer"), -1;
  auto frame = (const float*)&in->frame;
  for (auto k = 0; k < 12; k++)
    if (!std::isfinite(frame[k])) return set_error(err, errlen, "a frame value is not finite"), -1;
  if (!std::isfinite(in->scalef)) return set_error(err, errlen, "scalef is not finite"), -1;
  if (in->volume < 0 || in->volume >= (int)sc.volumes.size()) return set_error(err, errlen, "volume id out of range"), -1;
  if (in->material < 0 || in->material >= (int)sc.materials.size()) return set_error(err, errlen, "material id out of range"), -1;
  auto& i = sc.vol_instances[id];
  memcpy((void*)&i.frame, &in->frame, sizeof(vpt_frame));
  i.volume = in->volume, i.material = in->material, i.scalef = in->scalef;
  return 0;
}
int vpth_scene_get_sdf(void* hh, int id, vpt_sdf* out) {
  auto& sc = ((host_scene*)hh)->scene;
  if (id < 0 || id >= (int)sc.sdfs.size() || !out) return -1;
  auto& s = sc.sdfs[id];
  memcpy(&out->frame, &s.frame, sizeof(vpt_frame));
  out->type = (int)s.type, out->material = s.material;
  memcpy(out->whd, &s.whd, 12), memcpy(out->p, s.p, 16);
  return 0;
}
// the whole SDF, type included
int vpth_scene_set_sdf(void* hh, int id, const vpt_sdf* in, char* err, int errlen) {
  auto& sc = ((host_scene*)hh)->scene;
  if (id < 0 || id >= (int)sc.sdfs.size() || !in) return set_error(err, errlen, "sdf id out of range or null pointer"), -1;
  auto frame = (const float*)&in->frame;
  for (auto k = 0; k < 12; k++)
    if (!std::isfinite(frame[k])) return set_error(err, errlen, "a frame value is not finite"), -1;
  for (auto k = 0; k < 3; k++)
    if (!std::isfinite(in->whd[k])) return set_error(err, errlen, "a whd value is not finite"), -1;
  for (auto k = 0; k < 4; k++)
    if (!std::isfinite(in->p[k])) return set_error(err, errlen, "a parameter is not finite"), -1;
  if (in->type < 0 || in->type > VPT_SDF_TORUS) return set_error(err, errlen, "sdf type is not one of 0..5"), -1;
  if (in->material < 0 || in->material >= (int)sc.materials.size()) return set_error(err, errlen, "material id out of range"), -1;
  auto& s = sc.sdfs[id];
  memcpy((void*)&s.frame, &in->frame, sizeof(vpt_frame));
  s.type = (sdf_type)in->type, s.material = in->material;
  memcpy((void*)&s.whd, in->whd, 12), memcpy(s.p, in->p, 16);
  return 0;
}
// The box region_lo .. region_lo + region_whd of volume `id` written from `voxels` (region order, x fastest), whd and res the volume's
// AFTER the call: the same whd writes in place, a new one needs the whole grid and mode 0.  mode 1: op_union(resident, incoming) =
// (a < b) ? a : b, the select (yocto_sdfs.h:82).  The rules of vpt_scene_update_volumes.
int vpth_scene_set_volume(void* hh, int id, const int32_t* whd, float res, const int32_t* lo, const int32_t* size, int mode, const float* voxels, char* err,
    int errlen) {
  auto& sc = ((host_scene*)hh)->scene;
  if (id < 0 || id >= (int)sc.volumes.size() || !whd || !lo || !size) return set_error(err, errlen, "volume id out of range or null pointer"), -1;
  if (!std::isfinite(res)) return set_error(err, errlen, "res is not finite"), -1;
  if (whd[0] < 0 || whd[1] < 0 || whd[2] < 0) return set_error(err, errlen, "bad volume size"), -1;
  if (whd[0] > 0 && whd[1] > 0 && whd[2] > 0) {   // a product below 2^31, factor by factor: no partial product can overflow
    auto count = (int64_t)1;
    for (auto k = 0; k < 3; k++)
      if ((count *= whd[k]) >= (1ll << 31)) return set_error(err, errlen, "bad volume size: 2^31 voxels or more"), -1;
  }
  for (auto k = 0; k < 3; k++)
    if (lo[k] < 0 || size[k] < 0 || (int64_t)lo[k] + size[k] > whd[k]) return set_error(err, errlen, "the region leaves the grid"), -1;
  if (mode != VPT_VOXELS_REPLACE && mode != VPT_VOXELS_UNION) return set_error(err, errlen, "mode is neither REPLACE nor UNION"), -1;
  auto& v = sc.volumes[id];
  auto  n = (size_t)size[0] * (size_t)size[1] * (size_t)size[2];
  if (n > 0 && !voxels) return set_error(err, errlen, "null voxels"), -1;
  if (whd[0] != v.whd.x || whd[1] != v.whd.y || whd[2] != v.whd.z) {
    if (size[0] != whd[0] || size[1] != whd[1] || size[2] != whd[2] || mode != VPT_VOXELS_REPLACE)
      return set_error(err, errlen, "a new whd needs the whole grid as its region, in REPLACE mode"), -1;
    v.whd = {whd[0], whd[1], whd[2]};
    v.vol.assign((size_t)whd[0] * (size_t)whd[1] * (size_t)whd[2], 0.0f);
  }
  v.res = res;
  for (auto z = 0; z < size[2]; z++)
    for (auto y = 0; y < size[1]; y++)
      for (auto x = 0; x < size[0]; x++) {
        auto& a = v.vol[(size_t)(lo[0] + x) + (size_t)(lo[1] + y) * (size_t)whd[0] + (size_t)(lo[2] + z) * (size_t)whd[0] * (size_t)whd[1]];
        auto  b = voxels[(size_t)x + (size_t)y * (size_t)size[0] + (size_t)z * (size_t)size[0] * (size_t)size[1]];
        a = mode == VPT_VOXELS_UNION ? ((a < b) ? a : b) : b;
      }
  return 0;
}
// One entry of a vpt_sculpt_edit applied to the scene's copy of volume entry->volume by the host mirror (host/vpt_sculpt.cpp), its stamps
// taken from `stamps` (the edit's list of `num_stamps`).  The rules of vpt_scene_sculpt_volumes; a refused call writes nothing.
int vpth_scene_sculpt_volume(void* hh, const vpt_sculpt_entry* entry, const vpt_sculpt_stamp* stamps, int num_stamps, char* err, int errlen) {
  auto& sc = ((host_scene*)hh)->scene;
  if (!entry) return set_error(err, errlen, "sculpt: null entry"), -1;
  if (entry->volume < 0 || entry->volume >= (int)sc.volumes.size())
    return set_error(err, errlen, "sculpt: entry 0: volume " + std::to_string(entry->volume) + " out of range (" + std::to_string(sc.volumes.size()) + ")"), -1;
  auto error = string{};
  if (!sculpt_volume(sc.volumes[entry->volume], *entry, stamps, num_stamps, error)) return set_error(err, errlen, error), -1;
  return 0;
}
// make_lights of the scene as the setters above left it (an SDF is a light iff its material is emissive), then the flattened descriptor again
int vpth_scene_update_volumes(void* hh, char* err, int errlen) { return vpth_scene_update_lights(hh, err, errlen); }
// The host side of vpt_scene_update_volume_set (include/vpt.h) under its rules: the removed entries of the three lists erased (current
// ids; survivors keep their order, ids close up, a surviving grid instance's volume id follows), then the added ones appended - an added
// instance names a volume of the new list - then make_lights and the flattened descriptor again (its address changes).  A FROM_BAKE
// volume gets zeros here: the caller writes the host mirror of the bake through vpth_scene_set_volume when the copy is read.  A refused
// call changes nothing.
int vpth_scene_edit_volume_set(void* hh, const vpt_volume_set_edit* e, char* err, int errlen) {
  try {
    auto& h  = *(host_scene*)hh;
    auto& sc = h.scene;
    if (!e) return set_error(err, errlen, "volume_set: null edit"), -1;
    auto keep_of = [&](const char* what, int n, const int32_t* ids, size_t limit, vector<char>& keep) {
      keep.assign(limit, 1);
      if (n < 0 || (n > 0 && !ids)) throw std::invalid_argument{string{"volume_set: "} + what + " list is null or has a negative count"};
      for (auto i = 0; i < n; i++) {
        if (ids[i] < 0 || (size_t)ids[i] >= limit) throw std::invalid_argument{string{"volume_set: "} + what + " id " + std::to_string(ids[i]) + " out of range"};
        if (!keep[(size_t)ids[i]]) throw std::invalid_argument{string{"volume_set: "} + what + " id " + std::to_string(ids[i]) + " repeated"};
        keep[(size_t)ids[i]] = 0;
      }
    };
    auto keep_inst = vector<char>{}, keep_sdf = vector<char>{}, keep_vol = vector<char>{};
    keep_of("remove_vol_instance", e->num_remove_vol_instances, e->remove_vol_instance_ids, sc.vol_instances.size(), keep_inst);
    keep_of("remove_sdf", e->num_remove_sdfs, e->remove_sdf_ids, sc.sdfs.size(), keep_sdf);
    keep_of("remove_volume", e->num_remove_volumes, e->remove_volume_ids, sc.volumes.size(), keep_vol);
    if (e->num_add_volumes < 0 || e->num_add_vol_instances < 0 || e->num_add_sdfs < 0 || e->num_voxels < 0 || (e->num_add_volumes > 0 && !e->add_volumes) ||
        (e->num_add_vol_instances > 0 && !e->add_vol_instances) || (e->num_add_sdfs > 0 && !e->add_sdfs) || (e->num_voxels > 0 && !e->voxels))
      return set_error(err, errlen, "volume_set: a list of additions is null or has a negative count"), -1;
    auto new_volume = vector<int>(sc.volumes.size(), -1);
    auto volumes    = vector<volume_data>{};
    for (size_t i = 0; i < sc.volumes.size(); i++)
      if (keep_vol[i]) new_volume[i] = (int)volumes.size(), volumes.push_back(sc.volumes[i]);
    for (auto i = 0; i < e->num_add_volumes; i++) {
      auto& n    = e->add_volumes[i];
      auto  name = "volume_set: add_volume entry " + std::to_string(i);
      if (!std::isfinite(n.res)) return set_error(err, errlen, name + ": res is not finite"), -1;
      if (n.whd[0] < 0 || n.whd[1] < 0 || n.whd[2] < 0) return set_error(err, errlen, name + ": negative whd"), -1;
      auto count = (int64_t)1;
      for (auto k = 0; k < 3; k++) {
        count *= n.whd[k];
        if (count >= (1ll << 31)) return set_error(err, errlen, name + ": 2^31 voxels or more"), -1;
      }
      if (n.whd[0] == 0 || n.whd[1] == 0 || n.whd[2] == 0) count = 0;
      auto& v = volumes.emplace_back();
      v.whd = {n.whd[0], n.whd[1], n.whd[2]}, v.res = n.res;
      if (n.source == VPT_VOLUME_FROM_HOST) {
        if (n.offset < 0 || n.offset > e->num_voxels - count) return set_error(err, errlen, name + ": voxels out of range of the edit's payload"), -1;
        v.vol.assign(e->voxels + n.offset, e->voxels + n.offset + count);
      } else if (n.source == VPT_VOLUME_FROM_BAKE) {
        v.vol.assign((size_t)count, 0.0f);
      } else if (n.source == VPT_VOLUME_FILL) {
        v.vol.assign((size_t)count, 0.0f);
        for (auto& x : v.vol) memcpy(&x, &n.fill, 4);   // the bits, a NaN's payload included
      } else if (n.source == VPT_VOLUME_COPY) {
        if (n.copy_of < 0 || (size_t)n.copy_of >= sc.volumes.size()) return set_error(err, errlen, name + ": copy_of out of range"), -1;
        auto& from = sc.volumes[(size_t)n.copy_of];
        if (from.whd.x != n.whd[0] || from.whd.y != n.whd[1] || from.whd.z != n.whd[2]) return set_error(err, errlen, name + ": whd differs from its source's"), -1;
        v.vol = from.vol;
      } else
        return set_error(err, errlen, name + ": source is not one of 0..3"), -1;
    }
    auto finite = [](const float* p, int n) {
      for (auto k = 0; k < n; k++)
        if (!std::isfinite(p[k])) return false;
      return true;
    };
    auto instances = vector<volume_instance>{};
    for (size_t i = 0; i < sc.vol_instances.size(); i++) {
      if (!keep_inst[i]) continue;
      auto inst = sc.vol_instances[i];
      if (new_volume[(size_t)inst.volume] < 0)
        return set_error(err, errlen, "volume_set: remove_volume: volume " + std::to_string(inst.volume) + " is still named by vol_instance " + std::to_string(i)), -1;
      inst.volume = new_volume[(size_t)inst.volume];
      instances.push_back(inst);
    }
    for (auto i = 0; i < e->num_add_vol_instances; i++) {
      auto& in   = e->add_vol_instances[i];
      auto  name = "volume_set: add_vol_instance entry " + std::to_string(i);
      if (!finite((const float*)&in.frame, 12) || !std::isfinite(in.scalef)) return set_error(err, errlen, name + ": a value is not finite"), -1;
      if (in.volume < 0 || (size_t)in.volume >= volumes.size()) return set_error(err, errlen, name + ": volume out of range"), -1;
      if (in.material < 0 || (size_t)in.material >= sc.materials.size()) return set_error(err, errlen, name + ": material out of range"), -1;
      auto& o = instances.emplace_back();
      memcpy((void*)&o.frame, &in.frame, sizeof(vpt_frame));
      o.volume = in.volume, o.material = in.material, o.scalef = in.scalef;
    }
    auto sdfs = vector<sdf_data>{};
    for (size_t i = 0; i < sc.sdfs.size(); i++)
      if (keep_sdf[i]) sdfs.push_back(sc.sdfs[i]);
    for (auto i = 0; i < e->num_add_sdfs; i++) {
      auto& in   = e->add_sdfs[i];
      auto  name = "volume_set: add_sdf entry " + std::to_string(i);
      if (!finite((const float*)&in.frame, 12) || !finite(in.whd, 3) || !finite(in.p, 4)) return set_error(err, errlen, name + ": a value is not finite"), -1;
      if (in.type < 0 || in.type > VPT_SDF_TORUS) return set_error(err, errlen, name + ": type is not one of 0..5"), -1;
      if (in.material < 0 || (size_t)in.material >= sc.materials.size()) return set_error(err, errlen, name + ": material out of range"), -1;
      auto& s = sdfs.emplace_back();
      memcpy((void*)&s.frame, &in.frame, sizeof(vpt_frame));
      s.type = (sdf_type)in.type, s.material = in.material;
      memcpy((void*)&s.whd, in.whd, 12), memcpy(s.p, in.p, 16);
    }
    sc.volumes = std::move(volumes), sc.vol_instances = std::move(instances), sc.sdfs = std::move(sdfs);
    return vpth_scene_update_lights(hh, err, errlen);
  } catch (const std::exception& ex) {
    return set_error(err, errlen, ex.what()), -1;
  }
}
void vpth_scene_free(void* h) { delete (host_scene*)h; }
const vpt_scene_desc* vpth_scene_desc(void* h) { return &((host_scene*)h)->flat->desc; }
const vpt_scene_curves* vpth_scene_curves(void* h) { return ((host_scene*)h)->flat->curves_or_null(); }   // null: no points or lines

// make_state dimensions (yocto_pathtrace.cpp:964-970)
int vpth_state_size(void* h, int camera, int resolution, int* width, int* height) {
  auto& scene = ((host_scene*)h)->scene;
  if (camera < 0 || camera >= (int)scene.cameras.size()) return -1;
  auto aspect       = scene.cameras[camera].aspect;
  if (aspect >= 1) *width = resolution, *height = (int)std::round(resolution / aspect);
  else *height = resolution, *width = (int)std::round(resolution * aspect);
  return 0;
}
// fills caller arrays of w*h entries: image float4 zeros, hits zeros, rng {state, inc}
int vpth_make_state(void* h, int camera, int resolution, float* image, int32_t* hits, uint64_t* rng) {
  try {
    auto params       = pathtrace_params{};
  (void)params;
    params.camera     = camera;
    params.resolution = resolution;
    auto state        = make_state(((host_scene*)h)->scene, params);
    auto n            = state.image.size();
    memset(image, 0, n * 16), memset(hits, 0, n * 4);
    memcpy(rng, state.rngs.data(), n * 16);
    return 0;
  } catch (...) {
    return -1;
  }
}

// same JSON shape as oracle/ref_driver.cpp --stats, so tests can diff the two verbatim
int vpth_scene_stats(void* hh, char* buf, int buflen) {
  auto& h = *(host_scene*)hh;
  auto  s = string{};
  char  tmp[1024];
  auto  add = [&](const char* fmt, auto... args) {
    if constexpr (sizeof...(args) == 0) s += fmt;
    else {
      snprintf(tmp, sizeof(tmp), fmt, args...);
      s += tmp;
    }
  };
  add("{\n \"scene_bvh\": {\"nodes\": %zu, \"prims\": %zu, \"nodes_fnv\": \"%016llx\", \"prims_fnv\": \"%016llx\"},\n",
      h.bvh.nodes.size(), h.bvh.primitives.size(), (unsigned long long)fnv1a(h.bvh.nodes),
      (unsigned long long)fnv1a(h.bvh.primitives));
  add(" \"shapes\": [\n");
  for (size_t i = 0; i < h.scene.shapes.size(); i++) {
    auto& sh = h.scene.shapes[i];
    auto& b  = h.bvh.shapes[i];
    add("  {\"positions\": %zu, \"normals\": %zu, \"texcoords\": %zu, \"colors\": %zu, "
        "\"triangles\": %zu, \"quads\": %zu, \"pos_fnv\": \"%016llx\", \"nrm_fnv\": \"%016llx\", "
        "\"uv_fnv\": \"%016llx\", \"tri_fnv\": \"%016llx\", \"quad_fnv\": \"%016llx\", "
        "\"bvh_nodes\": %zu, \"bvh_nodes_fnv\": \"%016llx\", \"bvh_prims_fnv\": \"%016llx\"}%s\n",
        sh.positions.size(), sh.normals.size(), sh.texcoords.size(), sh.colors.size(), sh.triangles.size(),
        sh.quads.size(), (unsigned long long)fnv1a(sh.positions), (unsigned long long)fnv1a(sh.normals),
        (unsigned long long)fnv1a(sh.texcoords), (unsigned long long)fnv1a(sh.triangles),
        (unsigned long long)fnv1a(sh.quads), b.nodes.size(), (unsigned long long)fnv1a(b.nodes),
        (unsigned long long)fnv1a(b.primitives), "");
    // shapes of points or lines only: the lines of a scene of faces stay those of oracle/ref_driver.cpp --stats
    if (!sh.points.empty() || !sh.lines.empty() || !sh.radius.empty()) {
      s.erase(s.size() - 2);   // "}\n"
      add(", \"points\": %zu, \"lines\": %zu, \"radius\": %zu, \"points_fnv\": \"%016llx\", \"lines_fnv\": \"%016llx\", \"radius_fnv\": \"%016llx\"}\n",
          sh.points.size(), sh.lines.size(), sh.radius.size(), (unsigned long long)fnv1a(sh.points), (unsigned long long)fnv1a(sh.lines),
          (unsigned long long)fnv1a(sh.radius));
    }
    if (i + 1 < h.scene.shapes.size()) s.insert(s.size() - 1, ",");
  }
  add(" ],\n \"textures\": [\n");
  for (size_t i = 0; i < h.scene.textures.size(); i++) {
    auto& t = h.scene.textures[i];
    add("  {\"width\": %d, \"height\": %d, \"linear\": %d, \"f_fnv\": \"%016llx\", \"b_fnv\": \"%016llx\"}%s\n",
        t.width, t.height, (int)t.linear, (unsigned long long)fnv1a(t.pixelsf),
        (unsigned long long)fnv1a(t.pixelsb), i + 1 < h.scene.textures.size() ? "," : "");
  }
  add(" ],\n \"volumes\": [\n");
  for (size_t i = 0; i < h.scene.volumes.size(); i++) {
    auto& v = h.scene.volumes[i];
    add("  {\"whd\": [%d, %d, %d], \"res\": %.9g, \"n\": %zu, \"fnv\": \"%016llx\"}%s\n", v.whd.x, v.whd.y,
        v.whd.z, v.res, v.vol.size(), (unsigned long long)fnv1a(v.vol),
        i + 1 < h.scene.volumes.size() ? "," : "");
  }
  add(" ],\n \"lights\": [\n");
  for (size_t i = 0; i < h.lights.lights.size(); i++) {
    auto& l = h.lights.lights[i];
    add("  {\"instance\": %d, \"environment\": %d, \"sdf\": %d, \"cdf_len\": %zu, \"cdf_back\": %.9g, \"cdf_fnv\": \"%016llx\"}%s\n",
        l.instance, l.environment, l.sdf, l.elements_cdf.size(),
        l.elements_cdf.empty() ? 0.0f : l.elements_cdf.back(), (unsigned long long)fnv1a(l.elements_cdf),
        i + 1 < h.lights.lights.size() ? "," : "");
  }
  add(" ]\n}\n");
  if ((int)s.size() + 1 > buflen) return -(int)s.size() - 1;
  memcpy(buf, s.c_str(), s.size() + 1);
  return (int)s.size();
}

// output stage: linear float4 sums / samples -> sRGB8 (w*h*4 bytes)
void vpth_linear_to_srgb8(int width, int height, const float* image_sum, int samples, uint8_t* rgba8) {
  auto img   = color_image{width, height, true, {}};
  auto scale = 1.0f / (float)samples;
  img.pixels.resize((size_t)width * height);
  for (size_t i = 0; i < img.pixels.size(); i++)
    img.pixels[i] = {image_sum[4 * i] * scale, image_sum[4 * i + 1] * scale, image_sum[4 * i + 2] * scale,
        image_sum[4 * i + 3] * scale};
  auto ldr = linear_to_srgb8(img);
  memcpy(rgba8, ldr.data(), ldr.size() * 4);
}
// denoise_render on row-major float4 images (normal / albedo / variance nullable): the host mirror (device < 0) or vpt_denoise on that GPU
int vpth_denoise(int width, int height, const float* color, const float* normal, const float* albedo, const float* variance, int iterations,
    float sigma_luminance, float sigma_normal, float sigma_albedo, int device, float* out, char* err, int errlen) {
  try {
    if (width < 1 || height < 1 || !color || !out) throw std::invalid_argument{"bad image"};
    auto n     = (size_t)width * height;
    auto image = [&](const float* p) {
      auto img = color_image{p ? width : 0, p ? height : 0, true, {}};
      if (p) img.pixels.assign((const vec4f*)p, (const vec4f*)p + n);
      return img;
    };
    auto var = variance ? vector<float>(variance, variance + n) : vector<float>{};
    auto res = color_image{};
    auto par = denoise_params{iterations, sigma_luminance, sigma_normal, sigma_albedo};
    if (device < 0) denoise_render(res, image(color), image(albedo), image(normal), var, par);
    else denoise_render_device(res, image(color), image(albedo), image(normal), var, par, device);
    memcpy(out, res.pixels.data(), n * 16);
    return 0;
  } catch (const std::exception& e) {
    return set_error(err, errlen, e.what()), -1;
  }
}
// half_variance on two row-major float4 sum images: host loops (device < 0) or vpt_half_variance on that GPU
int vpth_half_variance(int width, int height, const float* sum_a, int a, const float* sum_n, int n, int device, float* variance, char* err, int errlen) {
  try {
    if (width < 1 || height < 1 || !sum_a || !sum_n || !variance) throw std::invalid_argument{"bad image"};
    auto px  = (size_t)width * height;
    auto out = half_variance(width, height, vector<vec4f>((const vec4f*)sum_a, (const vec4f*)sum_a + px), a,
        vector<vec4f>((const vec4f*)sum_n, (const vec4f*)sum_n + px), n, device);
    memcpy(variance, out.data(), px * 4);
    return 0;
  } catch (const std::exception& e) {
    return set_error(err, errlen, e.what()), -1;
  }
}
// tonemap_image on a row-major float4 image of n pixels: floats to display_f and / or bytes to rgba8 (either may be null)
int vpth_tonemap(int64_t n, const float* linear, float exposure, int filmic, int srgb, float* display_f, uint8_t* rgba8) {
  if (n < 0 || !linear || (!display_f && !rgba8)) return -1;
  auto hdr = vector<vec4f>((const vec4f*)linear, (const vec4f*)linear + n);
  if (display_f) {
    auto ldr = vector<vec4f>{};
    tonemap_image(ldr, hdr, exposure, filmic != 0, srgb != 0);
    memcpy(display_f, ldr.data(), (size_t)n * 16);
  }
  if (rgba8) {
    auto ldr = vector<vec4b>{};
    tonemap_image(ldr, hdr, exposure, filmic != 0, srgb != 0);
    memcpy(rgba8, ldr.data(), (size_t)n * 4);
  }
  return 0;
}
// the preview (pw x ph float4) replicated into out (width x height float4)
int vpth_upscale_preview(int pratio, int pw, int ph, const float* preview, int width, int height, float* out) {
  try {
    if (pw < 1 || ph < 1 || !preview || !out) return -1;
    auto src = color_image{pw, ph, true, {}};
    src.pixels.assign((const vec4f*)preview, (const vec4f*)preview + (size_t)pw * ph);
    auto dst = color_image{};
    upscale_preview(dst, src, pratio, width, height);
    memcpy(out, dst.pixels.data(), dst.pixels.size() * 16);
    return 0;
  } catch (...) {
    return -1;
  }
}
// make_state's rngs {state, inc} of a width x height frame by jumps of the master stream (csrc/vpt_rng_jump.h)
int vpth_make_state_jump(int width, int height, uint64_t* rng) {
  try {
    if (!rng) return -1;
    auto rngs = make_state_rngs_jump(width, height);
    memcpy(rng, rngs.data(), rngs.size() * 16);
    return 0;
  } catch (...) {
    return -1;
  }
}
// returns the encoded size; call with out == nullptr to query
int64_t vpth_encode_jpeg_q75(int width, int height, const uint8_t* rgba8, uint8_t* out, int64_t outlen) {
  auto px = vector<vec4b>((size_t)width * height);
  memcpy(px.data(), rgba8, px.size() * 4);
  auto bytes = encode_jpeg_q75(width, height, px);
  if (out && outlen >= (int64_t)bytes.size()) memcpy(out, bytes.data(), bytes.size());
  return (int64_t)bytes.size();
}

// ---- baking a mesh into a signed-distance grid (include/vpt.h: vpt_bake_sdf; vpt_host.h: bake_sdf) ------------------------------------
// faces (int4 quads, z == w: a triangle; or int3) to the triangles the bake takes: out has room for 2 * nfaces triangles
int vpth_bake_triangles(const int32_t* faces, int nfaces, int corners, int32_t* out, int* count) {
  if (nfaces < 0 || (nfaces > 0 && !faces) || !out || !count || (corners != 3 && corners != 4)) return -1;
  auto shape = shape_data{};
  if (corners == 3) shape.triangles.assign((const vec3i*)faces, (const vec3i*)faces + nfaces);
  else shape.quads.assign((const vec4i*)faces, (const vec4i*)faces + nfaces);
  auto triangles = bake_triangles(shape);
  memcpy(out, triangles.data(), triangles.size() * sizeof(vec3i));
  *count = (int)triangles.size();
  return 0;
}
// bake_sdf over an explicit grid: the host mirror (device < 0) or vpt_bake_sdf on that GPU; voxels: whd[0] * whd[1] * whd[2] floats, untouched on failure
int vpth_bake_grid(const float* positions, int nverts, const int32_t* triangles, int ntris, const int32_t* whd, const float* origin, const float* step,
    int device, float* voxels, vpt_bake_stats* stats, char* err, int errlen) {
  try {
    if (nverts < 0 || ntris < 0 || (nverts > 0 && !positions) || (ntris > 0 && !triangles) || !whd || !origin || !step || !voxels)
      throw std::invalid_argument{"bake_sdf: null pointer or negative count"};
    auto pos = vector<vec3f>((const vec3f*)positions, (const vec3f*)positions + nverts);
    auto tri = vector<vec3i>((const vec3i*)triangles, (const vec3i*)triangles + ntris);
    auto out = vector<float>{};
    auto st  = vpt_bake_stats{};
    if (device < 0) bake_sdf(out, pos, tri, {whd[0], whd[1], whd[2]}, {origin[0], origin[1], origin[2]}, {step[0], step[1], step[2]}, &st);
    else bake_sdf_device(out, pos, tri, {whd[0], whd[1], whd[2]}, {origin[0], origin[1], origin[2]}, {step[0], step[1], step[2]}, device, &st);
    memcpy(voxels, out.data(), out.size() * 4);
    if (stats) *stats = st;
    return 0;
  } catch (const std::exception& e) {
    return set_error(err, errlen, e.what()), -1;
  }
}
int vpth_fit_volume(const float* bmin, const float* bmax, const int32_t* whd, int padding, float* res, float* origin, float* step, float* frame,
    char* err, int errlen) {
  try {
    auto fit = fit_volume({bmin[0], bmin[1], bmin[2]}, {bmax[0], bmax[1], bmax[2]}, {whd[0], whd[1], whd[2]}, padding);
    *res = fit.res;
    memcpy(origin, &fit.origin, 12), memcpy(step, &fit.step, 12), memcpy(frame, &fit.instance.frame, 48);
    return 0;
  } catch (const std::exception& e) {
    return set_error(err, errlen, e.what()), -1;
  }
}
// bake_volume: fit_volume around the triangles, then the bake; frame: the 12 floats of the instance's frame
int vpth_bake_volume(const float* positions, int nverts, const int32_t* triangles, int ntris, const int32_t* whd, int padding, int device, float* voxels,
    float* res, float* frame, vpt_bake_stats* stats, char* err, int errlen) {
  try {
    if (nverts < 0 || ntris < 0 || (nverts > 0 && !positions) || (ntris > 0 && !triangles) || !whd || !voxels || !res || !frame)
      throw std::invalid_argument{"bake_volume: null pointer or negative count"};
    auto baked = bake_volume(vector<vec3f>((const vec3f*)positions, (const vec3f*)positions + nverts),
        vector<vec3i>((const vec3i*)triangles, (const vec3i*)triangles + ntris), {whd[0], whd[1], whd[2]}, padding, device);
    memcpy(voxels, baked.volume.vol.data(), baked.volume.vol.size() * 4);
    *res = baked.volume.res;
    memcpy(frame, &baked.instance.frame, 48);
    if (stats) *stats = baked.stats;
    return 0;
  } catch (const std::exception& e) {
    return set_error(err, errlen, e.what()), -1;
  }
}
// a loaded scene's volume `id`: whd (three int32) and res; its voxels to `voxels` when `capacity` floats hold them; returns their number, -1 for a bad id
int64_t vpth_scene_get_volume(void* hh, int id, int32_t* whd, float* res, float* voxels, int64_t capacity) {
  auto& sc = ((host_scene*)hh)->scene;
  if (id < 0 || id >= (int)sc.volumes.size() || !whd || !res) return -1;
  auto& v = sc.volumes[id];
  whd[0] = v.whd.x, whd[1] = v.whd.y, whd[2] = v.whd.z, *res = v.res;
  auto n = (int64_t)v.whd.x * v.whd.y * v.whd.z;
  if (voxels && capacity >= n && (int64_t)v.vol.size() >= n) memcpy(voxels, v.vol.data(), (size_t)n * 4);
  return n;
}
int vpth_save_volume(const char* filename, const int32_t* whd, float res, const float* voxels, char* err, int errlen) {
  try {
    if (!filename || !whd || !voxels || whd[0] < 1 || whd[1] < 1 || whd[2] < 1) throw std::invalid_argument{"save_volume: null pointer or empty volume"};
    auto vol = volume_data{};
    vol.whd = {whd[0], whd[1], whd[2]}, vol.res = res;
    vol.vol.assign(voxels, voxels + (size_t)whd[0] * whd[1] * whd[2]);
    auto error = string{};
    if (!save_volume(filename, vol, error)) throw std::runtime_error{error};
    return 0;
  } catch (const std::exception& e) {
    return set_error(err, errlen, e.what()), -1;
  }
}

}  // extern "C"
