// vpt_pathtrace.cpp — load-time builders + the drop-in pathtrace_samples() that forwards
// to the HIP path through the C-ABI (include/vpt.h).  No rendering arithmetic lives here.
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>

#include "vpt_host.h"
#include "vpt_hostmath.h"

namespace vpt {

// =============================================================================================
// make_state — per-pixel PCG32 seeding, yocto_pathtrace.cpp:960-980, yocto_sampling.h:184-205
// =============================================================================================
static uint32_t pcg32_next(rng_state& rng) {
  auto old     = rng.state;
  rng.state    = old * 6364136223846793005ULL + rng.inc;
  auto xs      = (uint32_t)(((old >> 18u) ^ old) >> 27u);
  auto rot     = (uint32_t)(old >> 59u);
  return (xs >> rot) | (xs << ((~rot + 1u) & 31));
}
static rng_state pcg32_make(uint64_t seed, uint64_t seq) {
  auto rng  = rng_state{};
  rng.state = 0;
  rng.inc   = (seq << 1u) | 1u;
  pcg32_next(rng);
  rng.state += seed;
  pcg32_next(rng);
  return rng;
}

pathtrace_state make_state(const scene_data& scene, const pathtrace_params& params) {
  if (params.camera < 0 || params.camera >= (int)scene.cameras.size())
    throw std::out_of_range{"camera index out of range"};
  auto& camera = scene.cameras[params.camera];
  auto  state  = pathtrace_state{};
  if (camera.aspect >= 1) {
    state.width  = params.resolution;
    state.height = (int)std::round(params.resolution / camera.aspect);
  } else {
    state.height = params.resolution;
    state.width  = (int)std::round(params.resolution * camera.aspect);
  }
  auto npixels = (size_t)state.width * state.height;
  state.image.assign(npixels, {0, 0, 0, 0});
  state.hits.assign(npixels, 0);
  state.rngs.resize(npixels);
  // master stream: make_rng(1301081) uses the default sequence 1 (yocto_sampling.h:146)
  auto master = pcg32_make(1301081, 1);
  for (auto& rng : state.rngs) {
    // rand1i(rng_, 1 << 31): the int argument wraps to 2147483648u in the unsigned modulo
    auto seq = (int)(pcg32_next(master) % 2147483648u) / 2 + 1;
    rng      = pcg32_make(961748941ull, (uint64_t)seq);
  }
  return state;
}

// =============================================================================================
// make_bvh — middle split (quality 0) or SAH split (quality 1), <=4 prims per leaf.  yocto_bvh.cpp:317-373, 411-441, 447-507, 521-611
// =============================================================================================
static void check_quality(int quality, const char* who) {
  if (quality != VPT_BVH_MIDDLE && quality != VPT_BVH_SAH) throw std::invalid_argument{string{who} + ": unknown bvh quality"};
}
// split_sah's search (include/vpt.h: vpt_build_bvh_quality), the plain form: 45 candidate planes, one pass over the node's primitives
// each.  cbox: the box of the node's centres, not all of its sizes zero.  Returns the axis and, in `split`, the plane; {0, 0.0f} when
// no candidate's cost is below flt_max (an empty side gives 0 * inf = NaN, which never wins).
static int sah_search(const int* prims, int start, int end, const vector<bbox3f>& bboxes, const vector<vec3f>& centers, const bbox3f& cbox, float& split) {
  auto area = [](const bbox3f& b) {
    auto size = b.max - b.min;
    return 1e-12f + 2 * size.x * size.y + 2 * size.x * size.z + 2 * size.y * size.z;
  };
  auto csize = cbox.max - cbox.min;
  auto axis = 0;
  auto min_cost = flt_max;
  split = 0.0f;
  for (auto saxis = 0; saxis < 3; saxis++) {
    for (auto b = 1; b < 16; b++) {
      auto bsplit = comp(cbox.min, saxis) + (float)b * comp(csize, saxis) / 16.0f;
      auto left = bbox3f{}, right = bbox3f{};
      auto nleft = 0, nright = 0;
      for (auto i = start; i < end; i++) {
        if (comp(centers[prims[i]], saxis) < bsplit) left = merge(left, bboxes[prims[i]]), nleft++;
        else right = merge(right, bboxes[prims[i]]), nright++;
      }
      auto cost = 1 + (float)nleft * area(left) / area(cbox) + (float)nright * area(right) / area(cbox);
      if (cost < min_cost) min_cost = cost, split = bsplit, axis = saxis;
    }
  }
  return axis;
}
static void build_nodes(bvh_data& bvh, const vector<bbox3f>& bboxes, int quality = VPT_BVH_MIDDLE) {
  const int max_prims = 4;  // yocto_bvh.cpp:444
  auto      n         = (int)bboxes.size();
  bvh.nodes.clear();
  bvh.nodes.reserve((size_t)n * 2);
  bvh.primitives.resize(n);
  for (auto i = 0; i < n; i++) bvh.primitives[i] = i;
  auto centers = vector<vec3f>(n);
  for (auto i = 0; i < n; i++) centers[i] = center(bboxes[i]);

  struct work { int node, start, end; };
  auto todo = vector<work>{{0, 0, n}};
  bvh.nodes.emplace_back();
  auto* prims = bvh.primitives.data();
  while (!todo.empty()) {
    auto [nodeid, start, end] = todo.back();
    todo.pop_back();
    auto box = bbox3f{};
    for (auto i = start; i < end; i++) box = merge(box, bboxes[prims[i]]);
    auto& node       = bvh.nodes[nodeid];
    node.bbox_min[0] = box.min.x, node.bbox_min[1] = box.min.y, node.bbox_min[2] = box.min.z;
    node.bbox_max[0] = box.max.x, node.bbox_max[1] = box.max.y, node.bbox_max[2] = box.max.z;
    if (end - start <= max_prims) {
      node.internal = 0, node.axis = 0;
      node.num   = (int16_t)(end - start);
      node.start = start;
      continue;
    }
    // split_middle: partition at the centre of the centroid box along its largest axis
    auto cbox = bbox3f{};
    for (auto i = start; i < end; i++) cbox = merge(cbox, centers[prims[i]]);
    auto csize = cbox.max - cbox.min;
    auto mid = (start + end) / 2, axis = 0;
    if (!(csize == vec3f{0, 0, 0})) {
      auto split = 0.0f;
      if (quality == VPT_BVH_SAH) {
        axis = sah_search(prims, start, end, bboxes, centers, cbox, split);
      } else {
        if (csize.x >= csize.y && csize.x >= csize.z) axis = 0;
        if (csize.y >= csize.x && csize.y >= csize.z) axis = 1;
        if (csize.z >= csize.x && csize.z >= csize.y) axis = 2;
        split = comp(center(cbox), axis);
      }
      mid = (int)(std::partition(prims + start, prims + end,
                      [&](int prim) { return comp(centers[prim], axis) < split; }) -
                  prims);
      if (mid == start || mid == end) mid = (start + end) / 2;
    }
    node.internal = 1;
    node.axis     = (int8_t)axis;
    node.num      = 2;
    node.start    = (int)bvh.nodes.size();
    auto first    = node.start;  // `node` dangles after emplace_back only if capacity grew: it cannot
    bvh.nodes.emplace_back();
    bvh.nodes.emplace_back();
    todo.push_back({first + 0, start, mid});
    todo.push_back({first + 1, mid, end});
  }
  bvh.nodes.shrink_to_fit();
}

// the nodes of one tree: on the host (build_nodes) or on a GPU (vpt_build_bvh: the same arrays)
static void build_nodes_on(int device, bvh_data& bvh, const vector<bbox3f>& bboxes, int quality) {
  if (device < 0) return build_nodes(bvh, bboxes, quality);
  static_assert(sizeof(bbox3f) == 6 * sizeof(float), "bbox layout");
  auto n = (int)bboxes.size(), count = 0;
  bvh.nodes.assign((size_t)std::max(1, 2 * n), bvh_node{});
  bvh.primitives.assign((size_t)n, 0);
  if (vpt_build_bvh_quality(device, (const float*)bboxes.data(), n, quality, bvh.nodes.data(), (int)bvh.nodes.size(), &count, bvh.primitives.data()) != VPT_OK)
    throw std::runtime_error{string{"make_bvh_device: "} + vpt_last_error()};
  bvh.nodes.resize((size_t)count);
  bvh.nodes.shrink_to_fit();
}
bvh_data build_bvh_host(const float* bboxes, int n, int quality) {
  check_quality(quality, "build_bvh_host");
  auto boxes = vector<bbox3f>((size_t)n);
  if (n > 0) memcpy((void*)boxes.data(), bboxes, (size_t)n * sizeof(bbox3f));
  auto bvh = bvh_data{};
  build_nodes(bvh, boxes, quality);
  return bvh;
}

// the primitives' bounds of a shape, in the reference's order: points, lines, triangles, quads (yocto_bvh.cpp:536-565, 620-649)
static vector<bbox3f> shape_bboxes(const shape_data& shape) {
  auto bboxes = vector<bbox3f>{};
  // point_bounds(p, r) / line_bounds(p0, p1, r0, r1), yocto_geometry.h:461-471, in the reference's order: points, lines, faces
  auto sub = [](const vec3f& p, float r) { return vec3f{p.x - r, p.y - r, p.z - r}; };
  auto add = [](const vec3f& p, float r) { return vec3f{p.x + r, p.y + r, p.z + r}; };
  if (!shape.points.empty()) {
    bboxes.resize(shape.points.size());
    for (size_t i = 0; i < bboxes.size(); i++) {
      auto& p = shape.positions[shape.points[i]];
      auto  r = shape.radius[shape.points[i]];
      bboxes[i] = {vmin(sub(p, r), add(p, r)), vmax(sub(p, r), add(p, r))};
    }
  } else if (!shape.lines.empty()) {
    bboxes.resize(shape.lines.size());
    for (size_t i = 0; i < bboxes.size(); i++) {
      auto& l = shape.lines[i];
      auto &p0 = shape.positions[l.x], &p1 = shape.positions[l.y];
      auto  r0 = shape.radius[l.x], r1 = shape.radius[l.y];
      bboxes[i] = {vmin(sub(p0, r0), sub(p1, r1)), vmax(add(p0, r0), add(p1, r1))};
    }
  } else if (!shape.triangles.empty()) {
    bboxes.resize(shape.triangles.size());
    for (size_t i = 0; i < bboxes.size(); i++) {
      auto& t = shape.triangles[i];
      auto &p0 = shape.positions[t.x], &p1 = shape.positions[t.y], &p2 = shape.positions[t.z];
      bboxes[i] = {vmin(p0, vmin(p1, p2)), vmax(p0, vmax(p1, p2))};
    }
  } else if (!shape.quads.empty()) {
    bboxes.resize(shape.quads.size());
    for (size_t i = 0; i < bboxes.size(); i++) {
      auto& q = shape.quads[i];
      auto &p0 = shape.positions[q.x], &p1 = shape.positions[q.y], &p2 = shape.positions[q.z],
           &p3 = shape.positions[q.w];
      bboxes[i] = {vmin(p0, vmin(p1, vmin(p2, p3))), vmax(p0, vmax(p1, vmax(p2, p3)))};
    }
  }
  return bboxes;
}
static bvh_data make_shape_bvh(const shape_data& shape, int device, int quality) {
  auto bvh = bvh_data{};
  build_nodes_on(device, bvh, shape_bboxes(shape), quality);
  return bvh;
}

// the instances' bounds: transform_bbox(frame, root box of the shape's BVH); invalidb3f for a shape without nodes
static vector<bbox3f> instance_bboxes(const scene_data& scene, const bvh_data& bvh) {
  auto bboxes = vector<bbox3f>(scene.instances.size());
  for (size_t i = 0; i < bboxes.size(); i++) {
    auto& instance = scene.instances[i];
    auto& sbvh     = bvh.shapes.at(instance.shape);
    if (sbvh.nodes.empty()) continue;  // invalidb3f
    auto& root = sbvh.nodes[0];
    auto  box  = bbox3f{};  // transform_bbox, yocto_geometry.h:441-452: 8 corners, z fastest
    for (auto cx = 0; cx < 2; cx++)
      for (auto cy = 0; cy < 2; cy++)
        for (auto cz = 0; cz < 2; cz++) {
          auto corner = vec3f{cx ? root.bbox_max[0] : root.bbox_min[0],
              cy ? root.bbox_max[1] : root.bbox_min[1], cz ? root.bbox_max[2] : root.bbox_min[2]};
          box = merge(box, transform_point(instance.frame, corner));
        }
    bboxes[i] = box;
  }
  return bboxes;
}

static bvh_scene make_bvh_on(int device, const scene_data& scene, int quality) {
  auto bvh = bvh_data{};
  bvh.shapes.resize(scene.shapes.size());
  for (size_t i = 0; i < scene.shapes.size(); i++) bvh.shapes[i] = make_shape_bvh(scene.shapes[i], device, quality);
  build_nodes_on(device, bvh, instance_bboxes(scene, bvh), quality);
  return bvh;
}

// refit_bvh, yocto_bvh.cpp:510-524: nodes in reverse order (children follow their parent), every box from invalidb3f
static void refit_nodes(bvh_data& bvh, const vector<bbox3f>& bboxes) {
  for (auto nodeid = (int)bvh.nodes.size() - 1; nodeid >= 0; nodeid--) {
    auto& node = bvh.nodes[nodeid];
    auto  box  = bbox3f{};
    if (node.internal) {
      for (auto idx = 0; idx < 2; idx++) {
        auto& child = bvh.nodes[node.start + idx];
        box = merge(box, bbox3f{{child.bbox_min[0], child.bbox_min[1], child.bbox_min[2]}, {child.bbox_max[0], child.bbox_max[1], child.bbox_max[2]}});
      }
    } else {
      for (auto idx = 0; idx < node.num; idx++) box = merge(box, bboxes[bvh.primitives[node.start + idx]]);
    }
    node.bbox_min[0] = box.min.x, node.bbox_min[1] = box.min.y, node.bbox_min[2] = box.min.z;
    node.bbox_max[0] = box.max.x, node.bbox_max[1] = box.max.y, node.bbox_max[2] = box.max.z;
  }
}
// update_bvh, yocto_bvh.cpp:680-689: the edited shapes, then the scene BVH from all instances (`updated_instances` is not read
// by the reference's own refit either)
void update_bvh(bvh_scene& bvh, const scene_data& scene, const vector<int>& updated_instances, const vector<int>& updated_shapes) {
  (void)updated_instances;
  for (auto shape : updated_shapes) refit_nodes(bvh.shapes.at(shape), shape_bboxes(scene.shapes.at(shape)));
  refit_nodes(bvh, instance_bboxes(scene, bvh));
}
void rebuild_bvh(bvh_scene& bvh, const scene_data& scene, const vector<int>& shapes, bool scene_level, int quality) {
  check_quality(quality, "rebuild_bvh");
  auto seen = vector<char>(scene.shapes.size(), 0);
  for (auto shape : shapes) {
    if (shape < 0 || shape >= (int)scene.shapes.size()) throw std::invalid_argument{"rebuild_bvh: shape id out of range"};
    if (seen[(size_t)shape]) throw std::invalid_argument{"rebuild_bvh: shape id repeated"};
    seen[(size_t)shape] = 1;
  }
  for (auto shape : shapes) bvh.shapes[(size_t)shape] = make_shape_bvh(scene.shapes[(size_t)shape], -1, quality);
  if (!scene_level && shapes.empty()) return;
  auto top = bvh_data{};
  build_nodes(top, instance_bboxes(scene, bvh), quality);
  bvh.nodes = std::move(top.nodes), bvh.primitives = std::move(top.primitives);
}
bvh_scene make_bvh(const scene_data& scene, const pathtrace_params&, int quality) {
  check_quality(quality, "make_bvh");
  return make_bvh_on(-1, scene, quality);
}
bvh_scene make_bvh_device(const scene_data& scene, const pathtrace_params&, int device, int quality) {
  if (device < 0) throw std::invalid_argument{"make_bvh_device: negative device"};
  check_quality(quality, "make_bvh_device");
  return make_bvh_on(device, scene, quality);
}

// tesselate_surfaces: host/vpt_tesselate.cpp

// =============================================================================================
// make_lights — serial float32 running sums.  yocto_pathtrace.cpp:983-1049
// =============================================================================================
void edit_instances(scene_data& scene, bvh_scene& bvh, pathtrace_lights& lights, const vector<int>& remove, const vector<int>& set_ids,
    const vector<instance_data>& set, const vector<instance_data>& add) {
  const auto n = (int)scene.instances.size();
  if (set_ids.size() != set.size()) throw std::invalid_argument{"edit_instances: set ids and instances differ in number"};
  auto removed = vector<char>((size_t)n, 0), is_set = vector<char>((size_t)n, 0);
  for (auto id : remove) {
    if (id < 0 || id >= n) throw std::invalid_argument{"edit_instances: removed id out of range"};
    if (removed[(size_t)id]) throw std::invalid_argument{"edit_instances: removed id repeated"};
    removed[(size_t)id] = 1;
  }
  for (auto id : set_ids) {
    if (id < 0 || id >= n) throw std::invalid_argument{"edit_instances: set id out of range"};
    if (is_set[(size_t)id]) throw std::invalid_argument{"edit_instances: set id repeated"};
    if (removed[(size_t)id]) throw std::invalid_argument{"edit_instances: an id is both set and removed"};
    is_set[(size_t)id] = 1;
  }
  for (auto* list : {&set, &add})
    for (auto& in : *list) {
      if (in.shape < 0 || in.shape >= (int)scene.shapes.size()) throw std::invalid_argument{"edit_instances: shape out of range"};
      if (in.material < 0 || in.material >= (int)scene.materials.size()) throw std::invalid_argument{"edit_instances: material out of range"};
    }
  for (auto i = (size_t)0; i < set.size(); i++) scene.instances[(size_t)set_ids[i]] = set[i];
  for (auto id = n - 1; id >= 0; id--)   // erase from the back: the ids of the list are the current ones throughout
    if (removed[(size_t)id]) scene.instances.erase(scene.instances.begin() + id);
  for (auto& in : add) scene.instances.push_back(in);
  rebuild_bvh(bvh, scene, {}, true);
  lights = make_lights(scene, pathtrace_params{});
}
void edit_shapes(scene_data& scene, bvh_scene& bvh, pathtrace_lights& lights, const vector<int>& remove, const vector<int>& set_ids,
    const vector<shape_data>& set, const vector<shape_data>& add) {
  const auto n = (int)scene.shapes.size();
  if (set_ids.size() != set.size()) throw std::invalid_argument{"edit_shapes: set ids and shapes differ in number"};
  if (bvh.shapes.size() != scene.shapes.size()) throw std::invalid_argument{"edit_shapes: bvh does not belong to this scene"};
  auto removed = vector<char>((size_t)n, 0), is_set = vector<char>((size_t)n, 0);
  for (auto id : remove) {
    if (id < 0 || id >= n) throw std::invalid_argument{"edit_shapes: removed id out of range"};
    if (removed[(size_t)id]) throw std::invalid_argument{"edit_shapes: removed id repeated"};
    removed[(size_t)id] = 1;
  }
  for (auto id : set_ids) {
    if (id < 0 || id >= n) throw std::invalid_argument{"edit_shapes: set id out of range"};
    if (is_set[(size_t)id]) throw std::invalid_argument{"edit_shapes: set id repeated"};
    if (removed[(size_t)id]) throw std::invalid_argument{"edit_shapes: an id is both set and removed"};
    is_set[(size_t)id] = 1;
  }
  for (auto& in : scene.instances)
    if (removed[(size_t)in.shape]) throw std::invalid_argument{"edit_shapes: a removed shape is still named by an instance"};
  for (auto* list : {&set, &add})
    for (auto& shape : *list) {   // the rules of vpt_scene_create for one shape
      auto nv = (int)shape.positions.size();
      if (!shape.triangles.empty() && !shape.quads.empty()) throw std::invalid_argument{"edit_shapes: both triangles and quads"};
      if ((int)!shape.points.empty() + (int)!shape.lines.empty() + (int)(!shape.triangles.empty() || !shape.quads.empty()) > 1)
        throw std::invalid_argument{"edit_shapes: a shape that mixes points, lines and faces is not supported"};
      if ((!shape.points.empty() || !shape.lines.empty()) && shape.radius.size() != shape.positions.size())
        throw std::invalid_argument{"edit_shapes: a shape of points or lines needs one radius per vertex"};
      if ((!shape.normals.empty() && shape.normals.size() != shape.positions.size()) || (!shape.texcoords.empty() && shape.texcoords.size() != shape.positions.size()) ||
          (!shape.colors.empty() && shape.colors.size() != shape.positions.size()))
        throw std::invalid_argument{"edit_shapes: a vertex attribute differs from the positions in number"};
      auto ok = [nv](int v) { return v >= 0 && v < nv; };
      for (auto v : shape.points)
        if (!ok(v)) throw std::invalid_argument{"edit_shapes: point vertex index out of range"};
      for (auto& l : shape.lines)
        if (!ok(l.x) || !ok(l.y)) throw std::invalid_argument{"edit_shapes: line vertex index out of range"};
      for (auto& t : shape.triangles)
        if (!ok(t.x) || !ok(t.y) || !ok(t.z)) throw std::invalid_argument{"edit_shapes: triangle vertex index out of range"};
      for (auto& q : shape.quads)
        if (!ok(q.x) || !ok(q.y) || !ok(q.z) || !ok(q.w)) throw std::invalid_argument{"edit_shapes: quad vertex index out of range"};
    }
  for (auto i = (size_t)0; i < set.size(); i++) scene.shapes[(size_t)set_ids[i]] = set[i];
  auto new_of_old = vector<int>((size_t)n, -1);
  for (auto id = 0, next = 0; id < n; id++)
    if (!removed[(size_t)id]) new_of_old[(size_t)id] = next++;
  for (auto id = n - 1; id >= 0; id--)   // erase from the back: the ids of the list are the current ones throughout
    if (removed[(size_t)id]) scene.shapes.erase(scene.shapes.begin() + id), bvh.shapes.erase(bvh.shapes.begin() + id);
  for (auto& shape : add) scene.shapes.push_back(shape), bvh.shapes.emplace_back();
  for (auto& in : scene.instances) in.shape = new_of_old[(size_t)in.shape];
  for (auto& sd : scene.subdivs)
    if (sd.shape >= 0 && sd.shape < n) sd.shape = new_of_old[(size_t)sd.shape];
  // make_bvh for the replaced and the added shapes; the scene BVH only when a shape was replaced (another root box) - an added shape
  // has no instance yet and a removed one had none, so the untouched trees and the scene's keep the form they have, refitted or not
  for (auto id : set_ids) bvh.shapes[(size_t)new_of_old[(size_t)id]] = make_shape_bvh(scene.shapes[(size_t)new_of_old[(size_t)id]], -1, VPT_BVH_MIDDLE);
  for (auto id = scene.shapes.size() - add.size(); id < scene.shapes.size(); id++) bvh.shapes[id] = make_shape_bvh(scene.shapes[id], -1, VPT_BVH_MIDDLE);
  if (!set.empty()) rebuild_bvh(bvh, scene, {}, true);
  lights = make_lights(scene, pathtrace_params{});
}
pathtrace_lights make_lights(const scene_data& scene, const pathtrace_params&) {
  auto lights = pathtrace_lights{};
  for (auto handle = 0; handle < (int)scene.instances.size(); handle++) {
    auto& instance = scene.instances[handle];
    auto& material = scene.materials.at(instance.material);
    if (material.emission == vec3f{0, 0, 0}) continue;
    auto& shape = scene.shapes.at(instance.shape);
    if (shape.triangles.empty() && shape.quads.empty()) continue;
    auto& light    = lights.lights.emplace_back();
    light.instance = handle;
    auto& cdf      = light.elements_cdf;
    auto& pos      = shape.positions;
    if (!shape.triangles.empty()) {
      cdf.resize(shape.triangles.size());
      for (size_t i = 0; i < cdf.size(); i++) {
        auto& t = shape.triangles[i];
        cdf[i]  = triangle_area(pos[t.x], pos[t.y], pos[t.z]);
        if (i != 0) cdf[i] += cdf[i - 1];
      }
    }
    if (!shape.quads.empty()) {
      cdf.resize(shape.quads.size());
      for (size_t i = 0; i < cdf.size(); i++) {
        auto& q = shape.quads[i];
        cdf[i]  = quad_area(pos[q.x], pos[q.y], pos[q.z], pos[q.w]);
        if (i != 0) cdf[i] += cdf[i - 1];
      }
    }
  }
  for (auto handle = 0; handle < (int)scene.environments.size(); handle++) {
    auto& environment = scene.environments[handle];
    if (environment.emission == vec3f{0, 0, 0}) continue;
    auto& light       = lights.lights.emplace_back();
    light.environment = handle;
    if (environment.emission_tex == invalidid) continue;
    auto& texture = scene.textures.at(environment.emission_tex);
    auto& cdf     = light.elements_cdf;
    cdf.resize((size_t)texture.width * texture.height);
    for (size_t idx = 0; idx < cdf.size(); idx++) {
      auto i = (int)(idx % texture.width), j = (int)(idx / texture.width);
      auto th = (j + 0.5f) * pif / texture.height;
      // lookup_texture(texture, i, j) without as_linear, then max over ALL FOUR channels
      // (yocto_math.h:1824 — alpha = 1 participates; kept on purpose)
      auto value = vec4f{};
      if (!texture.pixelsf.empty()) {
        value = texture.pixelsf[(size_t)j * texture.width + i];
      } else {
        auto b = texture.pixelsb[(size_t)j * texture.width + i];
        value  = {b.x / 255.0f, b.y / 255.0f, b.z / 255.0f, b.w / 255.0f};
      }
      auto m   = fmax_(fmax_(fmax_(value.x, value.y), value.z), value.w);
      cdf[idx] = m * std::sin(th);
      if (idx != 0) cdf[idx] += cdf[idx - 1];
    }
  }
  for (auto handle = 0; handle < (int)scene.sdfs.size(); handle++) {
    auto& sdf      = scene.sdfs[handle];
    auto& material = scene.materials.at(sdf.material);
    if (material.emission == vec3f{0, 0, 0}) continue;
    auto& light        = lights.lights.emplace_back();
    light.sdf          = handle;
    light.elements_cdf = {sdf.whd.x * sdf.whd.y};
  }
  return lights;
}

// =============================================================================================
// flatten to the C-ABI
// =============================================================================================
static vpt_frame to_abi(const frame3f& f) {
  auto r = vpt_frame{};
  std::memcpy(&r, &f, sizeof(r));
  return r;
}

vpt_params to_abi(const pathtrace_params& p) {
  auto r                = vpt_params{};
  r.camera              = p.camera;
  r.resolution          = p.resolution;
  r.shader              = (int)p.shader;
  r.samples             = p.samples;
  r.bounces             = p.bounces;
  r.noparallel          = p.noparallel;
  r.noimplicit_mis      = p.noimplicit_mis;
  r.spheretrace_maxiter = p.spheretrace_maxiter;
  return r;
}

void flatten_scene(flat_scene& flat, const scene_data& scene, const bvh_scene& bvh,
    const pathtrace_lights& lights) {
  if (bvh.shapes.size() != scene.shapes.size())
    throw std::invalid_argument{"bvh does not belong to this scene"};
  for (auto& c : scene.cameras) {
    auto& d = flat.cameras.emplace_back();
    d.frame = to_abi(c.frame), d.orthographic = c.orthographic, d.lens = c.lens, d.film = c.film;
    d.aspect = c.aspect, d.focus = c.focus, d.aperture = c.aperture;
  }
  for (size_t s = 0; s < scene.shapes.size(); s++) {
    auto& shape = scene.shapes[s];
    // a shape of points or lines holds nothing else: the reference's BVH tests points first, its eval_* functions faces first
    auto kinds = (int)!shape.points.empty() + (int)!shape.lines.empty() + (int)(!shape.triangles.empty() || !shape.quads.empty());
    if (kinds > 1 && (!shape.points.empty() || !shape.lines.empty()))
      throw std::invalid_argument{"a shape that mixes points, lines and faces is not supported"};
    if ((!shape.points.empty() || !shape.lines.empty()) && shape.radius.size() != shape.positions.size())
      throw std::invalid_argument{"a shape of points or lines needs one radius per vertex"};
    auto& c         = flat.shape_curves.emplace_back();
    c.num_points    = (int)shape.points.size(), c.point_offset = (int)flat.points.size();
    c.num_lines     = (int)shape.lines.size(), c.line_offset = (int)flat.lines.size();
    c.radius_offset = shape.radius.empty() ? -1 : (int)flat.radius.size();
    flat.points.insert(flat.points.end(), shape.points.begin(), shape.points.end());
    flat.lines.insert(flat.lines.end(), shape.lines.begin(), shape.lines.end());
    flat.radius.insert(flat.radius.end(), shape.radius.begin(), shape.radius.end());
    auto& d           = flat.shapes.emplace_back();
    d.num_vertices    = (int)shape.positions.size();
    d.position_offset = (int)flat.positions.size();
    flat.positions.insert(flat.positions.end(), shape.positions.begin(), shape.positions.end());
    d.normal_offset = shape.normals.empty() ? -1 : (int)flat.normals.size();
    flat.normals.insert(flat.normals.end(), shape.normals.begin(), shape.normals.end());
    d.texcoord_offset = shape.texcoords.empty() ? -1 : (int)flat.texcoords.size();
    flat.texcoords.insert(flat.texcoords.end(), shape.texcoords.begin(), shape.texcoords.end());
    d.color_offset = shape.colors.empty() ? -1 : (int)flat.colors.size();
    flat.colors.insert(flat.colors.end(), shape.colors.begin(), shape.colors.end());
    d.num_triangles = (int)shape.triangles.size(), d.triangle_offset = (int)flat.triangles.size();
    flat.triangles.insert(flat.triangles.end(), shape.triangles.begin(), shape.triangles.end());
    // the reference tests triangles first (yocto_bvh.cpp:770-789): a shape with both keeps only them
    d.num_quads = shape.triangles.empty() ? (int)shape.quads.size() : 0;
    d.quad_offset = (int)flat.quads.size();
    if (d.num_quads) flat.quads.insert(flat.quads.end(), shape.quads.begin(), shape.quads.end());
    auto& sb          = bvh.shapes[s];
    d.num_bvh_nodes   = (int)sb.nodes.size();
    d.bvh_node_offset = (int)flat.shape_nodes.size();
    d.bvh_prim_offset = (int)flat.shape_prims.size();
    flat.shape_nodes.insert(flat.shape_nodes.end(), sb.nodes.begin(), sb.nodes.end());
    flat.shape_prims.insert(flat.shape_prims.end(), sb.primitives.begin(), sb.primitives.end());
  }
  for (auto& i : scene.instances) {
    auto& d = flat.instances.emplace_back();
    d.frame = to_abi(i.frame), d.shape = i.shape, d.material = i.material;
  }
  for (auto& m : scene.materials) {
    auto& d = flat.materials.emplace_back();
    d.type  = (int)m.type;
    std::memcpy(d.emission, &m.emission, 12), std::memcpy(d.color, &m.color, 12);
    d.roughness = m.roughness, d.metallic = m.metallic, d.ior = m.ior;
    std::memcpy(d.scattering, &m.scattering, 12);
    d.scanisotropy = m.scanisotropy, d.trdepth = m.trdepth, d.opacity = m.opacity;
    d.emission_tex = m.emission_tex, d.color_tex = m.color_tex, d.roughness_tex = m.roughness_tex;
    d.scattering_tex = m.scattering_tex, d.normal_tex = m.normal_tex;
  }
  for (auto& t : scene.textures) {
    auto& d = flat.textures.emplace_back();
    d.width = t.width, d.height = t.height, d.linear = t.linear;
    d.is_float = !t.pixelsf.empty();
    if (d.is_float) {
      d.offset = (int64_t)flat.texels_f.size();
      flat.texels_f.insert(flat.texels_f.end(), t.pixelsf.begin(), t.pixelsf.end());
    } else {
      d.offset = (int64_t)flat.texels_b.size();
      flat.texels_b.insert(flat.texels_b.end(), t.pixelsb.begin(), t.pixelsb.end());
    }
  }
  for (auto& e : scene.environments) {
    auto& d = flat.environments.emplace_back();
    d.frame = to_abi(e.frame), d.emission_tex = e.emission_tex;
    std::memcpy(d.emission, &e.emission, 12);
  }
  for (auto& v : scene.volumes) {
    auto& d  = flat.volumes.emplace_back();
    d.whd[0] = v.whd.x, d.whd[1] = v.whd.y, d.whd[2] = v.whd.z, d.res = v.res;
    d.offset = (int64_t)flat.voxels.size();
    flat.voxels.insert(flat.voxels.end(), v.vol.begin(), v.vol.end());
  }
  for (auto& i : scene.vol_instances) {
    auto& d = flat.vol_instances.emplace_back();
    d.frame = to_abi(i.frame), d.volume = i.volume, d.material = i.material, d.scalef = i.scalef;
  }
  for (auto& s : scene.sdfs) {
    auto& d = flat.sdfs.emplace_back();
    d.frame = to_abi(s.frame), d.type = (int)s.type, d.material = s.material;
    std::memcpy(d.whd, &s.whd, 12), std::memcpy(d.p, s.p, 16);
  }
  for (auto& l : lights.lights) {
    auto& d = flat.lights.emplace_back();
    d.instance = l.instance, d.environment = l.environment, d.sdf = l.sdf;
    d.cdf_len = (int)l.elements_cdf.size(), d.cdf_offset = (int64_t)flat.light_cdf.size();
    flat.light_cdf.insert(flat.light_cdf.end(), l.elements_cdf.begin(), l.elements_cdf.end());
  }
  flat.scene_nodes = bvh.nodes, flat.scene_prims = bvh.primitives;

  auto& d = flat.desc;
  d       = {};
#define VPT_SET(count, ptr, vec) d.count = (decltype(d.count))flat.vec.size(), d.ptr = flat.vec.empty() ? nullptr : (decltype(d.ptr))flat.vec.data()
  VPT_SET(num_cameras, cameras, cameras);
  VPT_SET(num_instances, instances, instances);
  VPT_SET(num_shapes, shapes, shapes);
  VPT_SET(num_materials, materials, materials);
  VPT_SET(num_textures, textures, textures);
  VPT_SET(num_environments, environments, environments);
  VPT_SET(num_volumes, volumes, volumes);
  VPT_SET(num_vol_instances, vol_instances, vol_instances);
  VPT_SET(num_sdfs, sdfs, sdfs);
  VPT_SET(num_lights, lights, lights);
  VPT_SET(num_positions, positions, positions);
  VPT_SET(num_normals, normals, normals);
  VPT_SET(num_texcoords, texcoords, texcoords);
  VPT_SET(num_colors, colors, colors);
  VPT_SET(num_triangles, triangles, triangles);
  VPT_SET(num_quads, quads, quads);
  VPT_SET(num_texels_f, texels_f, texels_f);
  VPT_SET(num_texels_b, texels_b, texels_b);
  VPT_SET(num_voxels, voxels, voxels);
  VPT_SET(num_light_cdf, light_cdf, light_cdf);
  VPT_SET(num_scene_bvh_nodes, scene_bvh_nodes, scene_nodes);
  VPT_SET(num_scene_bvh_prims, scene_bvh_prims, scene_prims);
  VPT_SET(num_shape_bvh_nodes, shape_bvh_nodes, shape_nodes);
  VPT_SET(num_shape_bvh_prims, shape_bvh_prims, shape_prims);
  // the side struct (include/vpt.h: vpt_scene_curves) only when some shape has points or lines: a scene of faces is created as before
  auto any_curves = false;
  for (auto& c : flat.shape_curves) any_curves |= c.num_points > 0 || c.num_lines > 0;
#undef VPT_SET
  flat.curves = {};
  if (any_curves) {
    auto& c = flat.curves;
    c.shape_curves = flat.shape_curves.data();
    c.num_points = (int64_t)flat.points.size(), c.points = flat.points.empty() ? nullptr : flat.points.data();
    c.num_lines = (int64_t)flat.lines.size(), c.lines = flat.lines.empty() ? nullptr : (const int32_t*)flat.lines.data();
    c.num_radius = (int64_t)flat.radius.size(), c.radius = flat.radius.empty() ? nullptr : flat.radius.data();
  }
}

// =============================================================================================
// pathtrace_samples — the drop-in.  Device copies of scenes are cached per scene_data address + content fingerprint.
// =============================================================================================
namespace {
// The reference's API has no release hook and keys nothing: a caller may mutate the scene, rebuild bvh / lights or
// allocate another scene at the same address between two calls.  The cached device copy therefore carries a cheap
// fingerprint of what it was made from (addresses and sizes of the containers the flattening reads, a hash over the
// heads of the big arrays); a mismatch rebuilds it.
struct device_entry {
  vpt_multi* handle = nullptr;
  vpt_scene* single = nullptr;   // pathtrace_adaptive's copy on one GPU (vpt_render_adaptive), made on first use
  uint64_t   fingerprint = 0;
  uint64_t   cameras     = 0;    // fingerprint of the cameras table alone: a change of it is an edit of the resident copy
  ~device_entry() {
    if (handle) vpt_multi_destroy(handle);
    if (single) vpt_scene_destroy(single);
  }
};
std::mutex                                                   cache_mutex;
std::map<const scene_data*, std::unique_ptr<device_entry>>& device_cache() {
  static auto cache = std::map<const scene_data*, std::unique_ptr<device_entry>>{};
  return cache;
}
vector<int>& device_list() {
  static auto devices = vector<int>{0};
  return devices;
}
uint64_t mix(uint64_t h, uint64_t v) { return (h ^ v) * 0x100000001b3ull; }
template <typename T>
uint64_t mix_array(uint64_t h, const vector<T>& v) {   // bulk arrays: address, size, head and tail
  h = mix(mix(h, (uint64_t)(uintptr_t)v.data()), v.size());
  auto bytes = (const unsigned char*)v.data();
  auto n     = v.size() * sizeof(T);
  for (size_t i = 0; i < n && i < 256; i++) h = mix(h, bytes[i]);          // head
  for (size_t i = n > 256 ? n - 256 : n; i < n; i++) h = mix(h, bytes[i]);  // tail
  return h;
}
template <typename T>
uint64_t mix_table(uint64_t h, const vector<T>& v) {   // small tables (a few KB): every byte, eight at a time
  h = mix(mix(h, (uint64_t)(uintptr_t)v.data()), v.size());
  auto bytes = (const unsigned char*)v.data();
  auto n     = v.size() * sizeof(T);
  auto i     = (size_t)0;
  for (; i + 8 <= n; i += 8) {
    uint64_t w;
    memcpy(&w, bytes + i, 8);
    h = mix(h, w);
  }
  for (; i < n; i++) h = mix(h, bytes[i]);
  return h;
}
// What the cached device copy was made from.  The small tables - cameras, instances, materials, environments, volume
// instances, SDFs, light ids - are hashed in full, so an in-place edit of any of them (a moved instance, a changed material or
// camera) rebuilds the copy on the next call, as the reference - which reads the live scene - would show it.  The bulk arrays
// (vertex data, texels, voxels, BVH nodes, light CDFs) are sampled at head and tail only: editing them in place between two calls
// needs pathtrace_release(scene) (vpt_host.h).  The cameras have a fingerprint of their own: a camera edited in place (the
// reference's viewer does it on every mouse drag, apps/ypathtrace/ypathtrace.cpp:269-297) goes to the resident copy through
// vpt_scene_update instead of making a new one.
uint64_t scene_fingerprint(const scene_data& scene, const bvh_scene& bvh, const pathtrace_lights& lights) {
  auto h = 0xcbf29ce484222325ull;
  h = mix(h, scene.cameras.size()), h = mix_table(h, scene.instances), h = mix_table(h, scene.materials);
  h = mix_table(h, scene.environments), h = mix_table(h, scene.vol_instances), h = mix_table(h, scene.sdfs);
  h = mix(h, scene.shapes.size()), h = mix(h, scene.textures.size()), h = mix(h, scene.volumes.size());
  for (auto& s : scene.shapes) h = mix_array(h, s.positions), h = mix(h, s.triangles.size()), h = mix(h, s.quads.size()),
                              h = mix(h, s.points.size()), h = mix(h, s.lines.size()), h = mix_array(h, s.radius);
  for (auto& t : scene.textures) h = mix(mix(h, (uint64_t)t.width), (uint64_t)t.height), h = mix_array(h, t.pixelsb), h = mix_array(h, t.pixelsf);
  for (auto& v : scene.volumes) h = mix_array(h, v.vol);
  h = mix_array(h, bvh.nodes), h = mix_array(h, bvh.primitives), h = mix(h, bvh.shapes.size());
  for (auto& b : bvh.shapes) h = mix_array(h, b.nodes);
  h = mix(h, lights.lights.size());
  for (auto& l : lights.lights) h = mix(mix(mix(h, (uint64_t)l.instance), (uint64_t)l.environment), (uint64_t)l.sdf), h = mix_array(h, l.elements_cdf);
  return h;
}
// the cache entry of `scene` (cache_mutex held): a fresh one, without device copies, when the fingerprint changed
device_entry& cached_entry(const scene_data& scene, const bvh_scene& bvh, const pathtrace_lights& lights) {
  auto& entry = device_cache()[&scene];
  auto  print = scene_fingerprint(scene, bvh, lights);
  auto  cams  = mix_table(0xcbf29ce484222325ull, scene.cameras);
  if (!entry || entry->fingerprint != print) {
    entry.reset();
    entry              = std::make_unique<device_entry>();
    entry->fingerprint = print, entry->cameras = cams;
  } else if (entry->cameras != cams) {
    auto ids = vector<int32_t>{};
    auto abi = vector<vpt_camera>{};
    for (auto& c : scene.cameras) {
      ids.push_back((int32_t)ids.size());
      auto& d = abi.emplace_back();
      d.frame = to_abi(c.frame), d.orthographic = c.orthographic, d.lens = c.lens, d.film = c.film;
      d.aspect = c.aspect, d.focus = c.focus, d.aperture = c.aperture;
    }
    auto edit = vpt_scene_edit{};
    edit.num_cameras = (int32_t)ids.size(), edit.camera_ids = ids.data(), edit.cameras = abi.data();
    if ((entry->handle && vpt_multi_update(entry->handle, &edit) != VPT_OK) || (entry->single && vpt_scene_update(entry->single, &edit) != VPT_OK)) {
      entry.reset();   // the copy may be half edited: it goes
      device_cache().erase(&scene);
      throw std::runtime_error{string{"vpt_scene_update: "} + vpt_last_error()};
    }
    entry->cameras = cams;
  }
  return *entry;
}
// the copy of `scene` on the first device alone (cache_mutex held), made on first use: pathtrace_adaptive, pathtrace_aovs
vpt_scene* single_scene(const scene_data& scene, const bvh_scene& bvh, const pathtrace_lights& lights) {
  auto& entry = cached_entry(scene, bvh, lights);
  if (!entry.single) {
    auto flat = flat_scene{};
    flatten_scene(flat, scene, bvh, lights);
    if (vpt_scene_create_curves(&flat.desc, flat.curves_or_null(), device_list()[0], &entry.single) != VPT_OK) {
      entry.single = nullptr;
      device_cache().erase(&scene);
      throw std::runtime_error{string{"vpt_scene_create_curves: "} + vpt_last_error()};
    }
  }
  return entry.single;
}
}  // namespace

pathtrace_aov_images pathtrace_aovs(const scene_data& scene, const bvh_scene& bvh, const pathtrace_lights& lights, const pathtrace_params& params,
    int samples, unsigned planes) {
  if (samples < 1) throw std::invalid_argument{"aov samples must be >= 1"};
  if ((planes & aov_all) == 0) throw std::invalid_argument{"no aov plane asked for"};
  auto handle = (vpt_scene*)nullptr;
  {
    auto lock = std::lock_guard{cache_mutex};
    handle    = single_scene(scene, bvh, lights);
  }
  auto p    = params;
  p.shader  = pathtrace_shader_type::normal, p.samples = samples;
  auto state = make_state(scene, p);
  auto n     = (size_t)state.width * state.height;
  auto out   = pathtrace_aov_images{};
  auto abi   = vpt_aov_planes{};
  auto sums  = [&](unsigned bit, color_image& image) -> void* {
    if (!(planes & bit)) return nullptr;
    image = color_image{state.width, state.height, true, vector<vec4f>(n)};
    return image.pixels.data();
  };
  abi.normal = sums(aov_normal, out.normal), abi.albedo = sums(aov_albedo, out.albedo);
  abi.texcoord = sums(aov_texcoord, out.texcoord), abi.depth = sums(aov_depth, out.depth);
  if (planes & aov_ids) out.ids.resize(n), out.uvt.resize(n), abi.ids = out.ids.data(), abi.uvt = out.uvt.data();
  static_assert(sizeof(vec2i) == 8 && sizeof(vec3f) == 12 && sizeof(vec4f) == 16, "plane layout");
  auto pabi = to_abi(p);
  if (vpt_render_aov(handle, &pabi, samples, state.width, state.height, &abi, state.hits.data(), (uint64_t*)state.rngs.data(), &state.samples) != VPT_OK)
    throw std::runtime_error{string{"vpt_render_aov: "} + vpt_last_error()};
  auto scale = 1.0f / (float)state.samples;   // get_render
  for (auto image : {&out.normal, &out.albedo, &out.texcoord, &out.depth})
    for (auto& q : image->pixels) q = {q.x * scale, q.y * scale, q.z * scale, q.w * scale};
  return out;
}

pathtrace_sdf_aov_images pathtrace_sdf_aovs(const scene_data& scene, const bvh_scene& bvh, const pathtrace_lights& lights,
    const pathtrace_params& params, int samples, unsigned planes) {
  if (samples < 1) throw std::invalid_argument{"aov samples must be >= 1"};
  if ((planes & sdf_aov_all) == 0) throw std::invalid_argument{"no aov plane asked for"};
  auto handle = (vpt_scene*)nullptr;
  {
    auto lock = std::lock_guard{cache_mutex};
    handle    = single_scene(scene, bvh, lights);
  }
  auto p    = params;
  p.shader  = pathtrace_shader_type::implicit_normal, p.samples = samples;
  auto state = make_state(scene, p);
  auto n     = (size_t)state.width * state.height;
  auto out   = pathtrace_sdf_aov_images{};
  auto abi   = vpt_sdf_aov_planes{};
  auto sums  = [&](unsigned bit, color_image& image) -> void* {
    if (!(planes & bit)) return nullptr;
    image = color_image{state.width, state.height, true, vector<vec4f>(n)};
    return image.pixels.data();
  };
  abi.normal = sums(sdf_aov_normal, out.normal), abi.albedo = sums(sdf_aov_albedo, out.albedo), abi.depth = sums(sdf_aov_depth, out.depth);
  if (planes & sdf_aov_ids) out.ids.resize(n), out.hit.resize(n), abi.ids = out.ids.data(), abi.hit = out.hit.data();
  static_assert(sizeof(vec2i) == 8 && sizeof(vec4f) == 16, "plane layout");
  auto pabi = to_abi(p);
  if (vpt_render_sdf_aov(handle, &pabi, samples, state.width, state.height, &abi, state.hits.data(), (uint64_t*)state.rngs.data(), &state.samples) != VPT_OK)
    throw std::runtime_error{string{"vpt_render_sdf_aov: "} + vpt_last_error()};
  auto scale = 1.0f / (float)state.samples;   // get_render
  for (auto image : {&out.normal, &out.albedo, &out.depth})
    for (auto& q : image->pixels) q = {q.x * scale, q.y * scale, q.z * scale, q.w * scale};
  return out;
}

void pathtrace_release(const scene_data& scene) {
  auto lock = std::lock_guard{cache_mutex};
  device_cache().erase(&scene);
}

void pathtrace_set_devices(const vector<int>& devices) {
  if (devices.empty()) throw std::invalid_argument{"empty device list"};
  auto lock = std::lock_guard{cache_mutex};
  device_list() = devices;
  device_cache().clear();
}

void pathtrace_samples(pathtrace_state& state, const scene_data& scene, const bvh_scene& bvh,
    const pathtrace_lights& lights, const pathtrace_params& params, int count) {
  if (state.samples >= params.samples) return;  // reference cpp:1055
  if (!pathtrace_shader_known(params.shader))
    throw std::runtime_error{"sampler unknown"};  // reference cpp:947-950
  auto handle = (vpt_multi*)nullptr;
  {
    auto  lock  = std::lock_guard{cache_mutex};
    auto& entry = cached_entry(scene, bvh, lights);
    if (!entry.handle) {
      auto flat = flat_scene{};
      flatten_scene(flat, scene, bvh, lights);
      if (vpt_multi_create_curves(&flat.desc, flat.curves_or_null(), device_list().data(), (int)device_list().size(), &entry.handle) != VPT_OK) {
        entry.handle = nullptr;
        device_cache().erase(&scene);
        throw std::runtime_error{string{"vpt_multi_create_curves: "} + vpt_last_error()};
      }
    }
    handle = entry.handle;
  }
  auto abi = to_abi(params);
  static_assert(sizeof(rng_state) == 16 && sizeof(vec4f) == 16, "state layout");
  if (vpt_multi_render(handle, &abi, count, state.width, state.height, (float*)state.image.data(),
          state.hits.data(), (uint64_t*)state.rngs.data(), &state.samples) != VPT_OK)
    throw std::runtime_error{string{"vpt_render: "} + vpt_last_error()};
}

void pathtrace_samples(pathtrace_state& state, const scene_data& scene, const bvh_scene& bvh,
    const pathtrace_lights& lights, const pathtrace_params& params) {
  pathtrace_samples(state, scene, bvh, lights, params, 1);
}

// get_render, yocto_pathtrace.cpp:1105-1116 (throws like check_image :1095-1102)
void get_render(color_image& image, const pathtrace_state& state) {
  if (image.width != state.width || image.height != state.height)
    throw std::invalid_argument{"image should have the same size"};
  if (!image.linear) throw std::invalid_argument{"expected linear image"};
  auto scale = 1.0f / (float)state.samples;
  for (size_t i = 0; i < state.image.size(); i++) {
    auto& p         = state.image[i];
    image.pixels[i] = {p.x * scale, p.y * scale, p.z * scale, p.w * scale};
  }
}
color_image get_render(const pathtrace_state& state) {
  auto image = color_image{state.width, state.height, true, {}};
  image.pixels.resize((size_t)state.width * state.height);
  get_render(image, state);
  return image;
}

pathtrace_adaptive_stats pathtrace_adaptive(pathtrace_state& state, const scene_data& scene, const bvh_scene& bvh,
    const pathtrace_lights& lights, const pathtrace_params& params, const pathtrace_adaptive_params& adaptive) {
  if (!pathtrace_shader_known(params.shader))
    throw std::runtime_error{"sampler unknown"};  // reference cpp:947-950
  auto handle = (vpt_scene*)nullptr;
  {
    auto lock = std::lock_guard{cache_mutex};
    if (device_list().size() != 1) throw std::invalid_argument{"adaptive sampling renders on one GPU"};
    handle = single_scene(scene, bvh, lights);
  }
  auto abi   = to_abi(params);
  auto ad    = vpt_adaptive{adaptive.threshold, adaptive.min_samples, adaptive.step};
  auto stats = pathtrace_adaptive_stats{};
  auto entry = state.hits.empty() ? 0 : state.hits[0];   // equal for all pixels (vpt_render_adaptive checks)
  if (vpt_render_adaptive(handle, &abi, &ad, state.width, state.height, (float*)state.image.data(), state.hits.data(),
          (uint64_t*)state.rngs.data(), &state.samples, &stats.samples) != VPT_OK)
    throw std::runtime_error{string{"vpt_render_adaptive: "} + vpt_last_error()};
  // the pixel that rendered longest was in every round, and each of its rounds but the last took `step` samples
  if (adaptive.step > 0 && state.samples > entry) stats.rounds = (state.samples - entry + adaptive.step - 1) / adaptive.step;
  return stats;
}

void get_render_hits(color_image& image, const pathtrace_state& state) {
  if (image.width != state.width || image.height != state.height)
    throw std::invalid_argument{"image should have the same size"};
  if (!image.linear) throw std::invalid_argument{"expected linear image"};
  for (size_t i = 0; i < state.image.size(); i++) {
    auto& p         = state.image[i];
    auto  h         = state.hits[i];
    auto  scale     = h > 0 ? 1.0f / (float)h : 0.0f;
    image.pixels[i] = h > 0 ? vec4f{p.x * scale, p.y * scale, p.z * scale, p.w * scale} : vec4f{0, 0, 0, 0};
  }
}
color_image get_render_hits(const pathtrace_state& state) {
  auto image = color_image{state.width, state.height, true, {}};
  image.pixels.resize((size_t)state.width * state.height);
  get_render_hits(image, state);
  return image;
}

}  // namespace vpt
