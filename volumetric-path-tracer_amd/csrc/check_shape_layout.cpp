// check_shape_layout.cpp — a stand-alone program over the host halves of vpt_scene_update_shapes, for a sanitizer build on a machine
// without a device (make check-shape-layout): the new list, the renumbering, the pool offsets and the survivor runs of
// vpt_shape_layout.h on edits of the kinds the tests use, against a plain restatement; and prep_check_shape_elements /
// prep_quad_nodes_and_stacks of vpt_scene_prep.cpp in their partial forms on small trees.  Exit status 0: every check held.
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "vpt_scene_prep.h"
#include "vpt_shape_layout.h"

int vpt_set_error(int code, const char*, ...) { return code; }   // (vpt_capi.hip's, which this program does not link)

static int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) printf("line %d: %s does not hold\n", __LINE__, #cond), failures++; \
  } while (0)

// a chain of `leaves` leaves: node 0 internal, its children a leaf and the next internal node (the form of a deep shape BVH)
static std::vector<vpt_bvh_node> chain(int leaves) {
  std::vector<vpt_bvh_node> nodes((size_t)(2 * leaves - 1));
  for (int i = 0; i < leaves - 1; i++) {
    vpt_bvh_node& n = nodes[(size_t)(2 * i)];
    n = {}, n.internal = 1, n.start = 2 * i + 1;
    for (int c = 0; c < 3; c++) n.bbox_min[c] = -1, n.bbox_max[c] = 1;
    vpt_bvh_node& leaf = nodes[(size_t)(2 * i + 1)];
    leaf = n, leaf.internal = 0, leaf.start = i, leaf.num = 1;
  }
  vpt_bvh_node& last = nodes.back();
  last = {}, last.start = leaves - 1, last.num = 1;
  if (leaves > 1) nodes[(size_t)(2 * leaves - 3)].start = leaves - 2;
  return nodes;
}

int main() {
  // ---- the list, the renumbering, the runs ----------------------------------------------------------------------------------
  struct edit { int n_old; std::vector<int> remove, set; int add; };
  const edit edits[] = {{7, {}, {0}, 0}, {7, {0}, {}, 0}, {7, {}, {}, 2}, {7, {1}, {4}, 2}, {9, {7, 8}, {}, 0}, {4, {}, {}, 1}, {5, {4}, {}, 0},
      {7, {2, 3, 4}, {0, 6}, 0}, {1, {0}, {}, 0}, {0, {}, {}, 3}, {300, {17, 250, 251}, {16, 18, 299}, 5}};
  for (const edit& e : edits) {
    std::vector<shape_slot> list;
    std::vector<int>        new_of_old;
    shape_list_of_edit(e.n_old, e.remove.data(), (int)e.remove.size(), e.set.data(), (int)e.set.size(), e.add, list, new_of_old);
    CHECK((int)list.size() == e.n_old - (int)e.remove.size() + e.add && (int)new_of_old.size() == e.n_old);
    int next = 0;
    for (int i = 0; i < e.n_old; i++) {
      bool gone = false, is_set = false;
      for (int r : e.remove) gone = gone || r == i;
      for (int s : e.set) is_set = is_set || s == i;
      CHECK(new_of_old[(size_t)i] == (gone ? -1 : next));
      if (gone) continue;
      CHECK(list[(size_t)next].old_id == i && (list[(size_t)next].payload >= 0) == is_set);
      next++;
    }
    for (int k = 0; k < e.add; k++) CHECK(list[(size_t)(next + k)].old_id == -1 && list[(size_t)(next + k)].payload == (int)e.set.size() + k);
    // pool offsets of lengths that depend on the shape, and the runs: together they cover every untouched survivor once, contiguously
    std::vector<long long> was((size_t)e.n_old), now(list.size());
    for (int i = 0; i < e.n_old; i++) was[(size_t)i] = (i * 37) % 11;
    for (size_t j = 0; j < list.size(); j++) now[j] = list[j].payload >= 0 ? 5 : list[j].old_id >= 0 ? was[(size_t)list[j].old_id] : 0;
    const std::vector<long long> old_at = pool_offsets(was), new_at = pool_offsets(now);
    CHECK(old_at.size() == was.size() + 1 && new_at.size() == now.size() + 1 && old_at[0] == 0 && new_at[0] == 0);
    std::vector<char> covered(list.size(), 0);
    for (const shape_run& run : survivor_runs(list)) {
      CHECK(run.count > 0 && run.first_new + run.count <= (int)list.size() && run.first_old + run.count <= e.n_old);
      CHECK(old_at[(size_t)(run.first_old + run.count)] - old_at[(size_t)run.first_old] == new_at[(size_t)(run.first_new + run.count)] - new_at[(size_t)run.first_new]);
      for (int k = 0; k < run.count; k++) {
        CHECK(list[(size_t)(run.first_new + k)].old_id == run.first_old + k && list[(size_t)(run.first_new + k)].payload < 0 && !covered[(size_t)(run.first_new + k)]);
        covered[(size_t)(run.first_new + k)] = 1;
      }
    }
    for (size_t j = 0; j < list.size(); j++) CHECK((covered[j] != 0) == (list[j].old_id >= 0 && list[j].payload < 0));
  }
  // ---- the rules for the elements of one shape -----------------------------------------------------------------------------------
  const int32_t tri[3] = {0, 1, 2}, bad[3] = {0, 1, 3}, quad[4] = {0, 1, 2, 2}, line[2] = {0, 1}, point[1] = {2};
  CHECK(prep_check_shape_elements(0, 3, tri, 1, nullptr, 0, nullptr, 0, nullptr, 0) == VPT_OK);
  CHECK(prep_check_shape_elements(0, 3, bad, 1, nullptr, 0, nullptr, 0, nullptr, 0) == VPT_ERR_INVALID_ARG);
  CHECK(prep_check_shape_elements(0, 3, tri, 1, quad, 1, nullptr, 0, nullptr, 0) == VPT_ERR_INVALID_ARG);
  CHECK(prep_check_shape_elements(0, 3, tri, 1, nullptr, 0, nullptr, 0, line, 1) == VPT_ERR_UNSUPPORTED);
  CHECK(prep_check_shape_elements(0, 3, nullptr, 0, nullptr, 0, point, 1, line, 1) == VPT_ERR_UNSUPPORTED);
  CHECK(prep_check_shape_elements(0, 3, nullptr, 0, nullptr, 0, point, 1, nullptr, 0) == VPT_OK);
  CHECK(prep_check_shape_elements(0, 2, nullptr, 0, nullptr, 0, point, 1, nullptr, 0) == VPT_ERR_INVALID_ARG);
  CHECK(prep_check_shape_elements(0, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0) == VPT_OK);
  // ---- the traversal limits from some new trees and what is kept of the others -----------------------------------------------------
  const std::vector<vpt_bvh_node> deep = chain(40), flat = chain(3), scene = chain(5);
  std::vector<vpt_bvh_node> pool(deep);
  pool.insert(pool.end(), flat.begin(), flat.end());
  vpt_shape shapes[2] = {};
  shapes[0].num_bvh_nodes = (int)deep.size(), shapes[1].bvh_node_offset = (int)deep.size(), shapes[1].num_bvh_nodes = (int)flat.size();
  vpt_scene_desc desc = {};
  desc.num_shapes = 2, desc.shapes = shapes, desc.shape_bvh_nodes = pool.data(), desc.num_shape_bvh_nodes = (int64_t)pool.size();
  desc.scene_bvh_nodes = scene.data(), desc.num_scene_bvh_nodes = (int)scene.size();
  scene_tables whole;
  whole.shapes.assign(2, DShape{});
  whole.shapes[0].num_nodes = (int)deep.size(), whole.shapes[1].num_nodes = (int)flat.size();
  CHECK(prep_quad_nodes_and_stacks(desc, whole) == VPT_OK);
  CHECK(whole.shape_depths.size() == 2 && whole.shape_depths[0] == 39 && whole.shape_depths[1] == 2 && whole.shape_depth == 39 && whole.scene_depth == 4);
  CHECK(whole.shape_wnodes == 8 * (size_t)(whole.shape_quads[0] + whole.shape_quads[1]) && whole.wnodes.size() == whole.scene_wnodes + whole.shape_wnodes);
  // shape 1 made anew, shape 0 and the scene BVH kept: the same limits and offsets, its quad nodes alone
  vpt_shape one[2] = {};
  one[1].num_bvh_nodes = (int)flat.size();
  vpt_scene_desc part = {};
  part.num_shapes = 2, part.shapes = one, part.shape_bvh_nodes = flat.data(), part.num_shape_bvh_nodes = (int64_t)flat.size();
  scene_tables some;
  some.shapes = whole.shapes, some.shape_depths = whole.shape_depths, some.shape_need4s = whole.shape_need4s, some.shape_quads = whole.shape_quads;
  some.shape_depths[1] = some.shape_need4s[1] = some.shape_quads[1] = -7;   // (to be made)
  some.scene_depth = whole.scene_depth, some.scene_need4 = whole.scene_need4, some.scene_wnodes = whole.scene_wnodes;
  const char made[2] = {0, 1};
  CHECK(prep_quad_nodes_and_stacks(part, some, false, made, true) == VPT_OK);
  CHECK(some.stack_cap == whole.stack_cap && some.stack_lds4 == whole.stack_lds4 && some.stack_spill4 == whole.stack_spill4);
  CHECK(some.shape_depths == whole.shape_depths && some.shape_need4s == whole.shape_need4s && some.shape_quads == whole.shape_quads);
  CHECK(some.shapes[1].wnode_offset == whole.shapes[1].wnode_offset && some.shapes[1].root_ref == whole.shapes[1].root_ref && some.shape_wnodes == whole.shape_wnodes);
  CHECK(some.wnodes.size() == 8 * (size_t)whole.shape_quads[1]);
  // the deep shape gone: the limits of the scene that is left
  vpt_shape left[1] = {};
  scene_tables fewer;
  fewer.shapes.assign(1, whole.shapes[1]);
  fewer.shape_depths = {whole.shape_depths[1]}, fewer.shape_need4s = {whole.shape_need4s[1]}, fewer.shape_quads = {whole.shape_quads[1]};
  fewer.scene_depth = whole.scene_depth, fewer.scene_need4 = whole.scene_need4, fewer.scene_wnodes = whole.scene_wnodes;
  vpt_scene_desc none = {};
  none.num_shapes = 1, none.shapes = left;
  const char kept[1] = {0};
  CHECK(prep_quad_nodes_and_stacks(none, fewer, false, kept, true) == VPT_OK);
  CHECK(fewer.shape_depth == 2 && fewer.stack_cap < whole.stack_cap && fewer.shapes[0].wnode_offset == 0 && fewer.wnodes.empty());
  printf(failures ? "%d checks failed\n" : "every check held\n", failures);
  return failures ? 1 : 0;
}
