// check_visit_ranks.cpp — a stand-alone program over the visit-rank tables of the quad nodes (vpt_device.h: words 28 .. 31 of a node),
// for a sanitizer build on a machine without a device (make check-visit-ranks).  prep_quad_nodes_and_stacks of vpt_scene_prep.cpp makes
// the quad nodes of small binary trees; this program walks the binary tree beside them and checks, for every quad node, all 8 octants of
// a ray's direction and all 4 slots: the two table bits against the rank formula evaluated from the binary nodes' axes, the ranks of the
// present slots against the order in which the reference's binary traversal visits them, the low 16 bits of word 28 against the axes
// word the other readers of the node expect, and the low 16 bits of words 29 .. 31 against zero.  Exit status 0: every check held.
#include <cstdio>
#include <cstring>
#include <vector>

#include "vpt_scene_prep.h"

int vpt_set_error(int code, const char*, ...) { return code; }   // (vpt_capi.hip's, which this program does not link)

static int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) printf("line %d: %s does not hold\n", __LINE__, #cond), failures++; \
  } while (0)

// a binary BVH from its preorder: 'L' a leaf of one primitive, '0' '1' '2' an internal node with that split axis (its two children
// are neighbours in the array, as the builders leave them)
struct tree {
  std::vector<vpt_bvh_node> nodes;
  int leaves = 0;
};
static void grow(tree& t, size_t i, const char*& s) {
  const char c = *s++;
  vpt_bvh_node n = {};
  for (int k = 0; k < 3; k++) n.bbox_min[k] = -1.0f - (float)i, n.bbox_max[k] = 1.0f + (float)i;
  if (c == 'L') {
    n.start = t.leaves++, n.num = 1;
    t.nodes[i] = n;
    return;
  }
  const size_t first = t.nodes.size();
  n.internal = 1, n.axis = c - '0', n.start = (int)first;
  t.nodes[i] = n;
  t.nodes.resize(first + 2);
  grow(t, first, s), grow(t, first + 1, s);
}
static tree tree_of(const char* preorder) {
  tree t;
  t.nodes.resize(1);
  grow(t, 0, preorder);
  return t;
}

// the order in which the reference's traversal reaches the (up to four) grandchildren of binary node i for a ray of octant s (bit a
// set: negative along axis a): of two children the second one first when the ray is negative along the node's axis
static std::vector<int> visit_order(const std::vector<vpt_bvh_node>& nodes, int i, int s) {
  std::vector<int> order;
  for (int a = 0; a < 2; a++) {
    const int c = nodes[(size_t)i].start + (((s >> nodes[(size_t)i].axis) & 1) ? 1 - a : a);
    if (!nodes[(size_t)c].internal) order.push_back(c);
    else
      for (int b = 0; b < 2; b++) order.push_back(nodes[(size_t)c].start + (((s >> nodes[(size_t)c].axis) & 1) ? 1 - b : b));
  }
  return order;
}

static int visited = 0;
static void walk(const std::vector<vpt_bvh_node>& nodes, const std::vector<float4>& quads, int qn, int i) {
  visited++;
  CHECK(qn >= 0 && 8 * (size_t)qn + 8 <= quads.size());
  if (qn < 0 || 8 * (size_t)qn + 8 > quads.size()) return;
  int ref[4];
  unsigned word[4];
  memcpy(ref, &quads[8 * (size_t)qn + 6], 16), memcpy(word, &quads[8 * (size_t)qn + 7], 16);
  // the binary nodes behind the slots, and the axes as the traversal kernels read them (a leaf child counts as axis 0)
  int slot[4], axes[3] = {nodes[(size_t)i].axis, 0, 0};
  for (int side = 0; side < 2; side++) {
    const int c = nodes[(size_t)i].start + side;
    if (nodes[(size_t)c].internal) slot[2 * side] = nodes[(size_t)c].start, slot[2 * side + 1] = nodes[(size_t)c].start + 1, axes[1 + side] = nodes[(size_t)c].axis;
    else slot[2 * side] = c, slot[2 * side + 1] = -1;
  }
  CHECK((word[0] & 0xffffu) == (unsigned)(axes[0] | (axes[1] << 2) | (axes[2] << 4)));   // (so the low 6 bits are the axes word the own form masks)
  for (int j = 1; j < 4; j++) CHECK((word[j] & 0xffffu) == 0);
  for (int s = 0; s < 8; s++) {
    int rank_of[4];
    for (int j = 0; j < 4; j++) {
      const int gn = (s >> axes[0]) & 1, g0 = (s >> axes[1]) & 1, g1 = (s >> axes[2]) & 1, grp = j >> 1;
      const int k = ((grp ^ gn) << 1) | ((j & 1) ^ (grp ? g1 : g0));
      rank_of[j] = (int)((word[j] >> (16 + 2 * s)) & 3u);
      CHECK(rank_of[j] == k);
    }
    // the ranks are a permutation, and the present slots in rank order are the reference's visit order
    CHECK(((1 << rank_of[0]) | (1 << rank_of[1]) | (1 << rank_of[2]) | (1 << rank_of[3])) == 15);
    std::vector<int> by_rank;
    for (int k = 0; k < 4; k++)
      for (int j = 0; j < 4; j++)
        if (rank_of[j] == k && slot[j] >= 0) by_rank.push_back(slot[j]);
    CHECK(by_rank == visit_order(nodes, i, s));
  }
  for (int j = 0; j < 4; j++) {
    if (slot[j] < 0) CHECK(ref[j] == -2147483647 - 1);
    else if (!nodes[(size_t)slot[j]].internal) CHECK(ref[j] < 0 && ref[j] != -2147483647 - 1);
    else {
      CHECK(ref[j] > qn);
      if (ref[j] > qn) walk(nodes, quads, ref[j], slot[j]);
    }
  }
}

int main() {
  // a root with a leaf child and an empty slot; two quad levels (the lower one with a leaf child of its own); axes that differ between
  // the node and both children, in two arrangements
  const char* const trees[] = {"0L1LL", "0120LLLL2LL", "20LL1LL", "12LL0LL", "1L0LL", "22LL2LL"};
  for (const char* preorder : trees) {
    const tree t = tree_of(preorder);
    vpt_scene_desc desc = {};
    desc.scene_bvh_nodes = t.nodes.data(), desc.num_scene_bvh_nodes = (int)t.nodes.size();
    scene_tables out;
    CHECK(prep_quad_nodes_and_stacks(desc, out) == VPT_OK);
    CHECK(out.scene_wnodes == out.wnodes.size() && !out.wnodes.empty() && out.d.scene_root_ref == 0);
    if (out.wnodes.empty()) continue;
    visited = 0;
    walk(t.nodes, out.wnodes, 0, 0);
    CHECK(8 * (size_t)visited == out.wnodes.size());
  }
  printf(failures ? "%d checks failed\n" : "every check held\n", failures);
  return failures ? 1 : 0;
}
