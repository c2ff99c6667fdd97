// check_bvh_sah.cpp — a stand-alone program over the host mirror's BVH build at both qualities (vpt_host.h: build_bvh_host), for a
// sanitizer build on a machine without a device (make check-bvh-sah): the synthetic boxes of the SAH tests' kinds - random sizes around
// a leaf, a wave and a block, identical boxes, collinear centres with ties, a lattice of repeated centres, radii that overflow the
// areas, and boxes with NaN and infinite coordinates - and on every tree the properties a build must keep whatever the split rule:
// the primitive order is a permutation, the leaves tile it in order with at most four primitives each, every node but the root has one
// parent, and the count is odd and at most 2 n - 1.  Exit status 0: every check held.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "vpt_host.h"

using namespace vpt;

static int failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) printf("line %d: %s does not hold\n", __LINE__, #cond), failures++; \
  } while (0)

using boxes = std::vector<float>;   // {min.xyz, max.xyz} per box

static boxes points(const std::vector<float>& xyz, float r) {
  boxes b;
  for (size_t i = 0; i + 2 < xyz.size(); i += 3)
    for (int s = -1; s <= 1; s += 2)
      for (int c = 0; c < 3; c++) b.push_back(xyz[i + c] + s * r);
  return b;
}
static boxes random_points(int n, unsigned seed, float r) {
  std::mt19937                          gen(seed);
  std::uniform_real_distribution<float> u(-1, 1);
  std::vector<float>                    xyz((size_t)n * 3);
  for (auto& x : xyz) x = u(gen);
  return points(xyz, r);
}

static void check_tree(const boxes& b, int quality) {
  const int n   = (int)(b.size() / 6);
  auto      bvh = build_bvh_host(b.data(), n, quality);
  const int count = (int)bvh.nodes.size();
  CHECK(count >= 1 && count % 2 == 1 && count <= (n > 0 ? 2 * n - 1 : 1));
  CHECK((int)bvh.primitives.size() == n);
  std::vector<char> seen((size_t)n, 0);
  for (auto p : bvh.primitives) {
    CHECK(p >= 0 && p < n && !seen[(size_t)p]);
    if (p >= 0 && p < n) seen[(size_t)p] = 1;
  }
  std::vector<int>  parents((size_t)count, 0);
  std::vector<char> covered((size_t)n, 0);
  for (int i = 0; i < count; i++) {
    const auto& node = bvh.nodes[(size_t)i];
    if (node.internal) {
      CHECK(node.num == 2 && node.start > i && node.start + 1 < count && node.axis >= 0 && node.axis < 3);
      if (node.start > 0 && node.start + 1 < count) parents[(size_t)node.start]++, parents[(size_t)node.start + 1]++;
    } else {
      CHECK(node.num >= 0 && node.num <= 4 && node.start >= 0 && node.start + node.num <= n);
      for (int k = 0; k < node.num && node.start + k < n; k++) {
        CHECK(!covered[(size_t)(node.start + k)]);
        covered[(size_t)(node.start + k)] = 1;
      }
    }
  }
  for (int i = 1; i < count; i++) CHECK(parents[(size_t)i] == 1);
  for (int i = 0; i < n; i++) CHECK(covered[(size_t)i]);
}

int main() {
  std::vector<boxes> cases;
  for (int n : {0, 1, 4, 5, 65, 257, 1000}) cases.push_back(random_points(n, 100u + (unsigned)n, 0.05f));
  cases.push_back(points(std::vector<float>(300, 0.25f), 0.125f));   // 100 identical boxes
  {
    std::vector<float> line, lattice, far;
    for (int i = 0; i < 90; i++) line.insert(line.end(), {0.5f * (float)(i / 3), 0.0f, 0.0f});
    for (int r = 0; r < 4; r++)
      for (int x = 0; x < 4; x++)
        for (int y = 0; y < 4; y++)
          for (int z = 0; z < 2; z++) lattice.insert(lattice.end(), {(float)x, (float)y, (float)z});
    for (int i = 0; i < 64; i++) far.insert(far.end(), {(float)(i - 20) * 1e9f, 0.0f, 0.0f});
    cases.push_back(points(line, 0.25f)), cases.push_back(points(lattice, 0.5f)), cases.push_back(points(far, 1e14f));
  }
  {
    auto odd = random_points(40, 9, 0.05f);   // coordinates no build should meet: the search must still end and index nothing out of range
    odd[6 * 3] = std::numeric_limits<float>::quiet_NaN(), odd[6 * 7 + 4] = std::numeric_limits<float>::infinity();
    odd[6 * 11 + 1] = -std::numeric_limits<float>::infinity(), odd[6 * 20 + 5] = std::numeric_limits<float>::max();
    cases.push_back(odd);
  }
  for (const auto& b : cases)
    for (int quality : {VPT_BVH_MIDDLE, VPT_BVH_SAH}) check_tree(b, quality);
  // quality 0 is the build without the argument; an unknown quality throws and builds nothing
  {
    const auto b = random_points(257, 3, 0.05f);
    auto       x = build_bvh_host(b.data(), 257), y = build_bvh_host(b.data(), 257, VPT_BVH_MIDDLE);
    CHECK(x.primitives == y.primitives && x.nodes.size() == y.nodes.size());
    auto thrown = false;
    try {
      build_bvh_host(b.data(), 257, 2);
    } catch (const std::invalid_argument&) {
      thrown = true;
    }
    CHECK(thrown);
  }
  printf("check_bvh_sah: %zu cases at two qualities, %d failures\n", cases.size(), failures);
  return failures ? 1 : 0;
}
