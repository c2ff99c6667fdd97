// vpt_bake_prep.cpp — the host half of vpt_bake_sdf (include/vpt.h): validation of a bake descriptor and the feature normals
// (angle-weighted pseudonormals, Baerentzen & Aanaes 2005) that decide a voxel's sign.  Plain C++ with no device call: the device
// path (csrc/vpt_bake.hip) and the host mirror (host/vpt_bake.cpp) both take their table from here, so one libm computes it.
#include "vpt_bake_prep.h"

#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include "vpt_bake_rule.h"
#include "vpt_error.h"

namespace {

struct d3 {
  double x, y, z;
};
d3     sub(d3 a, d3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
d3     cross(d3 a, d3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double dot(d3 a, d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
d3     unit(d3 a) {
  double l = std::sqrt(dot(a, a));
  return {a.x / l, a.y / l, a.z / l};
}
void add(d3& a, d3 b, double w) { a.x += b.x * w, a.y += b.y * w, a.z += b.z * w; }
double angle(d3 at, d3 p, d3 q) {   // the triangle's angle at `at`
  double c = dot(unit(sub(p, at)), unit(sub(q, at)));
  return std::acos(c < -1 ? -1 : c > 1 ? 1 : c);
}

}  // namespace

int vpt_bake_validate(const vpt_bake_desc* d, const char* entry) {
  REQUIRE(d, "%s: null descriptor", entry);
  REQUIRE(d->num_vertices >= 1 && d->positions, "%s: positions: null or num_vertices %d < 1", entry, d->num_vertices);
  REQUIRE(d->num_triangles >= 1 && d->triangles, "%s: triangles: null or num_triangles %d < 1", entry, d->num_triangles);
  long long voxels = 1;
  for (int k = 0; k < 3; k++) {
    REQUIRE(d->whd[k] >= 1, "%s: whd[%d] = %d < 1", entry, k, d->whd[k]);
    voxels *= d->whd[k];
    REQUIRE(voxels < (1ll << 31), "%s: whd %d x %d x %d: 2^31 voxels or more", entry, d->whd[0], d->whd[1], d->whd[2]);
    REQUIRE(std::isfinite(d->origin[k]), "%s: origin[%d] is not finite", entry, k);
    REQUIRE(std::isfinite(d->step[k]), "%s: step[%d] is not finite", entry, k);
  }
  for (long long i = 0; i < 3ll * d->num_vertices; i++)
    REQUIRE(std::isfinite(d->positions[i]), "%s: positions: vertex %lld has a component that is not finite", entry, i / 3);
  for (long long i = 0; i < 3ll * d->num_triangles; i++)
    REQUIRE(d->triangles[i] >= 0 && d->triangles[i] < d->num_vertices, "%s: triangles: triangle %lld names vertex %d of %d", entry, i / 3,
        d->triangles[i], d->num_vertices);
  return VPT_OK;
}

int vpt_bake_normals(const vpt_bake_desc* d, float* normals, int32_t* kept, const char* entry) {
  if (int rc = vpt_bake_validate(d, entry)) return rc;
  REQUIRE(normals, "%s: null normals", entry);
  const int nv = d->num_vertices, nt = d->num_triangles;
  // one id per distinct position (bit patterns, -0 as +0)
  std::vector<int> weld(nv);
  {
    std::map<std::array<uint32_t, 3>, int> ids;
    for (int v = 0; v < nv; v++) {
      std::array<uint32_t, 3> key;
      for (int c = 0; c < 3; c++) {
        float f = d->positions[3 * v + c];
        if (f == 0.0f) f = 0.0f;
        memcpy(&key[c], &f, 4);
      }
      weld[v] = ids.emplace(key, (int)ids.size()).first->second;
    }
  }
  auto pos_f = [&](int v) { return vpt_bake_f3{d->positions[3 * v], d->positions[3 * v + 1], d->positions[3 * v + 2]}; };
  auto pos_d = [&](int v) { return d3{d->positions[3 * v], d->positions[3 * v + 1], d->positions[3 * v + 2]}; };
  std::vector<char> keep(nt);
  std::vector<d3>   face(nt);
  std::vector<d3>   vertex_sum(nv, d3{0, 0, 0});   // by weld id
  std::map<std::pair<int, int>, d3> edge_sum;      // by the ordered pair of weld ids
  auto edge_key = [&](int u, int v) { return weld[u] < weld[v] ? std::make_pair(weld[u], weld[v]) : std::make_pair(weld[v], weld[u]); };
  int nkept = 0;
  for (int t = 0; t < nt; t++) {
    const int32_t* tri = d->triangles + 3 * t;
    vpt_bake_f3    cf  = vpt_bake_cross(pos_f(tri[0]), pos_f(tri[1]), pos_f(tri[2]));
    keep[t] = !(cf.x == 0.0f && cf.y == 0.0f && cf.z == 0.0f);
    if (!keep[t]) continue;
    nkept++;
    d3 a = pos_d(tri[0]), b = pos_d(tri[1]), c = pos_d(tri[2]);
    d3 n = cross(sub(b, a), sub(c, a));
    if (n.x == 0 && n.y == 0 && n.z == 0) n = {cf.x, cf.y, cf.z};   // float32 rounding alone kept it: its direction is that rounding's
    face[t] = unit(n);
    add(vertex_sum[weld[tri[0]]], face[t], angle(a, b, c));
    add(vertex_sum[weld[tri[1]]], face[t], angle(b, c, a));
    add(vertex_sum[weld[tri[2]]], face[t], angle(c, a, b));
    for (int e = 0; e < 3; e++) add(edge_sum.emplace(edge_key(tri[e], tri[(e + 1) % 3]), d3{0, 0, 0}).first->second, face[t], 1.0);
  }
  REQUIRE(nkept > 0, "%s: triangles: every triangle has a zero cross product, nothing to bake", entry);
  for (int t = 0; t < nt; t++) {
    float* o = normals + 21 * (size_t)t;
    if (kept) kept[t] = keep[t];
    if (!keep[t]) {
      for (int k = 0; k < 21; k++) o[k] = 0.0f;
      continue;
    }
    const int32_t* tri = d->triangles + 3 * t;
    auto put = [&](int slot, d3 n) { o[3 * slot] = (float)n.x, o[3 * slot + 1] = (float)n.y, o[3 * slot + 2] = (float)n.z; };
    put(VPT_BAKE_FACE, face[t]);
    put(VPT_BAKE_EDGE_AB, edge_sum[edge_key(tri[0], tri[1])]);
    put(VPT_BAKE_EDGE_BC, edge_sum[edge_key(tri[1], tri[2])]);
    put(VPT_BAKE_EDGE_CA, edge_sum[edge_key(tri[2], tri[0])]);
    put(VPT_BAKE_VERTEX_A, vertex_sum[weld[tri[0]]]);
    put(VPT_BAKE_VERTEX_B, vertex_sum[weld[tri[1]]]);
    put(VPT_BAKE_VERTEX_C, vertex_sum[weld[tri[2]]]);
  }
  return VPT_OK;
}

extern "C" int vpt_bake_feature_normals(const vpt_bake_desc* desc, float* normals, int32_t* kept) {
  return vpt_bake_normals(desc, normals, kept, "vpt_bake_feature_normals");
}
