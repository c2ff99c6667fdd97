// vpt_bake.cpp — baking a mesh into a signed-distance grid on the CPU: the rule of include/vpt.h (vpt_bake_sdf) through the same
// header the HIP kernel compiles (csrc/vpt_bake_rule.h, -ffp-contract=off), over every voxel and every kept triangle in the caller's
// order - the statement the kernel's BVH walk is held to bit for bit; the same through the GPU (vpt_bake_sdf); and the glue between
// a mesh and the renderer's lookup: fit_volume, the quad split, save_volume.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>

#include "vpt_bake_rule.h"
#include "vpt_host.h"

namespace vpt {

namespace {
vpt_bake_desc make_desc(const vector<vec3f>& positions, const vector<vec3i>& triangles, const vec3i& whd, const vec3f& origin, const vec3f& step) {
  auto desc = vpt_bake_desc{};
  desc.num_vertices = (int32_t)positions.size(), desc.positions = positions.empty() ? nullptr : &positions.data()->x;
  desc.num_triangles = (int32_t)triangles.size(), desc.triangles = triangles.empty() ? nullptr : &triangles.data()->x;
  desc.whd[0] = whd.x, desc.whd[1] = whd.y, desc.whd[2] = whd.z;
  desc.origin[0] = origin.x, desc.origin[1] = origin.y, desc.origin[2] = origin.z;
  desc.step[0] = step.x, desc.step[1] = step.y, desc.step[2] = step.z;
  return desc;
}
}  // namespace

void bake_sdf(vector<float>& voxels, const vector<vec3f>& positions, const vector<vec3i>& triangles, const vec3i& whd, const vec3f& origin,
    const vec3f& step, vpt_bake_stats* stats, int threads) {
  if (threads < 1 || threads > 16) throw std::invalid_argument{"bake_sdf: threads outside 1..16"};
  auto desc    = make_desc(positions, triangles, whd, origin, step);
  auto normals = vector<float>(21 * triangles.size());
  auto keep    = vector<int32_t>(triangles.size());
  // validation and the feature normals are the C-ABI's own (plain C++ in libvpt_hip.so: no device call)
  if (vpt_bake_feature_normals(&desc, normals.empty() ? nullptr : normals.data(), keep.data()) != VPT_OK)
    throw std::invalid_argument{string{"bake_sdf: "} + vpt_last_error()};
  auto records = vector<vpt_bake_record>{};
  for (auto t = 0; t < desc.num_triangles; t++)
    if (keep[t]) records.push_back(vpt_bake_make_record(desc.positions, desc.triangles, normals.data(), t));
  if (stats) *stats = vpt_bake_stats{}, stats->dropped_triangles = desc.num_triangles - (int32_t)records.size();
  auto rows = (size_t)whd.y * whd.z;
  auto out  = vector<float>((size_t)whd.x * rows);
  auto work = [&](size_t row_begin, size_t row_end) {
    for (auto row = row_begin; row < row_end; row++) {
      auto y = (int)(row % whd.y), z = (int)(row / whd.y);
      for (auto x = 0; x < whd.x; x++) {
        auto p = vpt_bake_f3{vpt_bake_sample(desc.origin[0], desc.step[0], x), vpt_bake_sample(desc.origin[1], desc.step[1], y),
            vpt_bake_sample(desc.origin[2], desc.step[2], z)};
        auto best = vpt_bake_none();
        for (auto slot = 0; slot < (int)records.size(); slot++) vpt_bake_offer(best, vpt_bake_distance2(p, records[slot]), records[slot].index, slot);
        out[(size_t)x + row * whd.x] = best.slot < 0 ? vpt_bake_no_winner() : vpt_bake_value(p, records[best.slot]);
      }
    }
  };
  auto nthreads = (size_t)std::min<size_t>((size_t)threads, rows);
  if (nthreads <= 1) {
    work(0, rows);
  } else {
    auto pool = vector<std::thread>{};
    for (size_t t = 0; t < nthreads; t++) pool.emplace_back(work, rows * t / nthreads, rows * (t + 1) / nthreads);
    for (auto& th : pool) th.join();
  }
  voxels = std::move(out);
}

void bake_sdf_device(vector<float>& voxels, const vector<vec3f>& positions, const vector<vec3i>& triangles, const vec3i& whd,
    const vec3f& origin, const vec3f& step, int device, vpt_bake_stats* stats) {
  auto desc = make_desc(positions, triangles, whd, origin, step);
  auto n    = (int64_t)whd.x * whd.y * whd.z;
  auto out  = vector<float>(whd.x >= 1 && whd.y >= 1 && whd.z >= 1 && n < (1ll << 31) ? (size_t)n : 1);   // a bad size is the C-ABI's to refuse
  if (vpt_bake_sdf(device, &desc, out.data(), stats) != VPT_OK) throw std::runtime_error{string{"vpt_bake_sdf: "} + vpt_last_error()};
  voxels = std::move(out);
}

volume_fit fit_volume(const vec3f& bmin, const vec3f& bmax, const vec3i& whd, int padding) {
  if (padding < 0) throw std::invalid_argument{"fit_volume: padding < 0"};
  const float lo[3] = {bmin.x, bmin.y, bmin.z}, hi[3] = {bmax.x, bmax.y, bmax.z};
  const int   n[3]  = {whd.x, whd.y, whd.z};
  auto extent_max = 0.0, res_d = 0.0;
  for (auto a = 0; a < 3; a++) {
    if (n[a] < 2 * padding + 3) throw std::invalid_argument{"fit_volume: whd below 2 * padding + 3 on an axis"};
    if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || hi[a] < lo[a]) throw std::invalid_argument{"fit_volume: bounds are empty or not finite"};
    auto extent = (double)hi[a] - (double)lo[a];
    extent_max  = std::max(extent_max, extent);
    // (n - 1 - 2 padding) steps of res * n / (n - 1) cover the extent
    res_d = std::max(res_d, extent * (n[a] - 1) / ((double)n[a] * (n[a] - 1 - 2 * padding)));
  }
  if (!(extent_max > 0)) throw std::invalid_argument{"fit_volume: bounds have no extent"};
  auto fit     = volume_fit{};
  fit.res      = (float)res_d;
  auto step_of = [&](int a) { return (fit.res * (float)n[a]) / (float)(n[a] - 1); };
  auto covers  = [&]() {
    for (auto a = 0; a < 3; a++)
      if ((double)step_of(a) * (n[a] - 1 - 2 * padding) < (double)hi[a] - (double)lo[a]) return false;
    return true;
  };
  while (!covers()) fit.res = std::nextafterf(fit.res, INFINITY);   // the rounding of res or of a step fell short: a few ulps at most
  float step[3], origin[3];
  for (auto a = 0; a < 3; a++) {
    step[a]   = step_of(a);
    origin[a] = (float)(((double)lo[a] + (double)hi[a]) / 2 - (double)step[a] * (n[a] - 1) / 2);
  }
  fit.step             = {step[0], step[1], step[2]};
  fit.origin           = {origin[0], origin[1], origin[2]};
  fit.instance.frame.o = {-origin[0], -origin[1], -origin[2]};
  fit.instance.scalef  = 1;
  return fit;
}

vector<vec3i> bake_triangles(const shape_data& shape) {
  auto triangles = shape.triangles;
  for (auto& q : shape.quads) {
    if (q.z == q.w) {
      triangles.push_back({q.x, q.y, q.z});
    } else {
      triangles.push_back({q.x, q.y, q.w});
      triangles.push_back({q.z, q.w, q.y});
    }
  }
  return triangles;
}

baked_volume bake_volume(const vector<vec3f>& positions, const vector<vec3i>& triangles, const vec3i& whd, int padding, int device) {
  if (positions.empty() || triangles.empty()) throw std::invalid_argument{"bake_volume: the mesh has no triangles"};
  auto bmin = vec3f{INFINITY, INFINITY, INFINITY}, bmax = vec3f{-INFINITY, -INFINITY, -INFINITY};
  for (auto& t : triangles) {   // the bounds of what the triangles name (an index out of range is the bake's to refuse)
    for (auto v : {t.x, t.y, t.z}) {
      if (v < 0 || v >= (int)positions.size()) continue;
      auto& p = positions[v];
      bmin = {std::min(bmin.x, p.x), std::min(bmin.y, p.y), std::min(bmin.z, p.z)};
      bmax = {std::max(bmax.x, p.x), std::max(bmax.y, p.y), std::max(bmax.z, p.z)};
    }
  }
  auto fit   = fit_volume(bmin, bmax, whd, padding);
  auto baked = baked_volume{};
  if (device < 0) bake_sdf(baked.volume.vol, positions, triangles, whd, fit.origin, fit.step, &baked.stats);
  else bake_sdf_device(baked.volume.vol, positions, triangles, whd, fit.origin, fit.step, device, &baked.stats);
  baked.volume.whd = whd, baked.volume.res = fit.res;
  baked.instance = fit.instance;
  return baked;
}

bool save_volume(const string& filename, const volume_data& vol, string& error) {
  auto n = (size_t)vol.whd.x * vol.whd.y * vol.whd.z;
  if (vol.whd.x <= 0 || vol.whd.y <= 0 || vol.whd.z <= 0 || vol.vol.size() < n) {
    error = filename + ": volume has no voxels";
    return false;
  }
  auto fs = fopen(filename.c_str(), "wb");
  if (!fs) {
    error = filename + ": write error";
    return false;
  }
  const int32_t whd[3]       = {vol.whd.x, vol.whd.y, vol.whd.z};
  const float   identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  auto ok = fwrite(whd, 4, 3, fs) == 3 && fwrite(&vol.res, 4, 1, fs) == 1 && fwrite(identity, 4, 16, fs) == 16 && fwrite(vol.vol.data(), 4, n, fs) == n;
  ok      = (fclose(fs) == 0) && ok;
  if (!ok) error = filename + ": write error";
  return ok;
}

}  // namespace vpt
