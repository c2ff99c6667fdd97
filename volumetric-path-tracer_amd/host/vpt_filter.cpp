// vpt_filter.cpp — filtering a voxel grid on the CPU: the rule of include/vpt.h (vpt_scene_filter_volumes) through the same header as
// the kernels (csrc/vpt_filter_rule.h), one op after another over the entry's region - the statement the kernels are held to bit for
// bit; and the Gaussian weights of a BLUR op from a sigma.
#include <algorithm>
#include <cstdio>

#include "vpt_filter_rule.h"
#include "vpt_host.h"

namespace vpt {

namespace {

struct box3 {
  int lo[3], hi[3];   // [lo, hi) per axis
  int    size(int k) const { return hi[k] - lo[k]; }
  size_t count() const { return (size_t)size(0) * (size_t)size(1) * (size_t)size(2); }
  size_t at(int x, int y, int z) const { return (size_t)(x - lo[0]) + (size_t)(y - lo[1]) * (size_t)size(0) + (size_t)(z - lo[2]) * (size_t)size(0) * (size_t)size(1); }
};

// One pass along `axis` over the nodes of `to`, read from `src` (the nodes of `from`, which holds every clamped neighbour)
template <int R>
void blur_pass(const float* w, int axis, const int32_t whd[3], const float* src, const box3& from, float* dst, const box3& to) {
  float line[2 * R + 1];
  for (auto z = to.lo[2]; z < to.hi[2]; z++)
    for (auto y = to.lo[1]; y < to.hi[1]; y++)
      for (auto x = to.lo[0]; x < to.hi[0]; x++) {
        for (auto i = -R; i <= R; i++) {
          int p[3] = {x, y, z};
          p[axis]  = vpt_filter_clamp(p[axis] + i, whd[axis]);
          line[i + R] = src[from.at(p[0], p[1], p[2])];
        }
        dst[to.at(x, y, z)] = vpt_filter_blur_taps<R>(w, line, R);
      }
}

// x, then y, then z: the x pass over the region widened by R along y and z (inside the volume), the y pass over it widened along z
template <int R>
void blur_region(float* voxels, const int32_t whd[3], const vpt_filter_entry& e, const float* w) {
  const auto whole  = box3{{0, 0, 0}, {whd[0], whd[1], whd[2]}};
  auto       region = box3{};
  for (auto k = 0; k < 3; k++) region.lo[k] = e.region_lo[k], region.hi[k] = e.region_lo[k] + e.region_whd[k];
  auto wide = [&](box3 b, int axis) {
    b.lo[axis] = std::max(0, b.lo[axis] - R), b.hi[axis] = std::min(whd[axis], b.hi[axis] + R);
    return b;
  };
  const auto after_y = wide(region, 2), after_x = wide(after_y, 1);
  auto       xs = vector<float>(after_x.count()), ys = vector<float>(after_y.count()), zs = vector<float>(region.count());
  blur_pass<R>(w, 0, whd, voxels, whole, xs.data(), after_x);
  blur_pass<R>(w, 1, whd, xs.data(), after_x, ys.data(), after_y);
  blur_pass<R>(w, 2, whd, ys.data(), after_y, zs.data(), region);
  for (auto z = region.lo[2]; z < region.hi[2]; z++)
    for (auto y = region.lo[1]; y < region.hi[1]; y++)
      for (auto x = region.lo[0]; x < region.hi[0]; x++) voxels[whole.at(x, y, z)] = zs[region.at(x, y, z)];
}

}  // namespace

bool filter_voxels(float* voxels, const int32_t whd[3], const vpt_filter_entry& e, const vpt_filter_op* ops, int num_ops, string& error) {
  if (num_ops < 0 || (num_ops > 0 && !ops)) return error = "filter: the op list is null or has a negative count", false;
  for (auto i = 0; i < num_ops; i++)
    if (auto fault = vpt_filter_op_fault(ops[i])) return error = "filter: op " + std::to_string(i) + ": " + fault, false;
  bool unsupported;
  if (auto fault = vpt_filter_entry_fault(e, whd, ops, num_ops, &unsupported)) return error = string{"filter: entry 0: "} + fault, false;
  if ((size_t)e.region_whd[0] * (size_t)e.region_whd[1] * (size_t)e.region_whd[2] == 0) return true;
  for (auto s = e.first_op; s < e.first_op + e.num_ops; s++) {
    const auto r = vpt_filter_make_record(ops[s]);
    if (r.type == VPT_FILTER_BLUR) {
      switch (r.count) {
        case 1: blur_region<1>(voxels, whd, e, r.p); break;
        case 2: blur_region<2>(voxels, whd, e, r.p); break;
        case 3: blur_region<3>(voxels, whd, e, r.p); break;
        default: blur_region<4>(voxels, whd, e, r.p); break;
      }
      continue;
    }
    for (auto z = 0; z < e.region_whd[2]; z++)
      for (auto y = 0; y < e.region_whd[1]; y++)
        for (auto x = 0; x < e.region_whd[0]; x++) {
          const int i = e.region_lo[0] + x, j = e.region_lo[1] + y, k = e.region_lo[2] + z;
          auto&     voxel = voxels[(size_t)i + (size_t)j * (size_t)whd[0] + (size_t)k * (size_t)whd[0] * (size_t)whd[1]];
          voxel = vpt_filter_pointwise(r, vpt_filter_sample(e.origin[0], e.step[0], i), vpt_filter_sample(e.origin[1], e.step[1], j),
              vpt_filter_sample(e.origin[2], e.step[2], k), voxel);
        }
  }
  return true;
}

bool filter_gaussian_weights(float sigma, int radius, float* weights) {
  if (!std::isfinite(sigma) || !(sigma > 0) || radius < 1 || radius > VPT_FILTER_MAX_RADIUS || !weights) return false;
  double g[VPT_FILTER_MAX_RADIUS + 1], sum = 0;
  for (auto i = 0; i <= radius; i++) {
    g[i] = std::exp(-(double)(i * i) / (2.0 * (double)sigma * (double)sigma));
    sum += i ? 2 * g[i] : g[i];
  }
  for (auto i = 0; i <= radius; i++) weights[i] = (float)(g[i] / sum);
  return true;
}

}  // namespace vpt

extern "C" {

// the host mirror on a host array of whd[0] * whd[1] * whd[2] voxels (x fastest); entry->volume is ignored.  A refused call writes nothing.
int vpth_filter_voxels(float* voxels, const int32_t* whd, const vpt_filter_entry* entry, const vpt_filter_op* ops, int num_ops, char* err, int errlen) {
  auto error = vpt::string{};
  if (!voxels || !whd || !entry) error = "filter: null argument";
  else if (whd[0] < 0 || whd[1] < 0 || whd[2] < 0) error = "filter: bad volume size";
  else if (vpt::filter_voxels(voxels, whd, *entry, ops, num_ops, error)) return 0;
  if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", error.c_str());
  return -1;
}
// w[0..radius] of a BLUR op from a sigma > 0: exp(-i^2 / (2 sigma^2)) in float64, normalised so that w0 + 2 sum wi = 1, rounded to float32;
// -1 for a sigma that is not finite and positive, a radius outside 1..4 or a null pointer
int vpth_filter_gaussian_weights(float sigma, int radius, float* weights) { return vpt::filter_gaussian_weights(sigma, radius, weights) ? 0 : -1; }

}  // extern "C"
