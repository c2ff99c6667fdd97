// vpt_volgrid.cpp — the host mirror of the volgrid shader's tables and lookup (include/vpt.h: VPT_SHADER_VOLGRID), compiled from the rule
// header the kernel compiles (csrc/vpt_volgrid_rule.h) with -ffp-contract=off: the brick majorants of a volume and the density of the
// grid instances at world points, over a flattened scene descriptor.  It is no renderer: the project has none on the CPU.  What the device
// answers to vpt_scene_get_volgrid_majorants and vpt_scene_volgrid_density for the same scene has these bits.
#include <cstdio>
#include <vector>

#include "vpt_volgrid_rule.h"

namespace {
int fail(char* err, int err_len, const char* fmt, int a, int b, double c) {
  if (err && err_len > 0) snprintf(err, (size_t)err_len, fmt, a, b, c);
  return -1;
}
}  // namespace

extern "C" {

// the brick table of `volume`, x fastest; dims (nullable): bricks per axis; out nullable with capacity 0
int vpth_volgrid_majorants(const vpt_scene_desc* d, int volume, float* out, int64_t capacity, int32_t* dims, char* err, int err_len) {
  if (!d || volume < 0 || volume >= d->num_volumes) return fail(err, err_len, "volume %d out of range (%d)", volume, d ? d->num_volumes : 0, 0);
  const vpt_volume& v = d->volumes[volume];
  const int nb[3] = {vpt_volgrid_bricks(v.whd[0]), vpt_volgrid_bricks(v.whd[1]), vpt_volgrid_bricks(v.whd[2])};
  if (dims) dims[0] = nb[0], dims[1] = nb[1], dims[2] = nb[2];
  if (!out) return 0;
  const long long n = (long long)nb[0] * nb[1] * nb[2];
  if (capacity < n) return fail(err, err_len, "capacity %d < %d bricks", (int)capacity, (int)n, 0);
  for (int bz = 0; bz < nb[2]; bz++)
    for (int by = 0; by < nb[1]; by++)
      for (int bx = 0; bx < nb[0]; bx++)
        out[bx + nb[0] * (by + nb[1] * bz)] = vpt_volgrid_brick_max(d->voxels + v.offset, v.whd[0], v.whd[1], v.whd[2], bx, by, bz);
  return 0;
}

// sigma[i] = the sum over the grid instances, in index order, of their densities at point i; instance[i] (nullable) = the first
// instance whose box holds the point, or -1
int vpth_volgrid_density(const vpt_scene_desc* d, int n, const float* points, int32_t* instance, float* sigma, char* err, int err_len) {
  if (!d || n < 0 || (n > 0 && (!points || !sigma))) return fail(err, err_len, "bad argument", 0, 0, 0);
  std::vector<vpt_volgrid_record> recs((size_t)d->num_vol_instances);
  for (int g = 0; g < d->num_vol_instances; g++) {
    const vpt_volume_instance& vi = d->vol_instances[g];
    if (!vpt_volgrid_trdepth_ok(d->materials[vi.material].trdepth))
      return fail(err, err_len, "volgrid: vol_instance %d: material %d has trdepth %g (a medium needs a finite trdepth > 0)", g, vi.material,
          (double)d->materials[vi.material].trdepth);
    recs[(size_t)g] = vpt_volgrid_make_record(vi, d->volumes[vi.volume], d->materials[vi.material], 0);
  }
  for (int i = 0; i < n; i++) {
    float sum   = 0.0f;
    int   first = -1;
    for (int g = 0; g < d->num_vol_instances; g++) {
      float node[3];
      if (!vpt_volgrid_locate(recs[(size_t)g], points[3 * i], points[3 * i + 1], points[3 * i + 2], node)) continue;
      if (first < 0) first = g;
      sum += vpt_volgrid_sigma_at(recs[(size_t)g], d->voxels, node);
    }
    sigma[i] = sum;
    if (instance) instance[i] = first;
  }
  return 0;
}

}  // extern "C"
