// vpt_volgrid.hip — the host side of the volgrid shader (include/vpt.h: VPT_SHADER_VOLGRID): K3's tables - the records of the grid instances
// as media, made on the host from the handle's mirrors, and the brick majorants of the volumes, reduced on the device from the voxels where
// they lie - kept current against the handle's edit counters, the refusals of a volgrid render, the two queries over a resident scene, and the host side
// of the free-flight probe (vpt_scene_volgrid_track).  The arithmetic is csrc/vpt_volgrid_rule.h's; K3 itself and the probe's kernel are vpt_k3.hip's.
#include <cmath>
#include <cstdlib>
#include <vector>

#include "vpt_scene_handle.h"
#include "vpt_volgrid_rule.h"

namespace {

// one lane per brick of one volume: vpt_volgrid_brick_max over its nine-node neighbourhood
__global__ void volgrid_brick_kernel(const float* __restrict__ vox, int w, int h, int d, int nbx, int nby, int nbz, float* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nbx * nby * nbz) return;
  out[b] = vpt_volgrid_brick_max(vox, w, h, d, b % nbx, (b / nbx) % nby, b / (nbx * nby));
}
// one block per volume: the maximum of its n bricks into the word behind them (non-negative floats order like their bits)
__global__ void volgrid_volume_max_kernel(float* __restrict__ bricks, int n) {
  __shared__ int s_max;
  if (threadIdx.x == 0) s_max = 0;
  __syncthreads();
  float m = 0.0f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) m = bricks[i] > m ? bricks[i] : m;
  atomicMax(&s_max, __float_as_int(m));
  __syncthreads();
  if (threadIdx.x == 0) bricks[n] = __int_as_float(s_max);
}
// one lane per point: the sum of the instances' densities in index order, and the first instance whose box holds the point
__global__ void volgrid_density_kernel(const vpt_volgrid_record* __restrict__ recs, int num, const float* __restrict__ voxels, int n,
    const float* __restrict__ points, int* __restrict__ instance, float* __restrict__ sigma) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
  float sum   = 0.0f;
  int   first = -1;
  for (int g = 0; g < num; g++) {
    float node[3];
    if (!vpt_volgrid_locate(recs[g], px, py, pz, node)) continue;
    if (first < 0) first = g;
    sum += vpt_volgrid_sigma_at(recs[g], voxels, node);
  }
  sigma[i] = sum;
  if (instance) instance[i] = first;
}

int check_media(const vpt_scene* s) {
  for (size_t g = 0; g < s->m.vol_instances.size(); g++) {
    const int mat = s->m.vol_instances[g].material;
    REQUIRE(vpt_volgrid_trdepth_ok(s->m.materials[(size_t)mat].trdepth), "volgrid: vol_instance %d: material %d has trdepth %g (a medium needs a finite trdepth > 0)",
        (int)g, mat, (double)s->m.materials[(size_t)mat].trdepth);
  }
  REQUIRE(s->m.vol_instances.size() * sizeof(vpt_volgrid_record) <= 64 * 1024, "volgrid: %d grid instances exceed the kernel's LDS copy of their records (512)",
      (int)s->m.vol_instances.size());
  return VPT_OK;
}

// the tables as the scene stands now, on `st`
int sync_tables(vpt_scene* s, hipStream_t st) {
  volgrid_tables& t = s->volgrid;
  if (t.built_edits == s->edit_generation) return VPT_OK;
  HIP_TRY(hipSetDevice(s->device));
  const std::vector<vpt_volume>& vols = s->m.volumes;
  std::vector<int> offset(vols.size());
  long long        total = 0;
  for (size_t v = 0; v < vols.size(); v++) {
    offset[v] = (int)total;
    total += (long long)vpt_volgrid_bricks(vols[v].whd[0]) * vpt_volgrid_bricks(vols[v].whd[1]) * vpt_volgrid_bricks(vols[v].whd[2]) + 1;
    if (total >= (1ll << 31)) return vpt_set_error(VPT_ERR_UNSUPPORTED, "volgrid: the scene's brick tables exceed 2^31 entries");
  }
  if (!t.steps.get()) {
    if (int rc = t.steps.allocate(8)) return rc;
    HIP_TRY(hipMemsetAsync(t.steps.get(), 0, 8, st));
  }
  if (t.built_voxels != s->voxel_generation || offset != t.brick_offset || total != t.num_bricks) {   // voxels were written, or volumes changed size
    if (total != t.num_bricks || !t.bricks.get())
      if (int rc = t.bricks.allocate((size_t)total * sizeof(float))) return rc;
    for (size_t v = 0; v < vols.size(); v++) {
      const int nbx = vpt_volgrid_bricks(vols[v].whd[0]), nby = vpt_volgrid_bricks(vols[v].whd[1]), nbz = vpt_volgrid_bricks(vols[v].whd[2]);
      const int n = nbx * nby * nbz;
      float*    out = t.bricks.get<float>() + offset[v];
      if (n > 0)
        hipLaunchKernelGGL(volgrid_brick_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, s->d.voxels + vols[v].offset, vols[v].whd[0], vols[v].whd[1],
            vols[v].whd[2], nbx, nby, nbz, out);
      hipLaunchKernelGGL(volgrid_volume_max_kernel, dim3(1), dim3(256), 0, st, out, n);
    }
    HIP_TRY(hipGetLastError());
    t.brick_offset = offset, t.num_bricks = total, t.built_voxels = s->voxel_generation, t.rebuilds++;
  }
  // the records: instances, volumes and materials as the mirrors hold them
  std::vector<vpt_volgrid_record> recs(s->m.vol_instances.size());
  for (size_t g = 0; g < recs.size(); g++) {
    const vpt_volume_instance& vi = s->m.vol_instances[g];
    recs[g] = vpt_volgrid_make_record(vi, vols[(size_t)vi.volume], s->m.materials[(size_t)vi.material], offset[(size_t)vi.volume]);
  }
  if (int rc = t.recs.allocate(recs.size() * sizeof(vpt_volgrid_record))) return rc;
  if (!recs.empty()) HIP_TRY(hipMemcpy(t.recs.get(), recs.data(), recs.size() * sizeof(vpt_volgrid_record), hipMemcpyHostToDevice));
  t.num_env_lights = 0;
  for (const vpt_light& l : s->m.lights) t.num_env_lights += l.environment >= 0;
  t.built_edits = s->edit_generation;
  return VPT_OK;
}

}  // namespace

int volgrid_prepare(vpt_scene* s, hipStream_t st) {
  if (int rc = check_media(s)) return rc;
  return sync_tables(s, st);
}

volgrid_args volgrid_arguments(const vpt_scene* s) {
  const volgrid_tables& t = s->volgrid;
  const char* e = getenv("VPT_VOLGRID_NO_BRICKS");
  return {t.recs.get<const vpt_volgrid_record>(), t.bricks.get<const float>(), s->d.num_vol_instances, t.num_env_lights, e && e[0] == '1' ? 1 : 0,
      s->d_watchdog.get<unsigned>(), t.steps.get<unsigned long long>()};
}

extern "C" {

int vpt_scene_get_volgrid_majorants(vpt_scene* s, int volume, float* out, int64_t capacity, int32_t dims[3]) {
  REQUIRE(s, "null argument");
  REQUIRE(volume >= 0 && volume < s->d.num_volumes, "volume %d out of range (%d)", volume, s->d.num_volumes);
  REQUIRE(capacity >= 0 && (capacity == 0 || out), "bad capacity");
  if (int rc = sync_tables(s, nullptr)) return rc;
  const vpt_volume& v = s->m.volumes[(size_t)volume];
  const int nb[3] = {vpt_volgrid_bricks(v.whd[0]), vpt_volgrid_bricks(v.whd[1]), vpt_volgrid_bricks(v.whd[2])};
  if (dims) dims[0] = nb[0], dims[1] = nb[1], dims[2] = nb[2];
  if (!out) return VPT_OK;
  const long long n = (long long)nb[0] * nb[1] * nb[2];
  REQUIRE(capacity >= n, "capacity %lld < %lld bricks", (long long)capacity, n);
  HIP_TRY(hipDeviceSynchronize());
  if (n > 0) HIP_TRY(hipMemcpy(out, s->volgrid.bricks.get<float>() + s->volgrid.brick_offset[(size_t)volume], (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  return VPT_OK;
}

int vpt_scene_volgrid_density(vpt_scene* s, int n, const float* points, int32_t* instance, float* sigma) {
  REQUIRE(s && n >= 0 && (n == 0 || (points && sigma)), "bad argument");
  if (int rc = volgrid_prepare(s, nullptr)) return rc;
  if (n == 0) return VPT_OK;
  device_buffer d_points, d_instance, d_sigma;
  if (int rc = d_points.allocate((size_t)n * 12)) return rc;
  if (int rc = d_instance.allocate((size_t)n * 4)) return rc;
  if (int rc = d_sigma.allocate((size_t)n * 4)) return rc;
  HIP_TRY(hipMemcpy(d_points.get(), points, (size_t)n * 12, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(volgrid_density_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, s->volgrid.recs.get<const vpt_volgrid_record>(),
      s->d.num_vol_instances, s->d.voxels, n, d_points.get<const float>(), d_instance.get<int>(), d_sigma.get<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(sigma, d_sigma.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
  if (instance) HIP_TRY(hipMemcpy(instance, d_instance.get(), (size_t)n * 4, hipMemcpyDeviceToHost));
  return VPT_OK;
}

int vpt_scene_volgrid_track(vpt_scene* s, int n, const float* rays, const uint64_t* rng_in, int32_t* event, int32_t* instance, float* t, int32_t* steps,
    uint64_t* rng_out) {
  REQUIRE(s && n >= 0 && (n == 0 || (rays && rng_in && event && instance && t && steps)), "bad argument");
  for (int i = 0; i < n; i++) {
    const float* r = rays + 6 * (size_t)i;
    for (int k = 0; k < 6; k++) REQUIRE(std::isfinite(r[k]), "volgrid_track: ray %d has a component that is not finite", i);
    const double len = std::sqrt((double)r[3] * r[3] + (double)r[4] * r[4] + (double)r[5] * r[5]);
    REQUIRE(std::fabs(len - 1.0) <= 1e-3, "volgrid_track: ray %d has a direction of length %g (a unit vector within 1e-3 is needed)", i, len);
  }
  if (int rc = volgrid_prepare(s, nullptr)) return rc;
  if (n == 0) return VPT_OK;
  HIP_TRY(hipSetDevice(s->device));
  device_buffer d_rays, d_rng, d_out;   // d_out: event, instance, t, steps - four planes of n words
  if (int rc = d_rays.allocate((size_t)n * 24)) return rc;
  if (int rc = d_rng.allocate((size_t)n * 32)) return rc;   // in, then out
  if (int rc = d_out.allocate((size_t)n * 16)) return rc;
  HIP_TRY(hipMemcpy(d_rays.get(), rays, (size_t)n * 24, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_rng.get(), rng_in, (size_t)n * 16, hipMemcpyHostToDevice));
  int*        o  = d_out.get<int>();
  ulonglong2* rg = d_rng.get<ulonglong2>();
  hipLaunchKernelGGL(vpt_volgrid_track_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, nullptr, s->d, volgrid_arguments(s), n, d_rays.get<const float>(),
      (const ulonglong2*)rg, o, o + n, (float*)(o + 2 * (size_t)n), o + 3 * (size_t)n, rng_out ? rg + n : nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(event, o, (size_t)n * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(instance, o + n, (size_t)n * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(t, o + 2 * (size_t)n, (size_t)n * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(steps, o + 3 * (size_t)n, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (rng_out) HIP_TRY(hipMemcpy(rng_out, rg + n, (size_t)n * 16, hipMemcpyDeviceToHost));
  return VPT_OK;
}

int vpt_scene_volgrid_stats(vpt_scene* s, uint64_t* steps, int32_t* table_builds) {
  REQUIRE(s, "null argument");
  if (table_builds) *table_builds = s->volgrid.rebuilds;
  if (steps) {
    *steps = 0;
    if (s->volgrid.steps.get()) {
      HIP_TRY(hipSetDevice(s->device));
      HIP_TRY(hipDeviceSynchronize());
      HIP_TRY(hipMemcpy(steps, s->volgrid.steps.get(), 8, hipMemcpyDeviceToHost));
    }
  }
  return VPT_OK;
}

}  // extern "C"
