// vpt_light_update.hip — the light tables of a resident scene rebuilt on the device (include/vpt.h: vpt_scene_update_lights;
// DESIGN.md §14): make_lights (yocto_pathtrace.cpp:983-1049) and build_lights (vpt_scene_prep.cpp) for a scene whose positions,
// elements, materials and instances already live in HBM.  The list is decided on the host from the handle's mirrors (integer
// work); nothing proportional to an element or texel count crosses PCIe: a light that stays moves device to device, a mesh
// light that is new or whose shape moved gets its areas, its running sum, its 16-ary levels and its guide table from the kernels
// below.  What does cross: a few words per light (its list entry, its index header, its record tag, the descriptor of its job,
// and {sorted, last entry} back).
// An edit of environments or textures (vpt_scene_update_textures, vpt_texture_update.hip) comes through here too: an environment whose
// CDF has to be made anew is a job like a mesh light's, with the weight of its texels where a mesh light has the areas of its elements.
// Arithmetic = the reference's, operation by operation (-ffp-contract=off, correctly rounded / and sqrt): the areas of
// yocto_geometry.h:506-518, cdf[i] = area_i + cdf[i - 1] in element order.  Float addition is not associative, so the running sum
// is a serial chain per light: no tree, no block scan.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "vpt_error.h"
#include "vpt_light_update.h"
#include "vpt_math.hip.h"
#include "vpt_texture_update.h"
#include "vpt_update_helpers.h"

namespace {

enum { JOB_QUADS = 0, JOB_TRIANGLES = 1, JOB_TEXELS = 2 };   // areas of a mesh light's elements / weights of an environment's texels
struct light_job {   // one light whose CDF is recomputed
  long long cdf_offset;
  int       elem_offset, vertex_offset, num_elems, kind;
};
struct job_result { int sorted; float back; };

// ---- kernels --------------------------------------------------------------------------------------------------------------
__device__ inline float triangle_area(f3 p0, f3 p1, f3 p2) { return length(cross(p1 - p0, p2 - p0)) / 2; }   // yocto_geometry.h:506-510

// one lane per element (blockIdx.y: the job): its area into the slot its CDF entry will take
__global__ void lit_areas_kernel(const light_job* __restrict__ jobs, int first_job, const int4* __restrict__ elems, const float4* __restrict__ positions,
    float* __restrict__ cdf) {
  const light_job j = jobs[first_job + blockIdx.y];
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= j.num_elems || j.kind == JOB_TEXELS) return;
  const int4    q = elems[(long long)j.elem_offset + e];
  const float4* P = positions + j.vertex_offset;
  const f3 p0 = xyz(P[q.x]), p1 = xyz(P[q.y]), p2 = xyz(P[q.z]);
  float a;
  if (j.kind == JOB_TRIANGLES) a = triangle_area(p0, p1, p2);
  else {   // quad_area, yocto_geometry.h:512-518
    const f3 p3 = xyz(P[q.w]);
    a = triangle_area(p0, p1, p3) + triangle_area(p2, p3, p1);
  }
  cdf[j.cdf_offset + e] = a;
}

// The running sum, in place, one wave per light.  A block of 64 areas sits one to a lane; the chain takes 64 dependent steps through
// it: the step's area comes out of its lane as a wave-uniform value (v_readlane) and is added to the carry that every lane holds,
// and the carry of step k goes to word k of an LDS row (every lane stores the same value: no mask to form), from where lane k
// picks it up after the block - three instructions a step, the add the only dependent one.  The next block's load is issued
// before the chain starts, so HBM latency hides behind the 64 steps; loads and stores are one coalesced 256-byte row per block.
// Lanes past the end hold zeros: they come after the last entry in the chain.
// result: {entries non-decreasing (false for NaN too), last entry}.
__global__ void __launch_bounds__(64) lit_scan_wave_kernel(const light_job* __restrict__ jobs, float* cdf, job_result* __restrict__ result) {
  __shared__ float sums[64];
  const light_job j = jobs[blockIdx.x];
  float*    c    = cdf + j.cdf_offset;
  const int n    = j.num_elems, lane = (int)threadIdx.x;
  float     carry = 0, out = 0;
  bool      ok    = true;
  float     next  = lane < n ? c[lane] : 0.0f;
  for (int base = 0; base < n; base += 64) {
    const float a = next, carry_in = carry;
    next = base + 64 + lane < n ? c[base + 64 + lane] : 0.0f;
#pragma unroll
    for (int k = 0; k < 64; k++) {
      const float ak = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), k));
      if (k == 0) carry = base == 0 ? ak : ak + carry;   // cdf[0] is the area itself
      else carry = ak + carry;
      sums[k] = carry;
    }
    out = sums[lane];   // this lane's own store among them: program order is enough
    float before = __shfl_up(out, 1);
    if (lane == 0) before = carry_in;
    const int i = base + lane;
    if (i >= 1 && i < n && !(before <= out)) ok = false;
    if (i < n) c[i] = out;
  }
  const float back = __shfl(out, (n - 1) & 63);
  const int sorted = __all(ok);
  if (lane == 0) result[blockIdx.x] = {sorted, n > 0 ? back : 0.0f};
}
// the same chain by one lane per light straight from global memory (VPT_LIGHTS_PLAIN=1: the A/B form, same bits)
__global__ void lit_scan_plain_kernel(const light_job* __restrict__ jobs, int njobs, float* cdf, job_result* __restrict__ result) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= njobs) return;
  const light_job j = jobs[t];
  float* c = cdf + j.cdf_offset;
  bool   ok = true;
  for (int i = 1; i < j.num_elems; i++) {
    c[i] = c[i] + c[i - 1];
    if (!(c[i - 1] <= c[i])) ok = false;
  }
  result[t] = {ok ? 1 : 0, j.num_elems > 0 ? c[j.num_elems - 1] : 0.0f};
}

// The levels of one light's 16-ary index (DCdfIndex, vpt_device.h) straight from its CDF: entry g of level k is the last element of
// a group of 16^k, cdf[min(n - 1, 16^k (g + 1) - 1)] - what build_lights reaches level by level; the padding of every level is +inf.
struct index_fill { int levels, end, offset[8], size[8]; };
__global__ void lit_index_levels_kernel(float* __restrict__ pool, index_fill f, const float* __restrict__ cdf, int n) {
  const long long at = (long long)f.offset[0] + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (at >= f.end) return;
  int lv = 0;
  while (lv + 1 < f.levels && at >= f.offset[lv + 1]) lv++;
  const long long g = at - f.offset[lv];
  float v = __int_as_float(0x7f800000);
  if (g < f.size[lv]) {
    long long k = ((g + 1) << (4 * lv)) - 1;
    if (k > n - 1) k = n - 1;
    v = cdf[k];
  }
  pool[at] = v;
}

__device__ inline int upper_bound(const float* c, int n, float v) {   // std::upper_bound
  int first = 0, len = n;
  while (len > 0) {
    const int half = len >> 1, mid = first + half;
    if (!(v < c[mid])) first = mid + 1, len -= half + 1;
    else len = half;
  }
  return first;
}
__device__ inline float next_down(float x) {   // std::nextafter(x, -inf) of a finite x
  if (x == 0) return __int_as_float((int)0x80000001);
  const int b = __float_as_int(x);
  return __int_as_float(x > 0 ? b - 1 : b + 1);
}
__device__ inline float next_up(float x) {   // std::nextafter(x, +inf) of a finite x (the largest float goes to +inf, as there)
  if (x == 0) return __int_as_float(1);
  const int b = __float_as_int(x);
  return __int_as_float(x > 0 ? b + 1 : b - 1);
}
// the guide table of build_lights, one lane per bucket: the bounds in double, widened by one float, bracketed by upper_bound
__global__ void lit_guide_kernel(int2* __restrict__ guide, int buckets, float scale, const float* __restrict__ cdf, int n) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= buckets) return;
  const double lo_r = (double)b * (1.0 - 1.0 / 8388608.0) / (double)scale, hi_r = (double)(b + 1) * (1.0 + 1.0 / 4194304.0) / (double)scale;
  const float  lf = next_down((float)lo_r), hf = next_up((float)hi_r);
  const int    lo = b == 0 ? 0 : upper_bound(cdf, n, lf);
  const int    hi = b == buckets - 1 ? n : upper_bound(cdf, n, hf);
  guide[b] = make_int2(lo, hi);
}

// light records (build_lights) of mesh and SDF lights; an environment's record moved as it was, or (env_totals) sent by the host
// without the one word that comes from the CDF: the total of a textured environment
__global__ void lit_records_kernel(float4* __restrict__ rec, const vpt_light* __restrict__ lights, const int* __restrict__ tags, int n,
    const float* __restrict__ cdf, const DInstance* __restrict__ instances, const DShape* __restrict__ shapes, int env_totals) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= n) return;
  const int tag = tags[l], kind = tag & 255;
  float4* r = rec + 8 * (long long)l;
  if (kind == VPT_LIGHT_ENV_TEX || kind == VPT_LIGHT_ENV_CONST) {
    if (env_totals && kind == VPT_LIGHT_ENV_TEX && lights[l].cdf_len > 0) r[6].z = cdf[lights[l].cdf_offset + lights[l].cdf_len - 1];
    return;
  }
  for (int k = 0; k < 8; k++) r[k] = make_float4(0, 0, 0, 0);
  const vpt_light lt = lights[l];
  if (lt.instance >= 0) {
    const DInstance& in = instances[lt.instance];
    const DShape&    sh = shapes[in.shape];
    const float total = lt.cdf_len > 0 ? cdf[lt.cdf_offset + lt.cdf_len - 1] : 0.0f;
    for (int k = 0; k < 3; k++) r[k] = in.inv[k], r[3 + k] = in.fwd[k];
    r[6] = make_float4(sh.root_box[0], sh.root_box[1], sh.root_box[2], total);
    r[7] = make_float4(sh.root_box[3], sh.root_box[4], sh.root_box[5], 0);
  }
  r[7].w = __int_as_float(tag);
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// The layout build_lights gives the index of an n-entry CDF that starts at `at` of the pool: the level offsets and sizes, and where
// the pool continues.  false: no index (more than 8 levels).
bool index_layout(long long n, long long at, DCdfIndex& ix, index_fill& f) {
  ix = {}, f = {};
  long long size = n;
  while (true) {
    if (ix.levels == 8) return ix = {}, false;
    f.offset[ix.levels] = ix.offset[ix.levels] = (int)at, f.size[ix.levels] = (int)size;
    ix.levels++, ix.top_count = (int)size;
    at = (at + size + 15) / 16 * 16 + (ix.levels == 1 ? 16 : 0);   // level 0 is also read 16-wide from any index
    if (size <= 16) break;
    size = (size + 15) / 16;
  }
  f.levels = ix.levels, f.end = (int)at;
  return true;
}

struct entry {   // one light of the new list
  vpt_light l;
  int  from;        // its place in the old list, -1: new
  bool recompute;   // a mesh light that is new or whose shape moved; an environment whose light, texture or texels are new
  int  tag;         // kind | count << 8 of its record
};

}  // namespace

int light_update_apply(resident& r, const vpt_scene_edit& e, bool* rebuilt, const std::vector<env_light>* envs, const std::vector<char>* sdf_resized,
    const std::vector<int>* old_instance, const std::vector<int>* old_sdf) {
  *rebuilt = false;
  DScene&             d = r.d;
  const host_mirrors& h = r.h;
  edit_mirrors&       u = r.m;

  // 1. the list (make_lights): emissive instances of faces, the environments that were lights, emissive SDFs - each in id order
  const std::vector<vpt_light>& old = u.lights;
  int old_instances = d.num_instances;   // (the instances were renumbered: the old list and the map name old ids)
  for (size_t l = 0; old_instance && l < old.size(); l++) old_instances = old[l].instance >= old_instances ? old[l].instance + 1 : old_instances;
  for (size_t i = 0; old_instance && i < old_instance->size(); i++) old_instances = (*old_instance)[i] >= old_instances ? (*old_instance)[i] + 1 : old_instances;
  int old_sdfs = d.num_sdfs;   // (the same of the SDFs)
  for (size_t l = 0; old_sdf && l < old.size(); l++) old_sdfs = old[l].sdf >= old_sdfs ? old[l].sdf + 1 : old_sdfs;
  for (size_t i = 0; old_sdf && i < old_sdf->size(); i++) old_sdfs = (*old_sdf)[i] >= old_sdfs ? (*old_sdf)[i] + 1 : old_sdfs;
  std::vector<int>  old_of_instance((size_t)old_instances, -1), old_of_sdf((size_t)old_sdfs, -1), old_of_env((size_t)d.num_environments, -1);
  std::vector<char> moved((size_t)d.num_shapes, 0);
  for (size_t l = 0; l < old.size(); l++) {
    if (old[l].instance >= 0) old_of_instance[(size_t)old[l].instance] = (int)l;
    else if (old[l].sdf >= 0) old_of_sdf[(size_t)old[l].sdf] = (int)l;
    else if (old[l].environment >= 0) old_of_env[(size_t)old[l].environment] = (int)l;
  }
  for (int i = 0; i < e.num_shapes; i++) moved[(size_t)e.shape_ids[i]] = 1;
  std::vector<entry> list;
  for (int i = 0; i < d.num_instances; i++) {
    if (!emissive(u.materials[(size_t)u.inst_material[(size_t)i]])) continue;
    const int     shape = h.inst_shape[(size_t)i];
    const DShape& sh    = u.shapes[(size_t)shape];
    if ((u.inst_flags[(size_t)i] & (VPT_SHP_POINTS | VPT_SHP_LINES)) || sh.num_elems <= 0) continue;   // points and lines are never lights
    const bool small = sh.root_ref < 0 && ((~sh.root_ref) & 15) <= 4;   // build_lights: one leaf of <= 4 primitives is walked inline
    const int  was   = old_instance ? (*old_instance)[(size_t)i] : i;   // -1: a new instance, or one whose shape is another now
    const int  from  = was >= 0 ? old_of_instance[(size_t)was] : -1;
    list.push_back({{i, VPT_INVALID, VPT_INVALID, sh.num_elems, 0}, from, from < 0 || moved[(size_t)shape] != 0,
        small ? VPT_LIGHT_SMALL_MESH | (((~sh.root_ref) & 15) << 8) : VPT_LIGHT_LARGE_MESH});
  }
  std::vector<int> env_of;   // the entry of `envs` behind a light of the new list, -1: none
  if (envs) {                // vpt_scene_update_textures: the environments as the edit leaves them
    for (size_t k = 0; k < envs->size(); k++) {
      const env_light& ev = (*envs)[k];
      env_of.resize(list.size(), -1), env_of.push_back((int)k);
      list.push_back({{VPT_INVALID, ev.environment, VPT_INVALID, ev.cdf_len, 0}, old_of_env[(size_t)ev.environment], ev.recompute, ev.tag});
    }
  } else
    for (size_t l = 0; l < old.size(); l++)   // the edit has no field for an environment's emission or texture
      if (old[l].instance < 0 && old[l].sdf < 0) list.push_back({old[l], (int)l, false, u.light_kind[l]});
  for (int i = 0; i < d.num_sdfs; i++) {
    if (!emissive(u.materials[(size_t)u.sdfs[(size_t)i].material])) continue;
    const int was = old_sdf ? (*old_sdf)[(size_t)i] : i;   // -1: an added SDF
    list.push_back({{VPT_INVALID, VPT_INVALID, i, 1, 0}, was >= 0 ? old_of_sdf[(size_t)was] : -1, false, VPT_LIGHT_SDF});
  }
  bool same = list.size() == old.size();
  for (size_t l = 0; same && l < list.size(); l++) same = list[l].from == (int)l && !list[l].recompute && list[l].l.cdf_len == old[l].cdf_len;
  // the same lights by position may be other instance ids after a renumbering: vpt_light::instance, the records and light_prims name them
  for (size_t l = 0; same && old_instance && l < list.size(); l++) same = list[l].l.instance == old[l].instance;
  for (size_t l = 0; same && old_sdf && l < list.size(); l++) same = list[l].l.sdf == old[l].sdf;   // the same of vpt_light::sdf
  for (size_t l = 0; same && sdf_resized && l < list.size(); l++) same = list[l].l.sdf < 0 || !(*sdf_resized)[(size_t)list[l].l.sdf];   // its one CDF entry is whd.x * whd.y
  env_of.resize(list.size(), -1);
  if (same) return VPT_OK;   // no consequence for the lights: the update has done all there is to do
  *rebuilt = true;

  // 2. the CDF pool: cdf_offset = the sum of the earlier lengths, as the host flattening lays it out
  const int nl = (int)list.size();
  long long num_cdf = 0;
  for (entry& en : list) en.l.cdf_offset = num_cdf, num_cdf += en.l.cdf_len;
  device_buffer cdf_buf;
  if (int rc = cdf_buf.allocate((size_t)num_cdf * sizeof(float))) return rc;
  float* cdf = cdf_buf.get<float>();
  std::vector<light_job> jobs;
  std::vector<int>       job_light;
  for (int l = 0; l < nl; l++) {
    const entry& en = list[(size_t)l];
    if (en.l.sdf >= 0) {   // make_lights: cdf = {whd.x * whd.y}
      const float area = u.sdfs[(size_t)en.l.sdf].whd[0] * u.sdfs[(size_t)en.l.sdf].whd[1];
      if (int rc = send(r, cdf + en.l.cdf_offset, &area, 1)) return rc;
    } else if (en.recompute && en.l.instance < 0) {   // an environment: one weight per texel
      jobs.push_back({en.l.cdf_offset, 0, 0, en.l.cdf_len, JOB_TEXELS});
      job_light.push_back(l);
    } else if (en.recompute) {
      const DShape& sh = u.shapes[(size_t)h.inst_shape[(size_t)en.l.instance]];
      jobs.push_back({en.l.cdf_offset, sh.elem_offset, sh.vertex_offset, sh.num_elems, sh.is_triangles ? JOB_TRIANGLES : JOB_QUADS});
      job_light.push_back(l);
    } else if (en.l.cdf_len == 0) {   // an environment without a texture
    } else if (int rc = copy_on_device(cdf + en.l.cdf_offset, d.light_cdf + old[(size_t)en.from].cdf_offset, (size_t)en.l.cdf_len * sizeof(float))) return rc;
  }
  const int njobs = (int)jobs.size();
  std::vector<job_result> results;
  if (njobs > 0) {
    if (int rc = send(r, r.d_jobs, jobs)) return rc;
    if (int rc = r.d_result.allocate((size_t)njobs * sizeof(job_result))) return rc;
    const light_job* d_jobs = r.d_jobs.get<light_job>();
    for (int first = 0; first < njobs; first += 65535) {   // grid.y is a 16-bit count
      const int count = njobs - first < 65535 ? njobs - first : 65535;
      int most = 0;
      for (int k = first; k < first + count; k++)
        if (jobs[(size_t)k].kind != JOB_TEXELS) most = jobs[(size_t)k].num_elems > most ? jobs[(size_t)k].num_elems : most;
      if (most == 0) continue;   // texel jobs only
      hipLaunchKernelGGL(lit_areas_kernel, dim3(blocks_for(most), (unsigned)count), dim3(BLOCK), 0, 0, d_jobs, first, d.elems, d.positions, cdf);
      LAUNCHED(r);
    }
    for (int k = 0; k < njobs; k++)
      if (jobs[(size_t)k].kind == JOB_TEXELS) {
        if (int rc = launch_texel_weights(r, (*envs)[(size_t)env_of[(size_t)job_light[(size_t)k]]], cdf + jobs[(size_t)k].cdf_offset)) return rc;
      }
    if (getenv("VPT_LIGHTS_PLAIN")) LAUNCH(r, lit_scan_plain_kernel, njobs, d_jobs, njobs, cdf, r.d_result.get<job_result>());
    else {
      hipLaunchKernelGGL(lit_scan_wave_kernel, dim3((unsigned)njobs), dim3(64), 0, 0, d_jobs, cdf, r.d_result.get<job_result>());
      LAUNCHED(r);
    }
    if (int rc = fetch(r, results, r.d_result.get(), (size_t)njobs)) return rc;
  }

  // 3. the search structures: a light whose CDF moved keeps its index with the offsets rebased, a recomputed one gets build_lights'
  std::vector<DCdfIndex>  index((size_t)nl);
  std::vector<index_fill> fills((size_t)nl);
  std::vector<float>      scales((size_t)nl, 0.0f);
  long long num_pool = 0, num_guide = 0;
  for (int l = 0, job = 0; l < nl; l++) {
    const entry& en = list[(size_t)l];
    DCdfIndex&   ix = index[(size_t)l];
    index_fill&  f  = fills[(size_t)l];
    ix = {}, f = {};
    const long long n = en.l.cdf_len;
    if (en.recompute) {
      const job_result& r = results[(size_t)job++];
      if (!(n > 64 && r.sorted) || !index_layout(n, num_pool, ix, f)) continue;
      num_pool = f.end;
      const long long M     = n / 4;
      const float     scale = (float)M / r.back;
      if (!(r.back > 0) || !std::isfinite(scale) || M < 16) continue;
      ix.guide_offset = (int)num_guide, ix.guide_buckets = (int)M, ix.guide_scale = scale;
      num_guide += M;
    } else if (en.from >= 0 && n > 0 && u.light_index[(size_t)en.from].levels > 0) {   // (n = 0: an environment that lost its texture)
      const DCdfIndex& was = u.light_index[(size_t)en.from];
      index_layout(n, num_pool, ix, f);
      num_pool = f.end;
      if (was.guide_buckets > 0) ix.guide_offset = (int)num_guide, ix.guide_buckets = was.guide_buckets, ix.guide_scale = was.guide_scale, num_guide += was.guide_buckets;
    }
  }
  device_buffer pool_buf, guide_buf;
  if (int rc = pool_buf.allocate((size_t)num_pool * sizeof(float))) return rc;
  if (int rc = guide_buf.allocate((size_t)num_guide * sizeof(int2))) return rc;
  for (int l = 0; l < nl; l++) {
    const entry&     en = list[(size_t)l];
    const DCdfIndex& ix = index[(size_t)l];
    const index_fill& f = fills[(size_t)l];
    if (ix.levels == 0) continue;
    float* pool  = pool_buf.get<float>();
    int2*  guide = guide_buf.get<int2>() + ix.guide_offset;
    if (en.recompute) {
      LAUNCH(r, lit_index_levels_kernel, f.end - f.offset[0], pool, f, cdf + en.l.cdf_offset, en.l.cdf_len);
      LAUNCH(r, lit_guide_kernel, ix.guide_buckets, guide, ix.guide_buckets, ix.guide_scale, cdf + en.l.cdf_offset, en.l.cdf_len);
    } else {
      const DCdfIndex& was = u.light_index[(size_t)en.from];
      if (int rc = copy_on_device(pool + f.offset[0], d.light_index_pool + was.offset[0], (size_t)(f.end - f.offset[0]) * sizeof(float))) return rc;
      if (int rc = copy_on_device(guide, d.light_guide + was.guide_offset, (size_t)ix.guide_buckets * sizeof(int2))) return rc;
    }
  }

  // 4. the list, the index headers, the records, and zeros for vpt_light_setup_kernel to fill
  std::vector<vpt_light> lights((size_t)nl);
  std::vector<int>       tags((size_t)nl);
  for (int l = 0; l < nl; l++) lights[(size_t)l] = list[(size_t)l].l, tags[(size_t)l] = list[(size_t)l].tag;
  device_buffer lights_buf, index_buf, rec_buf, prims_buf;
  if (int rc = send(r, lights_buf, lights)) return rc;
  if (int rc = send(r, index_buf, index)) return rc;
  if (int rc = send(r, r.d_tags, tags)) return rc;
  if (int rc = rec_buf.allocate((8 * (size_t)nl + 3 * (size_t)d.num_materials) * sizeof(float4))) return rc;   // + the medium records: the caller refills them
  if (int rc = prims_buf.allocate(20 * (size_t)nl * sizeof(float4))) return rc;
  HIP_TRY(hipMemset(prims_buf.get(), 0, 20 * (size_t)nl * sizeof(float4) + (nl ? 0 : 16)));
  for (int l = 0; l < nl; l++)
    if (env_of[(size_t)l] >= 0) {
      if (int rc = send(r, rec_buf.get<float4>() + 8 * (size_t)l, (*envs)[(size_t)env_of[(size_t)l]].record, 8)) return rc;
    } else if (list[(size_t)l].l.instance < 0 && list[(size_t)l].l.sdf < 0)
      if (int rc = copy_on_device(rec_buf.get<float4>() + 8 * (size_t)l, d.light_rec + 8 * (size_t)list[(size_t)l].from, 8 * sizeof(float4))) return rc;
  LAUNCH(r, lit_records_kernel, nl, rec_buf.get<float4>(), lights_buf.get<vpt_light>(), r.d_tags.get<int>(), nl, cdf, d.instances, d.shapes, envs ? 1 : 0);
  HIP_TRY(hipDeviceSynchronize());   // nothing reads the old tables any more

  // 5. the handle
  const void* was[7] = {d.lights, d.light_cdf, d.light_index, d.light_index_pool, d.light_guide, d.light_rec, d.light_prims};
  d.lights = lights_buf.get<vpt_light>(), d.light_cdf = cdf, d.light_index = index_buf.get<DCdfIndex>(), d.light_index_pool = pool_buf.get<float>();
  d.light_guide = guide_buf.get<int2>(), d.light_rec = rec_buf.get<float4>(), d.light_prims = prims_buf.get<float4>(), d.num_lights = nl;
  device_buffer* fresh[7] = {&lights_buf, &cdf_buf, &index_buf, &pool_buf, &guide_buf, &rec_buf, &prims_buf};
  for (int k = 0; k < 7; k++) adopt(r.tables, was[k], std::move(*fresh[k]));
  u.num_cdf = num_cdf, u.num_pool = num_pool, u.num_guide = num_guide, u.light_index = index;
  u.lights = lights, u.light_kind.assign((size_t)nl, VPT_LIGHT_NONE), u.shape_lit.assign((size_t)d.num_shapes, 0);
  int features = 0;
  for (int l = 0; l < nl; l++) {
    const int kind = tags[(size_t)l] & 255;
    u.light_kind[(size_t)l] = kind;
    if (lights[(size_t)l].instance >= 0) u.shape_lit[(size_t)h.inst_shape[(size_t)lights[(size_t)l].instance]] = 1;
    features |= kind == VPT_LIGHT_LARGE_MESH ? VPT_FEAT_LARGE_LIGHTS : kind == VPT_LIGHT_SMALL_MESH ? VPT_FEAT_SMALL_LIGHTS : kind == VPT_LIGHT_SDF ? VPT_FEAT_SDF_LIGHTS : 0;
  }
  r.light_features = features;
  return VPT_OK;
}
