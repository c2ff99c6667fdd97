// vpt_texture_update.hip — environments and textures of a resident scene edited in place (include/vpt.h: vpt_scene_update_textures;
// DESIGN.md §15).  The texels and the entries are the edit's payload and go where vpt_scene_create would have put them (a texture that
// changes size or format: at the end of a pool allocated anew).  Of the light tables only an environment's CDF depends on texels:
// make_lights' weight per texel (yocto_pathtrace.cpp:1023-1030) is the one piece of arithmetic here, everything after it - the serial
// running sum, the 16-ary levels, the guide table, the records, the moves of the lights that stay - is vpt_light_update.hip's.
// Arithmetic = the reference's, operation by operation (-ffp-contract=off, correctly rounded /): max over all four channels in its
// select form, times the sine of the row.  The sine is the HOST's (glibc's, where make_lights computes it), one float per row.
#include <cmath>
#include <cstring>
#include <vector>

#include "vpt_error.h"
#include "vpt_texture_update.h"
#include "vpt_update_helpers.h"

namespace {

// ---- kernels --------------------------------------------------------------------------------------------------------------
__device__ inline float max_sel(float a, float b) { return (a > b) ? a : b; }   // yocto_math.h:1356: with NaN the select decides
__device__ inline float max4(float x, float y, float z, float w) { return max_sel(max_sel(max_sel(x, y), z), w); }   // yocto_math.h:1824

// one lane per texel, 16 bytes a lane: its weight into the slot its CDF entry will take
__global__ void tex_weights_float_kernel(const float4* __restrict__ texels, const float* __restrict__ sin_row, int width, int n, float* __restrict__ cdf) {
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;   // n < 2^31: the last block's lanes stay below 2^32
  if (idx >= (unsigned)n) return;
  const float4 v = texels[idx];
  cdf[idx] = max4(v.x, v.y, v.z, v.w) * sin_row[idx / (unsigned)width];
}
// the same for bytes: lookup_texture without as_linear is b / 255.0f per channel, not the sRGB table
__global__ void tex_weights_byte_kernel(const uchar4* __restrict__ texels, const float* __restrict__ sin_row, int width, int n, float* __restrict__ cdf) {
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (unsigned)n) return;
  const uchar4 b = texels[idx];
  cdf[idx] = max4((float)b.x / 255.0f, (float)b.y / 255.0f, (float)b.z / 255.0f, (float)b.w / 255.0f) * sin_row[idx / (unsigned)width];
}

// ---- host -----------------------------------------------------------------------------------------------------------------
constexpr float pif = (float)3.14159265358979323846;

int validate_edit(const DScene& d, const edit_mirrors& m, const vpt_texture_edit& e) {
  if (int rc = check_ids("environment", e.num_environments, e.environment_ids, e.environments, d.num_environments)) return rc;
  if (int rc = check_ids("texture", e.num_textures, e.texture_ids, e.textures, d.num_textures)) return rc;
  REQUIRE(e.num_texels_f >= 0 && (e.num_texels_f == 0 || e.texels_f), "edit: the float texel pool is null or has a negative count");
  REQUIRE(e.num_texels_b >= 0 && (e.num_texels_b == 0 || e.texels_b), "edit: the byte texel pool is null or has a negative count");
  for (int i = 0; i < e.num_environments; i++) {
    const vpt_environment& en = e.environments[i];
    REQUIRE(finite_all((const float*)&en.frame, 12) && finite_all(en.emission, 3), "edit: environment entry %d: a value is not finite", i);
    REQUIRE(en.emission_tex >= -1 && en.emission_tex < d.num_textures, "edit: environment entry %d: emission_tex %d is neither -1 nor a texture (%d)", i,
        en.emission_tex, d.num_textures);
  }
  for (int i = 0; i < e.num_textures; i++) {
    const vpt_texture& t = e.textures[i];
    REQUIRE(t.width >= 0 && t.height >= 0, "edit: texture entry %d: negative width or height (%d x %d)", i, t.width, t.height);
    const long long n = (long long)t.width * t.height;
    REQUIRE(n < (1ll << 31), "edit: texture entry %d: 2^31 texels or more", i);
    REQUIRE(t.offset >= 0 && t.offset + n <= (t.is_float ? e.num_texels_f : e.num_texels_b), "edit: texture entry %d: texels out of range of the edit's %s pool", i,
        t.is_float ? "float" : "byte");
  }
  // the scene as the edit leaves it: an emissive environment's texture holds texels (vpt_scene_create: cdf length = texel count > 0)
  std::vector<vpt_environment> envs = m.environments;
  std::vector<vpt_texture>     texs = m.textures;
  for (int i = 0; i < e.num_environments; i++) envs[(size_t)e.environment_ids[i]] = e.environments[i];
  for (int i = 0; i < e.num_textures; i++) texs[(size_t)e.texture_ids[i]] = e.textures[i];
  for (int i = 0; i < d.num_environments; i++) {
    const vpt_environment& en = envs[(size_t)i];
    if (!emissive(en) || en.emission_tex < 0) continue;
    const vpt_texture& t = texs[(size_t)en.emission_tex];
    REQUIRE((long long)t.width * t.height > 0, "edit: environment %d: its emission texture %d has no texels", i, en.emission_tex);
  }
  return VPT_OK;
}

}  // namespace

int launch_texel_weights(resident& r, const env_light& env, float* cdf) {
  const int n = env.cdf_len;   // (> 0: validation refuses an emissive environment whose texture has no texels)
  if (env.is_float) LAUNCH(r, tex_weights_float_kernel, n, (const float4*)env.texels, env.sin_row, env.width, n, cdf);
  else LAUNCH(r, tex_weights_byte_kernel, n, (const uchar4*)env.texels, env.sin_row, env.width, n, cdf);
  return VPT_OK;
}

int texture_update_apply(resident& r, const vpt_texture_edit& e, edit_outcome& out) {
  DScene&       d = r.d;
  edit_mirrors& m = r.m;
  if (int rc = validate_edit(d, m, e)) return rc;   // every refusal happens here: nothing has been written
  out.changed = true;   // (an edit without entries too: it starts the counters again)
  if (int rc = begin_update(r)) return rc;

  // 1. textures: in place where the room is the same, else at the end of a pool that grows
  std::vector<vpt_texture> textures = m.textures;
  std::vector<char>        edited((size_t)d.num_textures, 0);
  long long more_f = 0, more_b = 0;
  for (int i = 0; i < e.num_textures; i++) {
    const int          id  = e.texture_ids[i];
    const vpt_texture& was = m.textures[(size_t)id];
    vpt_texture&       t   = textures[(size_t)id];
    t = e.textures[i], t.is_float = t.is_float != 0, t.offset = was.offset, edited[(size_t)id] = 1;
    if (t.width == was.width && t.height == was.height && t.is_float == (was.is_float != 0)) continue;
    long long& more = t.is_float ? more_f : more_b;
    t.offset = (t.is_float ? m.num_texels_f : m.num_texels_b) + more;
    more += (long long)t.width * t.height;
  }
  if (more_f > 0)
    if (int rc = grow_pool(r, d.texels_f, m.num_texels_f, more_f)) return rc;
  if (more_b > 0)
    if (int rc = grow_pool(r, d.texels_b, m.num_texels_b, more_b)) return rc;
  for (int i = 0; i < e.num_textures; i++) {
    const int          id = e.texture_ids[i];
    const vpt_texture& t  = textures[(size_t)id];
    const size_t       n  = (size_t)t.width * (size_t)t.height;
    if (t.is_float) {
      if (int rc = send(r, d.texels_f + t.offset, (const float4*)e.texels_f + e.textures[i].offset, n)) return rc;
    } else if (int rc = send(r, d.texels_b + t.offset, (const uchar4*)e.texels_b + e.textures[i].offset, n)) return rc;
    if (int rc = send(r, d.textures + id, &t, 1)) return rc;
  }

  // 2. environments: the entry and its inverse frame
  const std::vector<vpt_environment> before = m.environments;
  std::vector<vpt_environment> environments = before;
  for (int i = 0; i < e.num_environments; i++) {
    const int id = e.environment_ids[i];
    float4 inv[3], fwd[3];
    prep_environment_frames(e.environments[i].frame, inv, fwd);
    if (int rc = send(r, d.environments + id, &e.environments[i], 1)) return rc;
    if (int rc = send(r, d.env_inv + 3 * (size_t)id, inv, 3)) return rc;
    environments[(size_t)id] = e.environments[i];
  }

  // 3. the environment lights of the edited scene (make_lights); a CDF is made anew when its light is new, its texture another
  //    one, or the texels were edited
  std::vector<env_light> envs;
  bool ask = e.num_environments > 0;
  long long rows = 0;
  for (int i = 0; i < d.num_environments; i++) {
    const vpt_environment &en = environments[(size_t)i], &was = before[(size_t)i];
    if (!emissive(en)) continue;
    env_light ev = {};
    ev.environment = i, ev.tag = en.emission_tex < 0 ? VPT_LIGHT_ENV_CONST : VPT_LIGHT_ENV_TEX;
    if (en.emission_tex >= 0) {
      const vpt_texture& t = textures[(size_t)en.emission_tex];
      ev.cdf_len = t.width * t.height, ev.width = t.width, ev.is_float = t.is_float;
      ev.texels    = t.is_float ? (const void*)(d.texels_f + t.offset) : (const void*)(d.texels_b + t.offset);
      ev.recompute = !emissive(was) || was.emission_tex != en.emission_tex || edited[(size_t)en.emission_tex];
      ask          = ask || edited[(size_t)en.emission_tex];
      if (ev.recompute) rows += t.height;
      prep_environment_frames(en.frame, &ev.record[0], &ev.record[3]);
      const int dims[2] = {t.width, t.height};
      memcpy(&ev.record[6].x, dims, 8);
    }
    memcpy(&ev.record[7].w, &ev.tag, 4);
    envs.push_back(ev);
  }
  if (ask) {
    // the rows' sines, where make_lights computes them: std::sin((j + 0.5f) * pif / height)
    std::vector<float> sines;
    sines.reserve((size_t)rows);
    std::vector<size_t> at(envs.size(), 0);
    for (size_t k = 0; k < envs.size(); k++) {
      if (!envs[k].recompute) continue;
      const int height = textures[(size_t)environments[(size_t)envs[k].environment].emission_tex].height;
      at[k] = sines.size();
      for (int j = 0; j < height; j++) sines.push_back(std::sin(((float)j + 0.5f) * pif / (float)height));
    }
    if (!sines.empty()) {
      if (int rc = send(r, r.d_sin, sines)) return rc;
      for (size_t k = 0; k < envs.size(); k++)
        if (envs[k].recompute) envs[k].sin_row = r.d_sin.get<float>() + at[k];
    }
    HIP_TRY(hipEventRecord(r.upd_ev0, 0));
    if (int rc = light_update_apply(r, vpt_scene_edit{}, &out.lights_rebuilt, &envs)) return rc;   // no vertex moved
    if (int rc = mark_end(r)) return rc;
    if (int rc = finish_update(r)) return rc;
    if (!out.lights_rebuilt)   // the list stays: of the records only the frames of a textured environment can have changed (build_lights)
      for (int l = 0; l < d.num_lights; l++) {
        const vpt_light& lt = m.lights[(size_t)l];
        if (lt.instance >= 0 || lt.sdf >= 0 || m.light_kind[(size_t)l] != VPT_LIGHT_ENV_TEX) continue;
        if (!memcmp(&environments[(size_t)lt.environment].frame, &before[(size_t)lt.environment].frame, sizeof(vpt_frame))) continue;
        float4 both[6];
        prep_environment_frames(environments[(size_t)lt.environment].frame, &both[0], &both[3]);
        if (int rc = send(r, d.light_rec + 8 * (size_t)l, both, 6)) return rc;
      }
  }
  HIP_TRY(hipDeviceSynchronize());
  m.textures = textures, m.environments = environments;
  return VPT_OK;
}
