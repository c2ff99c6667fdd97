// vpt_session.hip — progressive rendering on one GPU (include/vpt.h: vpt_session): the session, and nothing else.  It
// strings the device stages of csrc/vpt_frame_stages.hip together with vpt_render_device, vpt_resolve_device, vpt_denoise_device and
// the first-hit passes over buffers that stay in HBM.  Plain host code over the C-ABI: it sees a scene through its public calls only,
// holds no kernel and launches none itself.  Written once for every entry point: buffer_group (buffers sized together), id_frame and
// ensure_id_frame (the first-hit frame behind the picks, of either kind), fetch (what a getter hands out), the two tails of a frame.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

#include "vpt_device_buffer.h"
#include "vpt_error.h"
#include "vpt_frame_stages.h"   // check_display, state_init, vpt_pick_device
#include "vpt_layout.h"
#include "vpt_sdf_aov.h"   // vpt_sdf_pick_device

namespace {

using sized = std::pair<device_buffer*, size_t>;
int allocate_all(std::initializer_list<sized> list) {
  for (auto& [b, bytes] : list)
    if (int rc = b->allocate(bytes)) return rc;
  return VPT_OK;
}
// What a lazily made group of buffers was last sized for (0: nothing).  The key is the frame's pixel count AND its tile-major slot
// count: frames of equal pixels can differ in slots (105 x 40 and 100 x 42), and no rule has to know which planes are row-major.
struct buffer_group {
  long long pixels = 0, slots = 0;
  // nothing when the key is unchanged; else the group is empty while it allocates and takes the key once every allocation has
  // succeeded: a failed one leaves a group that the next use makes anew, never one that claims a size it does not have
  int ensure(long long for_pixels, long long for_slots, std::initializer_list<sized> list) {
    if (for_pixels == pixels && for_slots == slots) return VPT_OK;
    pixels = slots = 0;
    if (int rc = allocate_all(list)) return rc;
    pixels = for_pixels, slots = for_slots;
    return VPT_OK;
  }
};

// The id frame behind a pick and a get_ids: one sample of a first-hit pass in the pixel-centre branch at full resolution over a state
// of its own, made on first use after a reset and kept until the next one (every edit resets).
struct id_frame {
  buffer_group  group;
  device_buffer hits, rng, t_ids, t_aux;   // tile-major: the state of the pass and its two planes
  device_buffer ids, aux, pick;            // row-major: the two planes as get_ids fetches them; the bytes of a pick
  bool          valid = false;
};

}  // namespace

struct vpt_session {
  vpt_scene*         scene  = nullptr;
  int                device = 0;
  hipStream_t        st     = nullptr;
  vpt_session_params p      = {};
  int                width = 0, height = 0, pw = 0, ph = 0;   // the frame and its preview (width 0: a reset failed, no frame)
  int                samples = 0;
  vpt_layout         lay = {}, play = {};
  device_buffer      s_image, s_hits, s_rng;            // the pathtrace_state, tile-major (the guides are rendered in it first)
  device_buffer      p_image, p_hits, p_rng, p_rows;    // the preview's state and its get_render
  device_buffer      image, display_f, rgba8;           // row-major: linear image, the two displays
  buffer_group       staging;                           // made by get_state when first asked for
  device_buffer      r_image, r_hits, r_rng;            // row-major staging of get_state
  // denoise = 1 (made by allocate(), null while the session does not denoise)
  device_buffer normal, albedo, variance, sum_a, sum_n, filtered, scratch;
  device_buffer g_albedo;   // tile-major sums of the albedo guide (the normal guide's are rendered in s_image)
  bool          has_albedo = false, filtered_valid = false;
  int           a = 0;   // samples behind sum_a (0: none)
  // adaptive mode (vpt_session_set_adaptive): the run lives from the first advance after a reset to the next reset
  bool              adaptive = false;
  vpt_adaptive      ad       = {};
  vpt_adaptive_run* run      = nullptr;
  buffer_group      noise;                                // made by the advance that creates a run
  device_buffer     a_se2, a_var, a_hits, a_mean, a_m2;   // row-major planes of the run's statistics
  id_frame                  id_frames[2];   // [0] ids / uvt of vpt_render_aov_device for a mesh session, [1] ids / hit of vpt_render_sdf_aov_device for an implicit one
  std::vector<vpt_instance> instances;   // the scene's instance table as of the mesh id frame: a pick's shape and material
  // what the last call cost
  int     launches = 0;
  int64_t up = 0, down = 0;
};

namespace {

bool implicit_shader(int shader) { return shader == VPT_SHADER_IMPLICIT || shader == VPT_SHADER_IMPLICIT_NORMAL; }
// the volgrid shader has no first hit on a surface: no guides to filter with, nothing to pick, no id frame
bool volgrid_shader(int shader) { return shader == VPT_SHADER_VOLGRID; }
const char* const k_volgrid_refusal = "the session renders the volgrid shader: a medium has no surface to filter by, to pick or to name";

// what tells the two id frames apart
struct id_frame_kind {
  bool        implicit;                // the shader family it accepts; the other one: VPT_ERR_UNSUPPORTED with `refusal`
  const char *refusal, *aux_name;      // the second plane: its name in a message,
  size_t      aux_bytes, pick_bytes;   // its bytes per entry; the bytes of a pick
  int (*pass)(vpt_scene*, const vpt_params*, const vpt_layout*, void* d_ids, void* d_aux, void* d_hits, void* d_rng, void* stream);
  int (*resolve)(const vpt_layout*, const void* d_ids, const void* d_aux, void* d_ids_rowmajor, void* d_aux_rowmajor, void* stream);
  int (*pack)(const vpt_scene*, const void* d_ids_rowmajor, const void* d_aux_rowmajor, long long pixel, void* d_out, void* stream);
};
const id_frame_kind k_mesh_ids = {false, "the session renders an implicit shader: its picture is not what the mesh BVH holds",
    "uvt", 12, 24, [](vpt_scene* scene, const vpt_params* p, const vpt_layout* lay, void* ids, void* uvt, void* hits, void* rng, void* st) {
      const vpt_aov_planes planes = {nullptr, nullptr, nullptr, nullptr, ids, uvt};
      return vpt_render_aov_device(scene, p, lay, 1, &planes, hits, rng, st);
    }, vpt_resolve_ids_device, vpt_pick_device};
const id_frame_kind k_sdf_ids = {true, "the session renders a mesh shader: use vpt_session_pick / vpt_session_get_ids",
    "hit", 16, sizeof(vpt_sdf_pick), [](vpt_scene* scene, const vpt_params* p, const vpt_layout* lay, void* ids, void* hit, void* hits, void* rng, void* st) {
      const vpt_sdf_aov_planes planes = {nullptr, nullptr, nullptr, ids, hit};
      return vpt_render_sdf_aov_device(scene, p, lay, 1, &planes, hits, rng, st);
    }, vpt_resolve_sdf_ids_device, vpt_sdf_pick_device};
static_assert(sizeof(vpt_sdf_pick) == 48, "the 48 bytes of a pick");

// make_state's size rule (yocto_pathtrace.cpp:964-970)
void frame_size(int resolution, float aspect, int& width, int& height) {
  if (aspect >= 1) width = resolution, height = (int)std::round(resolution / aspect);
  else height = resolution, width = (int)std::round(resolution * aspect);
}

int check_session_params(const vpt_session_params* p) {
  REQUIRE(p, "null session params");
  if (!vpt_shader_known(p->render.shader)) return vpt_set_error(VPT_ERR_UNKNOWN_SHADER, "sampler unknown");
  REQUIRE(p->render.resolution >= 1 && p->render.resolution < 32768, "resolution %d outside 1..32767", p->render.resolution);
  REQUIRE(p->render.samples >= 1, "samples %d must be >= 1", p->render.samples);
  REQUIRE(p->render.bounces >= 0, "negative bounce count");
  REQUIRE(p->pratio >= 1 && p->pratio <= 64, "pratio %d outside 1..64", p->pratio);
  REQUIRE(p->render.resolution / p->pratio >= 1, "pratio %d leaves no preview of resolution %d", p->pratio, p->render.resolution);
  if (int rc = check_display(&p->display)) return rc;
  REQUIRE(p->denoise == 0 || p->denoise == 1, "denoise must be 0 or 1");
  if (p->denoise) {
    const vpt_denoise_params& f = p->filter;
    REQUIRE(f.iterations >= 1 && f.iterations <= 8, "iterations %d outside 1..8", f.iterations);
    REQUIRE(std::isfinite(f.sigma_luminance) && f.sigma_luminance > 0, "sigma_luminance must be finite and > 0");
    REQUIRE(std::isfinite(f.sigma_normal) && f.sigma_normal > 0, "sigma_normal must be finite and > 0");
    REQUIRE(std::isfinite(f.sigma_albedo) && f.sigma_albedo > 0, "sigma_albedo must be finite and > 0");
    REQUIRE(p->guide_samples >= 1, "guide_samples %d must be >= 1", p->guide_samples);
    if (volgrid_shader(p->render.shader)) return vpt_set_error(VPT_ERR_UNSUPPORTED, "denoise: %s", k_volgrid_refusal);
  }
  return VPT_OK;
}

void   begin_call(vpt_session* s) { s->launches = 0, s->up = 0, s->down = 0; }
size_t pixels(const vpt_session* s) { return (size_t)s->width * s->height; }

void drop_run(vpt_session* s) {
  if (s->run) vpt_adaptive_run_destroy(s->run);
  s->run = nullptr;
}
// vpt_session_set_adaptive's conditions, against the per-pixel cap `samples`
int check_session_adaptive(const vpt_adaptive* a, int samples) {
  REQUIRE(std::isfinite(a->threshold) && a->threshold >= 0, "adaptive threshold must be finite and >= 0");
  REQUIRE(a->step >= 1, "adaptive step must be >= 1");
  REQUIRE(a->min_samples >= 1 && a->min_samples <= samples, "adaptive min_samples must be in 1 .. render.samples (%d)", samples);
  return VPT_OK;
}

// A frame of another size, preview or denoise setting (reset decides): its own buffers and, if it denoises, the filter's.  Until all
// of them exist the session holds no frame.  The lazily made groups need no word here: their keys name the frame they were made for.
int allocate(vpt_session* s, int width, int height, int pw, int ph, bool denoise) {
  s->width = s->height = 0;
  const vpt_layout lay = {width, height, 8, 8, 0, 1}, play = {pw, ph, 8, 8, 0, 1};
  const long long  slots = vpt_layout_slots(&lay), pslots = vpt_layout_slots(&play);
  if (slots < 0 || pslots < 0) return VPT_ERR_INVALID_ARG;
  const size_t n = (size_t)width * height;
  if (int rc = allocate_all({{&s->s_image, (size_t)slots * 16}, {&s->s_hits, (size_t)slots * 4}, {&s->s_rng, (size_t)slots * 16},
          {&s->p_image, (size_t)pslots * 16}, {&s->p_hits, (size_t)pslots * 4}, {&s->p_rng, (size_t)pslots * 16}, {&s->p_rows, (size_t)pw * ph * 16},
          {&s->image, n * 16}, {&s->display_f, n * 16}, {&s->rgba8, n * 4}}))
    return rc;
  if (denoise) {
    if (int rc = allocate_all({{&s->normal, n * 16}, {&s->albedo, n * 16}, {&s->variance, n * 4}, {&s->sum_a, n * 16}, {&s->sum_n, n * 16},
            {&s->filtered, n * 16}, {&s->scratch, (size_t)vpt_denoise_scratch_bytes(width, height)}, {&s->g_albedo, (size_t)slots * 16}}))
      return rc;
  } else {
    for (device_buffer* b : {&s->normal, &s->albedo, &s->variance, &s->sum_a, &s->sum_n, &s->filtered, &s->scratch, &s->g_albedo}) *b = device_buffer();
  }
  s->lay = lay, s->play = play, s->width = width, s->height = height, s->pw = pw, s->ph = ph;
  return VPT_OK;
}

// `image` (or the filtered image, where the display shows it) -> both displays
int tonemap_display(vpt_session* s) {
  const void* src = s->filtered_valid ? s->filtered.get() : s->image.get();
  s->launches++;
  return vpt_tonemap_device(&s->p.display, s->width, s->height, src, s->display_f.get(), s->rgba8.get(), s->st);
}

// the tail of an advance: the filter if the session denoises - over `variance`, or over its spatial seed for null -, then the tone map
int filter_and_tonemap(vpt_session* s, const void* variance) {
  if (s->p.denoise) {
    if (int rc = vpt_denoise_device(&s->p.filter, s->width, s->height, s->image.get(), s->normal.get(), s->has_albedo ? s->albedo.get() : nullptr,
            variance, s->filtered.get(), s->scratch.get(), s->st))
      return rc;
    s->filtered_valid = true, s->launches++;
  }
  return tonemap_display(s);
}

// after the implicit kernels ran: wait for them and read their watchdog's word (the mesh shaders have none: the call stays asynchronous)
int check_implicit_watchdog(vpt_session* s) {
  if (!implicit_shader(s->p.render.shader) && !volgrid_shader(s->p.render.shader)) return VPT_OK;   // (K3 reports through the same word)
  HIP_TRY(hipStreamSynchronize(s->st));
  if (int rc = vpt_check_watchdog(s->scene)) return rc;
  s->down += 4;
  return VPT_OK;
}

// one guide: `samples` passes of `shader` over a state initialised on the device (in the session's own state buffers), get_render
int render_guide(vpt_session* s, int shader, void* d_out) {
  vpt_params p = s->p.render;
  p.shader = shader, p.samples = s->p.guide_samples;
  if (int rc = vpt_state_init_device(&s->lay, s->s_image.get(), s->s_hits.get(), s->s_rng.get(), s->st)) return rc;
  if (int rc = vpt_render_device(s->scene, &p, &s->lay, p.samples, s->s_image.get(), s->s_hits.get(), s->s_rng.get(), s->st)) return rc;
  s->launches += 3;
  return vpt_resolve_device(&s->lay, s->s_image.get(), p.samples, d_out, s->st);
}

// both guides of the mesh shaders from one first-hit pass (include/vpt.h: vpt_render_aov_device): `normal` and `color` trace the same
// rays from the same streams, so one traversal per sample serves both; the bits are those of two calls of render_guide
int render_mesh_guides(vpt_session* s) {
  vpt_params p = s->p.render;
  p.samples    = s->p.guide_samples;
  if (int rc = vpt_state_init_device(&s->lay, s->s_image.get(), s->s_hits.get(), s->s_rng.get(), s->st)) return rc;   // zeroes s_image
  HIP_TRY(hipMemsetAsync(s->g_albedo.get(), 0, (size_t)vpt_layout_slots(&s->lay) * 16, s->st));
  const vpt_aov_planes planes = {s->s_image.get(), s->g_albedo.get(), nullptr, nullptr, nullptr, nullptr};
  if (int rc = vpt_render_aov_device(s->scene, &p, &s->lay, p.samples, &planes, s->s_hits.get(), s->s_rng.get(), s->st)) return rc;
  if (int rc = vpt_resolve_device(&s->lay, s->s_image.get(), p.samples, s->normal.get(), s->st)) return rc;
  s->launches += 4;
  return vpt_resolve_device(&s->lay, s->g_albedo.get(), p.samples, s->albedo.get(), s->st);
}

// The id frame of kind `k` (include/vpt.h: vpt_session_pick, vpt_session_pick_sdf), made unless the session holds it: state init, one
// sample of the kind's pass, its resolve; the state and the tile-major planes hold one entry per SLOT, the row-major ones per pixel.
int ensure_id_frame(vpt_session* s, const id_frame_kind& k) {
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  if (volgrid_shader(s->p.render.shader)) return vpt_set_error(VPT_ERR_UNSUPPORTED, "%s", k_volgrid_refusal);
  if (implicit_shader(s->p.render.shader) != k.implicit) return vpt_set_error(VPT_ERR_UNSUPPORTED, "%s", k.refusal);
  id_frame& f = s->id_frames[k.implicit];
  if (f.valid) return VPT_OK;
  const size_t n = pixels(s), slots = (size_t)vpt_layout_slots(&s->lay);
  if (int rc = f.group.ensure((long long)n, (long long)slots,
          {{&f.hits, slots * 4}, {&f.rng, slots * 16}, {&f.t_ids, slots * 8}, {&f.t_aux, slots * k.aux_bytes}, {&f.ids, n * 8}, {&f.aux, n * k.aux_bytes},
              {&f.pick, k.pick_bytes}}))
    return rc;
  vpt_params p = s->p.render;
  p.samples    = 1;
  if (int rc = state_init(&s->lay, nullptr, f.hits.get(), f.rng.get(), s->st)) return rc;
  if (int rc = k.pass(s->scene, &p, &s->lay, f.t_ids.get(), f.t_aux.get(), f.hits.get(), f.rng.get(), s->st)) return rc;
  if (int rc = k.resolve(&s->lay, f.t_ids.get(), f.t_aux.get(), f.ids.get(), f.aux.get(), s->st)) return rc;
  s->launches += 3;
  if (!k.implicit) {   // the mesh kind alone: a pick's shape and material are those of the instance table as it stands now, read once per id frame
    int count = 0;
    if (int rc = vpt_scene_get_instances(s->scene, nullptr, 0, &count)) return rc;
    s->instances.resize((size_t)count);
    if (int rc = vpt_scene_get_instances(s->scene, s->instances.data(), count, nullptr)) return rc;
    s->down += (int64_t)count * (int64_t)sizeof(vpt_instance);
  }
  f.valid = true;
  return VPT_OK;
}

int reset(vpt_session* s, const vpt_session_params& np) {
  vpt_camera cam;
  if (int rc = vpt_scene_get_camera(s->scene, np.render.camera, &cam)) return rc;
  s->down += sizeof(vpt_camera);
  int width = 0, height = 0, pw = 0, ph = 0;
  frame_size(np.render.resolution, cam.aspect, width, height);
  frame_size(np.render.resolution / np.pratio, cam.aspect, pw, ph);
  REQUIRE(width >= 1 && height >= 1 && pw >= 1 && ph >= 1, "camera aspect %g leaves an empty frame (%d x %d, preview %d x %d)", (double)cam.aspect,
      width, height, pw, ph);
  HIP_TRY(hipStreamSynchronize(s->st));   // nothing of the previous frame is in flight when its buffers go
  drop_run(s);                            // an adaptive run ends here; the first advance makes the next
  if (width != s->width || height != s->height || pw != s->pw || ph != s->ph || (np.denoise != 0) != (s->normal.get() != nullptr))   // (the filter's buffers exist)
    if (int rc = allocate(s, width, height, pw, ph, np.denoise != 0)) return rc;
  s->p = np, s->samples = 0, s->a = 0, s->filtered_valid = false, s->has_albedo = false, s->id_frames[0].valid = s->id_frames[1].valid = false;
  if (np.denoise) {
    if (implicit_shader(np.render.shader)) {
      if (int rc = render_guide(s, VPT_SHADER_IMPLICIT_NORMAL, s->normal.get())) return rc;
    } else {
      if (int rc = render_mesh_guides(s)) return rc;
      s->has_albedo = true;
    }
  }
  if (int rc = vpt_state_init_device(&s->lay, s->s_image.get(), s->s_hits.get(), s->s_rng.get(), s->st)) return rc;
  // the preview: a fresh state of resolution / pratio, samples = 1 (the pixel-centre branch), resolved and replicated
  vpt_params pp = np.render;
  pp.resolution = np.render.resolution / np.pratio, pp.samples = 1;
  if (int rc = vpt_state_init_device(&s->play, s->p_image.get(), s->p_hits.get(), s->p_rng.get(), s->st)) return rc;
  if (int rc = vpt_render_device(s->scene, &pp, &s->play, 1, s->p_image.get(), s->p_hits.get(), s->p_rng.get(), s->st)) return rc;
  if (int rc = vpt_resolve_device(&s->play, s->p_image.get(), 1, s->p_rows.get(), s->st)) return rc;
  if (int rc = vpt_upscale_device(np.pratio, pw, ph, s->p_rows.get(), width, height, s->image.get(), s->st)) return rc;
  s->launches += 5;
  if (int rc = tonemap_display(s)) return rc;
  return check_implicit_watchdog(s);
}

// What a getter hands out: on the session's device, every plane of the list whose host pointer is not null, counted in bytes_to_host,
// then the synchronise.  The getter has checked its preconditions and begun the call.
struct fetch_plane { void* host; const device_buffer* from; size_t bytes; };
int fetch(vpt_session* s, std::initializer_list<fetch_plane> planes) {
  HIP_TRY(hipSetDevice(s->device));
  for (const fetch_plane& f : planes) {
    if (!f.host) continue;
    HIP_TRY(hipMemcpyAsync(f.host, f.from->get(), f.bytes, hipMemcpyDeviceToHost, s->st));
    s->down += (int64_t)f.bytes;
  }
  HIP_TRY(hipStreamSynchronize(s->st));
  return VPT_OK;
}

// vpt_session_advance in adaptive mode (include/vpt.h): whole rounds of the run, the per-pixel resolve, the noise planes, the filter
// with the handed-over variance, the tone map
int advance_adaptive(vpt_session* s, int nsamples) {
  const int want = (int)(((long long)nsamples + s->ad.step - 1) / s->ad.step);
  if (want <= 0) return VPT_OK;
  HIP_TRY(hipSetDevice(s->device));
  void *img = s->s_image.get(), *hit = s->s_hits.get(), *rng = s->s_rng.get();
  const size_t n = pixels(s);
  if (!s->run) {
    if (int rc = s->noise.ensure((long long)n, vpt_layout_slots(&s->lay),
            {{&s->a_se2, n * 4}, {&s->a_var, n * 4}, {&s->a_hits, n * 4}, {&s->a_mean, n * 4}, {&s->a_m2, n * 4}}))
      return rc;
    if (int rc = vpt_adaptive_run_create(s->scene, &s->p.render, &s->ad, &s->lay, img, hit, rng, s->st, &s->run)) return rc;
    s->launches++, s->down += 16;
  }
  int     done = 0, active = 0, rounds = 0, hits = 0;
  int64_t taken = 0;
  if (int rc = vpt_adaptive_run_rounds(s->run, want, &done, &taken, &active)) return rc;
  if (done == 0) return VPT_OK;   // every pixel has stopped: nothing was enqueued, state and displays stay
  s->launches += done, s->down += (implicit_shader(s->p.render.shader) ? 20 : 16) * (int64_t)done;   // the read-back, the watchdog's word
  if (int rc = vpt_adaptive_run_progress(s->run, &rounds, nullptr, nullptr, &hits)) return rc;
  s->samples = hits;
  if (int rc = vpt_resolve_hits_device(&s->lay, img, hit, s->image.get(), s->st)) return rc;
  if (int rc = vpt_adaptive_run_noise_device(s->run, s->a_se2.get(), s->a_hits.get(), s->st)) return rc;
  if (int rc = vpt_box3_device(s->width, s->height, s->a_se2.get(), s->a_var.get(), s->st)) return rc;
  s->launches += 3;
  return filter_and_tonemap(s, rounds >= 2 ? s->a_var.get() : nullptr);
}

// one of the edits of a resident scene - apply(scene, edit) is its vpt_scene_* entry point - then a reset
template <class Edit, class Apply>
int session_edit(vpt_session* s, const Edit* edit, Apply apply) {
  REQUIRE(s && edit, "null argument");
  begin_call(s);
  if (int rc = apply(s->scene, edit)) return rc;   // a refused edit has changed nothing, here or there
  int     launches = 0;
  int64_t bytes    = 0;
  float   ms       = 0;
  if (vpt_scene_update_stats(s->scene, &launches, &bytes, &ms) == VPT_OK) s->launches += launches, s->up += bytes;
  return reset(s, s->p);
}

// vpt_session_get_ids and vpt_session_get_sdf_ids: the row-major planes of the id frame of kind `k`
int get_id_frame(vpt_session* s, const id_frame_kind& k, void* ids, void* aux) {
  REQUIRE(s, "null session");
  REQUIRE(ids || aux, "null ids and %s: nothing to fetch", k.aux_name);
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  if (int rc = ensure_id_frame(s, k)) return rc;
  const id_frame& f = s->id_frames[k.implicit];
  return fetch(s, {{ids, &f.ids, pixels(s) * 8}, {aux, &f.aux, pixels(s) * k.aux_bytes}});
}

// vpt_session_pick and vpt_session_pick_sdf around their unpack: the checks, the id frame of kind `k`, its pack of pixel (x, y) in one
// launch, the record's bytes into `record`
int pick_record(vpt_session* s, const id_frame_kind& k, int x, int y, void* record) {
  REQUIRE(s && record, "null argument");
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  REQUIRE(x >= 0 && x < s->width && y >= 0 && y < s->height, "pixel (%d, %d) outside the %d x %d frame", x, y, s->width, s->height);
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  if (int rc = ensure_id_frame(s, k)) return rc;
  const id_frame& f = s->id_frames[k.implicit];
  if (int rc = k.pack(s->scene, f.ids.get(), f.aux.get(), (long long)y * s->width + x, f.pick.get(), s->st)) return rc;
  s->launches++;
  return fetch(s, {{record, &f.pick, k.pick_bytes}});
}

}  // namespace

extern "C" {

int vpt_session_create(vpt_scene* scene, const vpt_session_params* params, vpt_session** out) {
  REQUIRE(scene && out, "null argument");
  *out = nullptr;
  if (int rc = check_session_params(params)) return rc;
  const int device = vpt_scene_get_device(scene);
  if (device < 0) return device;
  HIP_TRY(hipSetDevice(device));
  vpt_session* s = new vpt_session{};
  s->scene = scene, s->device = device;
  struct guard { vpt_session*& s; ~guard() { if (s) vpt_session_destroy(s); } } g{s};
  HIP_TRY(hipStreamCreate(&s->st));
  if (int rc = reset(s, *params)) return rc;
  *out = s;
  s    = nullptr;   // release the guard
  return VPT_OK;
}

void vpt_session_destroy(vpt_session* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);   // the buffers are freed on the session's device
  drop_run(s);
  if (s->st) (void)hipStreamSynchronize(s->st), (void)hipStreamDestroy(s->st);
  delete s;
}

int vpt_session_reset(vpt_session* s, const vpt_session_params* params_or_null) {
  REQUIRE(s, "null session");
  if (params_or_null)
    if (int rc = check_session_params(params_or_null)) return rc;
  if (params_or_null && s->adaptive)
    if (int rc = check_session_adaptive(&s->ad, params_or_null->render.samples)) return rc;
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  const vpt_session_params np = params_or_null ? *params_or_null : s->p;
  return reset(s, np);
}

int vpt_session_advance(vpt_session* s, int nsamples) {
  REQUIRE(s, "null session");
  REQUIRE(nsamples >= 0, "negative sample count");
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  begin_call(s);
  if (s->adaptive) return advance_adaptive(s, nsamples);
  const int todo = std::min(nsamples, s->p.render.samples - s->samples);   // a no-op once reached, yocto_pathtrace.cpp:1055
  if (todo <= 0) return VPT_OK;
  HIP_TRY(hipSetDevice(s->device));
  void *img = s->s_image.get(), *hit = s->s_hits.get(), *rng = s->s_rng.get();
  if (s->p.denoise && s->samples > 0 && s->samples >= 2 * s->a) {   // the variance rule of include/vpt.h: keep the sums of the first half
    if (int rc = vpt_resolve_device(&s->lay, img, 1, s->sum_a.get(), s->st)) return rc;   // * (1 / 1): the sums themselves, row-major
    s->a = s->samples, s->launches++;
  }
  if (int rc = vpt_render_device(s->scene, &s->p.render, &s->lay, todo, img, hit, rng, s->st)) return rc;
  s->samples += todo;
  if (int rc = vpt_resolve_device(&s->lay, img, s->samples, s->image.get(), s->st)) return rc;
  s->launches += 2;
  if (s->a > 0) {   // (only a denoising session keeps sums)
    if (int rc = vpt_resolve_device(&s->lay, img, 1, s->sum_n.get(), s->st)) return rc;
    if (int rc = vpt_half_variance_device(s->width, s->height, s->sum_a.get(), s->a, s->sum_n.get(), s->samples, s->variance.get(), s->st)) return rc;
    s->launches += 2;
  }
  if (int rc = filter_and_tonemap(s, s->a > 0 ? s->variance.get() : nullptr)) return rc;
  return check_implicit_watchdog(s);
}

int vpt_session_set_display(vpt_session* s, const vpt_display_params* display) {
  REQUIRE(s, "null session");
  if (int rc = check_display(display)) return rc;
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  s->p.display = *display;
  return tonemap_display(s);
}

int vpt_session_edit(vpt_session* s, const vpt_scene_edit* edit) { return session_edit(s, edit, vpt_scene_update); }
int vpt_session_edit_lights(vpt_session* s, const vpt_scene_edit* edit) { return session_edit(s, edit, vpt_scene_update_lights); }
int vpt_session_edit_textures(vpt_session* s, const vpt_texture_edit* edit) { return session_edit(s, edit, vpt_scene_update_textures); }
int vpt_session_edit_volumes(vpt_session* s, const vpt_volume_edit* edit) { return session_edit(s, edit, vpt_scene_update_volumes); }
int vpt_session_sculpt_volumes(vpt_session* s, const vpt_sculpt_edit* edit) { return session_edit(s, edit, vpt_scene_sculpt_volumes); }
int vpt_session_edit_volume_set(vpt_session* s, const vpt_volume_set_edit* edit) { return session_edit(s, edit, vpt_scene_update_volume_set); }
int vpt_session_rebuild_bvh(vpt_session* s, const vpt_bvh_rebuild* what) { return vpt_session_rebuild_bvh_quality(s, what, VPT_BVH_MIDDLE); }
int vpt_session_rebuild_bvh_quality(vpt_session* s, const vpt_bvh_rebuild* what, int quality) {
  return session_edit(s, what, [quality](vpt_scene* scene, const vpt_bvh_rebuild* w) { return vpt_scene_rebuild_bvh_quality(scene, w, quality); });
}
int vpt_session_edit_instances(vpt_session* s, const vpt_instance_edit* edit) { return session_edit(s, edit, vpt_scene_update_instances); }
int vpt_session_edit_shapes(vpt_session* s, const vpt_shape_edit* edit) { return session_edit(s, edit, vpt_scene_update_shapes); }
int vpt_session_edit_subdivs(vpt_session* s, const vpt_subdiv_edit* edit) { return session_edit(s, edit, vpt_scene_update_subdivs); }

int vpt_session_get_display(vpt_session* s, uint8_t* rgba8, float* display_f) {
  REQUIRE(s, "null session");
  REQUIRE(rgba8 || display_f, "null rgba8 and display_f: nothing to fetch");
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  begin_call(s);
  return fetch(s, {{rgba8, &s->rgba8, pixels(s) * 4}, {display_f, &s->display_f, pixels(s) * 16}});
}

int vpt_session_get_image(vpt_session* s, float* linear) {
  REQUIRE(s && linear, "null argument");
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  begin_call(s);
  return fetch(s, {{linear, &s->image, pixels(s) * 16}});
}

int vpt_session_get_denoised(vpt_session* s, float* linear) {
  REQUIRE(s && linear, "null argument");
  if (volgrid_shader(s->p.render.shader)) return vpt_set_error(VPT_ERR_UNSUPPORTED, "denoise: %s", k_volgrid_refusal);
  REQUIRE(s->filtered_valid, "no filtered image: the session needs denoise = 1 and an advance since its last reset");
  begin_call(s);
  return fetch(s, {{linear, &s->filtered, pixels(s) * 16}});
}

int vpt_session_get_state(vpt_session* s, float* image_rgba, int32_t* hits, uint64_t* rng, int* samples) {
  REQUIRE(s && image_rgba && hits && rng && samples, "null argument");
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  const size_t n = pixels(s);
  if (int rc = s->staging.ensure((long long)n, vpt_layout_slots(&s->lay), {{&s->r_image, n * 16}, {&s->r_hits, n * 4}, {&s->r_rng, n * 16}})) return rc;
  // the one-rank layout owns every pixel: the row-major staging is written in full
  const layout_plane state[3] = {{s->s_image.get(), s->r_image.get(), 16}, {s->s_hits.get(), s->r_hits.get(), 4}, {s->s_rng.get(), s->r_rng.get(), 16}};
  if (int rc = layout_copy(&s->lay, LAYOUT_TILES_TO_ROWS, state, 3, s->st)) return rc;
  s->launches++;
  if (int rc = fetch(s, {{image_rgba, &s->r_image, n * 16}, {hits, &s->r_hits, n * 4}, {rng, &s->r_rng, n * 16}})) return rc;
  *samples = s->samples;
  return VPT_OK;
}

int vpt_session_get_guides(vpt_session* s, float* normal, float* albedo) {
  REQUIRE(s, "null session");
  REQUIRE(normal || albedo, "null normal and albedo: nothing to fetch");
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  if (volgrid_shader(s->p.render.shader)) return vpt_set_error(VPT_ERR_UNSUPPORTED, "guides: %s", k_volgrid_refusal);
  REQUIRE(s->p.denoise, "no guides: the session needs denoise = 1");
  REQUIRE(!albedo || s->has_albedo, "no albedo guide: the implicit shaders have none");
  begin_call(s);
  return fetch(s, {{normal, &s->normal, pixels(s) * 16}, {albedo, &s->albedo, pixels(s) * 16}});
}

int vpt_session_get_ids(vpt_session* s, int32_t* ids, float* uvt) { return get_id_frame(s, k_mesh_ids, ids, uvt); }

int vpt_session_pick(vpt_session* s, int x, int y, vpt_pick* out) {
  struct { int32_t hit, instance, element; float u, v, distance; } rec;
  static_assert(sizeof(rec) == 24, "the 24 bytes of a pick");
  REQUIRE(out, "null argument");
  if (int rc = pick_record(s, k_mesh_ids, x, y, &rec)) return rc;
  *out = {rec.hit, rec.instance, rec.element, -1, -1, rec.u, rec.v, rec.distance};
  if (rec.hit && (size_t)rec.instance < s->instances.size()) out->shape = s->instances[(size_t)rec.instance].shape, out->material = s->instances[(size_t)rec.instance].material;
  return VPT_OK;
}

int vpt_session_get_sdf_ids(vpt_session* s, int32_t* ids, float* hit) { return get_id_frame(s, k_sdf_ids, ids, hit); }

// the record crosses as it is: vpt_sdf_pick_device packs a vpt_sdf_pick
int vpt_session_pick_sdf(vpt_session* s, int x, int y, vpt_sdf_pick* out) { return pick_record(s, k_sdf_ids, x, y, out); }

int vpt_session_set_adaptive(vpt_session* s, const vpt_adaptive* a) {
  REQUIRE(s, "null session");
  if (a)
    if (int rc = check_session_adaptive(a, s->p.render.samples)) return rc;
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  s->adaptive = a != nullptr;
  if (a) s->ad = *a;
  return reset(s, s->p);
}

int vpt_session_progress(const vpt_session* s, int* rounds, int64_t* rendered, int* active) {
  REQUIRE(s, "null session");
  REQUIRE(s->adaptive, "the session is not in adaptive mode");
  if (s->run) return vpt_adaptive_run_progress(s->run, rounds, rendered, active, nullptr);
  if (rounds) *rounds = 0;
  if (rendered) *rendered = 0;
  if (active) *active = s->width * s->height;   // nothing has rendered: every pixel is to
  return VPT_OK;
}

int vpt_session_get_hits(vpt_session* s, int32_t* hits) {
  REQUIRE(s && hits, "null argument");
  REQUIRE(s->adaptive, "the session is not in adaptive mode");
  REQUIRE(s->width > 0, "the session holds no frame (a reset failed)");
  begin_call(s);
  if (!s->run) {
    memset(hits, 0, pixels(s) * 4);
    return VPT_OK;
  }
  return fetch(s, {{hits, &s->a_hits, pixels(s) * 4}});
}

int vpt_session_get_noise(vpt_session* s, float* se2, float* variance) {
  REQUIRE(s, "null session");
  REQUIRE(se2 || variance, "null se2 and variance: nothing to fetch");
  REQUIRE(s->adaptive, "the session is not in adaptive mode");
  REQUIRE(s->run, "no noise estimate: no advance has run since the last reset");
  begin_call(s);
  return fetch(s, {{se2, &s->a_se2, pixels(s) * 4}, {variance, &s->a_var, pixels(s) * 4}});
}

int vpt_session_get_adaptive_stats(vpt_session* s, float* mean, float* m2) {
  REQUIRE(s && mean && m2, "null argument");
  REQUIRE(s->adaptive, "the session is not in adaptive mode");
  REQUIRE(s->run, "no statistics: no advance has run since the last reset");
  HIP_TRY(hipSetDevice(s->device));
  begin_call(s);
  if (int rc = vpt_adaptive_run_stats_device(s->run, s->a_mean.get(), s->a_m2.get(), s->st)) return rc;
  s->launches++;
  return fetch(s, {{mean, &s->a_mean, pixels(s) * 4}, {m2, &s->a_m2, pixels(s) * 4}});
}

int vpt_session_size(const vpt_session* s, int* width, int* height) {
  REQUIRE(s && width && height, "null argument");
  *width = s->width, *height = s->height;
  return VPT_OK;
}

int vpt_session_samples(const vpt_session* s) { return s ? s->samples : vpt_set_error(VPT_ERR_INVALID_ARG, "null session"); }

int vpt_session_stats(const vpt_session* s, int* launches, int64_t* bytes_to_device, int64_t* bytes_to_host) {
  REQUIRE(s && launches && bytes_to_device && bytes_to_host, "null argument");
  *launches = s->launches, *bytes_to_device = s->up, *bytes_to_host = s->down;
  return VPT_OK;
}

}  // extern "C"
