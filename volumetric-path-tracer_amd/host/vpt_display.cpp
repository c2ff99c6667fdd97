// vpt_display.cpp — the display stages of the reference on the host (host/vpt_host.h): tonemap_image, the preview's replication, make_state's
// seeds restated through the jump header the device compiles, and render_session, a thin owner of a vpt_scene and its vpt_session.
// The tone map is the rule of include/vpt.h (vpt_tonemap_device) in the reference's operation order; nothing here renders.
#include <cmath>
#include <cstring>
#include <stdexcept>

#include "vpt_host.h"
#include "vpt_rng_jump.h"

namespace vpt {

namespace {
float srgb_curve(float rgb) { return (rgb <= 0.0031308f) ? 12.92f * rgb : (1 + 0.055f) * std::pow(rgb, 1 / 2.4f) - 0.055f; }   // yocto_color.h:228-231
float filmic_curve(float c) {   // tonemap_filmic, :274-280, without accurate_fit
  auto h   = c * 0.6f;
  auto ldr = ((h * h) * 2.51f + h * 0.03f) / (((h * h) * 2.43f + h * 0.59f) + 0.14f);
  return (0 < ldr) ? ldr : 0.0f;   // max(0, ldr) of yocto_math.h
}
vec4f tonemap(const vec4f& hdr, float exposure, bool filmic, bool srgb) {   // :306-316
  auto c = hdr;
  if (exposure != 0) {
    auto scale = std::exp2(exposure);
    c.x = c.x * scale, c.y = c.y * scale, c.z = c.z * scale;
  }
  if (filmic) c.x = filmic_curve(c.x), c.y = filmic_curve(c.y), c.z = filmic_curve(c.z);
  if (srgb) c.x = srgb_curve(c.x), c.y = srgb_curve(c.y), c.z = srgb_curve(c.z);
  return c;
}
uint8_t float_to_byte(float a) {   // :207-211
  auto v = (int)(a * 256);
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
[[noreturn]] void fail(const char* what) { throw std::runtime_error{string{what} + ": " + vpt_last_error()}; }
}  // namespace

void tonemap_image(vector<vec4f>& ldr, const vector<vec4f>& hdr, float exposure, bool filmic, bool srgb) {
  ldr.resize(hdr.size());
  for (size_t i = 0; i < hdr.size(); i++) ldr[i] = tonemap(hdr[i], exposure, filmic, srgb);
}
void tonemap_image(vector<vec4b>& ldr, const vector<vec4f>& hdr, float exposure, bool filmic, bool srgb) {
  ldr.resize(hdr.size());
  for (size_t i = 0; i < hdr.size(); i++) {
    auto c = tonemap(hdr[i], exposure, filmic, srgb);
    ldr[i] = {float_to_byte(c.x), float_to_byte(c.y), float_to_byte(c.z), float_to_byte(c.w)};
  }
}

void upscale_preview(color_image& out, const color_image& preview, int pratio, int width, int height) {
  if (pratio < 1 || width < 1 || height < 1 || preview.width < 1 || preview.height < 1 ||
      preview.pixels.size() != (size_t)preview.width * preview.height)
    throw std::invalid_argument{"bad preview, size or ratio"};
  out.width = width, out.height = height, out.linear = preview.linear;
  out.pixels.resize((size_t)width * height);
  for (auto j = 0; j < height; j++)
    for (auto i = 0; i < width; i++) {
      auto pi = std::min(i / pratio, preview.width - 1), pj = std::min(j / pratio, preview.height - 1);
      out.pixels[(size_t)j * width + i] = preview.pixels[(size_t)pj * preview.width + pi];
    }
}

vector<rng_state> make_state_rngs_jump(int width, int height) {
  if (width < 1 || height < 1) throw std::invalid_argument{"bad state size"};
  auto rngs = vector<rng_state>((size_t)width * height);
  for (size_t idx = 0; idx < rngs.size(); idx++) {
    auto r    = vpt_state_pixel_rng_at(idx);
    rngs[idx] = {r.state, r.inc};
  }
  return rngs;
}

// ---- render_session -----------------------------------------------------------------------------------------------------------
static vpt_session_params session_abi(const render_session_params& p) {
  auto abi          = vpt_session_params{};
  abi.render        = to_abi(p.render);
  abi.pratio        = p.render.pratio;
  abi.display       = {p.render.exposure, p.render.filmic ? 1 : 0, 1};
  abi.denoise       = p.denoise ? 1 : 0;
  abi.filter        = {p.filter.iterations, p.filter.sigma_luminance, p.filter.sigma_normal, p.filter.sigma_albedo};
  abi.guide_samples = p.guide_samples;
  return abi;
}

render_session::render_session(const scene_data& scene, const bvh_scene& bvh, const pathtrace_lights& lights, const render_session_params& params,
    int device) {
  auto flat = flat_scene{};
  flatten_scene(flat, scene, bvh, lights);
  if (vpt_scene_create_curves(&flat.desc, flat.curves_or_null(), device, &scene_) != VPT_OK) fail("vpt_scene_create");
  auto abi = session_abi(params);
  if (vpt_session_create(scene_, &abi, &session_) != VPT_OK) {
    auto message = string{"vpt_session_create: "} + vpt_last_error();
    vpt_scene_destroy(scene_);
    throw std::runtime_error{message};
  }
}
render_session::~render_session() {
  vpt_session_destroy(session_);
  vpt_scene_destroy(scene_);
}
void render_session::reset() {
  if (vpt_session_reset(session_, nullptr) != VPT_OK) fail("vpt_session_reset");
}
void render_session::reset(const render_session_params& params) {
  auto abi = session_abi(params);
  if (vpt_session_reset(session_, &abi) != VPT_OK) fail("vpt_session_reset");
}
void render_session::advance(int nsamples) {
  if (vpt_session_advance(session_, nsamples) != VPT_OK) fail("vpt_session_advance");
}
void render_session::set_display(float exposure, bool filmic) {
  auto display = vpt_display_params{exposure, filmic ? 1 : 0, 1};
  if (vpt_session_set_display(session_, &display) != VPT_OK) fail("vpt_session_set_display");
}
void render_session::set_adaptive(const pathtrace_adaptive_params& adaptive) {
  auto abi = vpt_adaptive{adaptive.threshold, adaptive.min_samples, adaptive.step};
  if (vpt_session_set_adaptive(session_, adaptive.threshold < 0 ? nullptr : &abi) != VPT_OK) fail("vpt_session_set_adaptive");
}
render_session::progress_stats render_session::progress() const {
  auto out = progress_stats{};
  if (vpt_session_progress(session_, &out.rounds, &out.samples, &out.active) != VPT_OK) fail("vpt_session_progress");
  return out;
}
bool        render_session::converged() const { return progress().active == 0; }
vector<int> render_session::hits() {
  auto out = vector<int>((size_t)width() * height());
  if (vpt_session_get_hits(session_, out.data()) != VPT_OK) fail("vpt_session_get_hits");
  return out;
}
int render_session::width() const {
  auto w = 0, h = 0;
  vpt_session_size(session_, &w, &h);
  return w;
}
int render_session::height() const {
  auto w = 0, h = 0;
  vpt_session_size(session_, &w, &h);
  return h;
}
int render_session::samples() const { return vpt_session_samples(session_); }
vector<vec4b> render_session::display() {
  auto out = vector<vec4b>((size_t)width() * height());
  if (vpt_session_get_display(session_, &out.data()->x, nullptr) != VPT_OK) fail("vpt_session_get_display");
  return out;
}
color_image render_session::image(bool denoised) {
  auto out = color_image{width(), height(), true, {}};
  out.pixels.resize((size_t)out.width * out.height);
  auto rc = denoised ? vpt_session_get_denoised(session_, &out.pixels.data()->x) : vpt_session_get_image(session_, &out.pixels.data()->x);
  if (rc != VPT_OK) fail(denoised ? "vpt_session_get_denoised" : "vpt_session_get_image");
  return out;
}
pathtrace_state render_session::state() {
  auto st   = pathtrace_state{};
  st.width  = width(), st.height = height();
  auto n    = (size_t)st.width * st.height;
  st.image.resize(n), st.hits.resize(n), st.rngs.resize(n);
  if (vpt_session_get_state(session_, &st.image.data()->x, st.hits.data(), (uint64_t*)st.rngs.data(), &st.samples) != VPT_OK) fail("vpt_session_get_state");
  return st;
}

}  // namespace vpt
