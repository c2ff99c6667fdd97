// vpt_denoise.cpp — denoise_render on the CPU: the rule of include/vpt.h (vpt_denoise_params) restated in plain C++, the
// statement the HIP kernels of csrc/vpt_denoise.hip are held to bit for bit (-ffp-contract=off, float32 throughout, the sums
// in tap order); the same through the GPU (vpt_denoise); and pathtrace_guides, the two renders that guide the filter.
#include <cmath>

#include "vpt_host.h"

namespace vpt {

namespace {
float lum(const vec4f& c) { return ((c.x + c.y) + c.z) / 3.0f; }
float d2(const vec4f& a, const vec4f& b) {
  auto x = a.x - b.x, y = a.y - b.y, z = a.z - b.z, w = a.w - b.w;
  return ((x * x + y * y) + z * z) + w * w;
}
float max0(float a) { return a > 0.0f ? a : 0.0f; }
const float kernel_h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};

// box3(f): mean of f over the 3x3 taps of each pixel that fall inside the image
template <typename F>
float box3(int width, int height, int px, int py, F&& f) {
  auto sum = 0.0f, count = 0.0f;
  for (auto dy = -1; dy <= 1; dy++) {
    for (auto dx = -1; dx <= 1; dx++) {
      auto qx = px + dx, qy = py + dy;
      if (qx < 0 || qx >= width || qy < 0 || qy >= height) continue;
      sum = sum + f((size_t)qy * width + qx), count = count + 1.0f;
    }
  }
  return sum / count;
}

void check_inputs(const color_image& render, const color_image& albedo, const color_image& normal, const vector<float>& variance,
    const denoise_params& params) {
  if (render.width < 1 || render.height < 1 || render.pixels.size() != (size_t)render.width * render.height)
    throw std::invalid_argument{"render is empty"};
  for (auto guide : {&albedo, &normal})
    if (!guide->pixels.empty() && (guide->width != render.width || guide->height != render.height || guide->pixels.size() != render.pixels.size()))
      throw std::invalid_argument{"image should have the same size"};
  if (!variance.empty() && variance.size() != render.pixels.size()) throw std::invalid_argument{"variance should have the same size"};
  if (params.iterations < 1 || params.iterations > 8) throw std::invalid_argument{"iterations outside 1..8"};
  for (auto sigma : {params.sigma_luminance, params.sigma_normal, params.sigma_albedo})
    if (!std::isfinite(sigma) || !(sigma > 0)) throw std::invalid_argument{"sigma must be finite and > 0"};
}
}  // namespace

void denoise_render(color_image& denoised, const color_image& render, const color_image& albedo, const color_image& normal,
    const vector<float>& variance, const denoise_params& params) {
  check_inputs(render, albedo, normal, variance, params);
  auto width = render.width, height = render.height;
  auto n     = render.pixels.size();
  auto has_n = !normal.pixels.empty(), has_a = !albedo.pixels.empty();
  auto c = render.pixels, c_next = vector<vec4f>(n);
  auto v = variance, v_next = vector<float>(n);
  if (v.empty()) {   // the spatial seed
    v.resize(n);
    for (auto py = 0; py < height; py++) {
      for (auto px = 0; px < width; px++) {
        auto m  = box3(width, height, px, py, [&](size_t q) { return lum(c[q]); });
        auto m2 = box3(width, height, px, py, [&](size_t q) { return lum(c[q]) * lum(c[q]); });
        v[(size_t)py * width + px] = max0(m2 - m * m);
      }
    }
  }
  auto rn = 1.0f / (params.sigma_normal * params.sigma_normal), ra = 1.0f / (params.sigma_albedo * params.sigma_albedo);
  for (auto k = 0; k < params.iterations; k++) {
    auto s = 1 << k;
    for (auto py = 0; py < height; py++) {
      for (auto px = 0; px < width; px++) {
        auto p   = (size_t)py * width + px;
        auto lp  = lum(c[p]);
        auto r   = 1.0f / (params.sigma_luminance * std::sqrt(v[p]) + 1e-4f);
        auto W = 0.0f, V = 0.0f, Cx = 0.0f, Cy = 0.0f, Cz = 0.0f;
        for (auto dy = -2; dy <= 2; dy++) {
          for (auto dx = -2; dx <= 2; dx++) {
            auto qx = px + s * dx, qy = py + s * dy;
            if (qx < 0 || qx >= width || qy < 0 || qy >= height) continue;
            auto q = (size_t)qy * width + qx;
            auto x = std::fabs(lp - lum(c[q])) * r;
            if (has_n) x = x + d2(normal.pixels[p], normal.pixels[q]) * rn;
            if (has_a) x = x + d2(albedo.pixels[p], albedo.pixels[q]) * ra;
            auto u = max0(1.0f - x / 4.0f);
            auto w = (kernel_h[dy + 2] * kernel_h[dx + 2]) * ((u * u) * (u * u));
            W = W + w;
            Cx = Cx + w * c[q].x, Cy = Cy + w * c[q].y, Cz = Cz + w * c[q].z;
            V = V + (w * w) * v[q];
          }
        }
        c_next[p] = {Cx / W, Cy / W, Cz / W, c[p].w};
        v_next[p] = V / (W * W);
      }
    }
    c.swap(c_next), v.swap(v_next);
  }
  denoised.width = width, denoised.height = height, denoised.linear = render.linear;
  denoised.pixels = std::move(c);
}

void denoise_render_device(color_image& denoised, const color_image& render, const color_image& albedo, const color_image& normal,
    const vector<float>& variance, const denoise_params& params, int device) {
  check_inputs(render, albedo, normal, variance, params);
  auto abi = vpt_denoise_params{params.iterations, params.sigma_luminance, params.sigma_normal, params.sigma_albedo};
  auto out = vector<vec4f>(render.pixels.size());
  if (vpt_denoise(&abi, device, render.width, render.height, &render.pixels.data()->x, normal.pixels.empty() ? nullptr : &normal.pixels.data()->x,
          albedo.pixels.empty() ? nullptr : &albedo.pixels.data()->x, variance.empty() ? nullptr : variance.data(), &out.data()->x) != VPT_OK)
    throw std::runtime_error{string{"vpt_denoise: "} + vpt_last_error()};
  denoised.width = render.width, denoised.height = render.height, denoised.linear = render.linear;
  denoised.pixels = std::move(out);
}

vector<float> half_variance(int width, int height, const vector<vec4f>& sum_a, int a, const vector<vec4f>& sum_n, int n, int device) {
  if (width < 1 || height < 1 || sum_a.size() != (size_t)width * height || sum_n.size() != sum_a.size())
    throw std::invalid_argument{"image should have the same size"};
  if (a <= 0 || a >= n) throw std::invalid_argument{"sample counts must satisfy 0 < a < n"};
  auto variance = vector<float>(sum_a.size());
  if (device >= 0) {
    if (vpt_half_variance(device, width, height, &sum_a.data()->x, a, &sum_n.data()->x, n, variance.data()) != VPT_OK)
      throw std::runtime_error{string{"vpt_half_variance: "} + vpt_last_error()};
    return variance;
  }
  auto fa = (float)a, fb = (float)(n - a);
  auto g2 = [&](size_t q) {
    auto &sa = sum_a[q], &sn = sum_n[q];
    auto A = vec4f{sa.x / fa, sa.y / fa, sa.z / fa, 0};
    auto B = vec4f{(sn.x - sa.x) / fb, (sn.y - sa.y) / fb, (sn.z - sa.z) / fb, 0};
    auto g = (lum(A) - lum(B)) / 2.0f;
    return g * g;
  };
  for (auto py = 0; py < height; py++)
    for (auto px = 0; px < width; px++) variance[(size_t)py * width + px] = box3(width, height, px, py, g2);
  return variance;
}

denoise_guides pathtrace_guides(const scene_data& scene, const bvh_scene& bvh, const pathtrace_lights& lights, const pathtrace_params& params,
    int samples) {
  if (samples < 1) throw std::invalid_argument{"guide samples must be >= 1"};
  if ((int)params.shader == 16) throw std::invalid_argument{"the volgrid shader has no guides: a medium has no surface normal and no albedo"};
  auto implicit = params.shader == pathtrace_shader_type::implicit || params.shader == pathtrace_shader_type::implicit_normal;
  auto render   = [&](pathtrace_shader_type shader) {
    auto p    = params;
    p.shader  = shader;
    p.samples = samples;
    auto state = make_state(scene, p);
    pathtrace_samples(state, scene, bvh, lights, p, samples);
    return get_render(state);
  };
  auto guides = denoise_guides{};
  if (implicit) {
    guides.normal = render(pathtrace_shader_type::implicit_normal);
  } else {   // both guides trace the same rays: one first-hit pass
    auto aovs     = pathtrace_aovs(scene, bvh, lights, params, samples, aov_normal | aov_albedo);
    guides.normal = std::move(aovs.normal), guides.albedo = std::move(aovs.albedo);
  }
  return guides;
}

}  // namespace vpt
