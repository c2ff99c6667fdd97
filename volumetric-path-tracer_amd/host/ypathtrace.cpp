// ypathtrace — offline renderer CLI with the reference's command line (apps/ypathtrace/ypathtrace.cpp:307-337 over
// libs/yocto/yocto_cli.cpp): --scene --output --shader --samples --resolution --bounces --noparallel --noimplicitmis
// --stmaxiter, each with the reference's default and range, --config <file.json> (yocto_cli.cpp:912-945: a JSON object of
// option values, the command line wins), --help; errors are reported as the reference's parser words them ("unknown
// option X", "missing value for X", "bad value for X") and end the program with status 1.  --interactive is out of scope.
// The run itself is the reference's run_offline sequence (:41-87): load, tesselate, bvh, lights, state, N x
// pathtrace_samples, save.  Rendering happens on the GPU through include/vpt.h; two extensions: --gpus N (tiles dealt
// round-robin over N GPUs, same image), --batch n (samples per kernel launch; default: all in one, same image) and --gpubvh
// (the BVHs built on the GPU by vpt_build_bvh: the same trees), --highqualitybvh (the reference's SAH build, make_bvh(scene, true), on the
// host or with --gpubvh on the GPU: include/vpt.h, vpt_build_bvh_quality), --gputess (the float32 half of tesselate_surfaces on the GPU by
// vpt_subdivide_vertices: the same meshes), --adaptive t (adaptive sampling, vpt_render_adaptive: every pixel renders in rounds of
// --adaptivestep samples until the relative standard error of its mean is within t, never below --adaptivemin samples, at most --samples;
// the image is written from each pixel's own sample count), --denoise (denoise_render: the guided à-trous filter of include/vpt.h over
// the finished render, on GPU 0; its guides are --denoiseguides samples of the `normal` and `color` shaders, its variance comes from the two
// halves of the sample chain, or from the image itself after --adaptive; --denoiseiters and --denoisesigma* set its parameters),
// --cameras FILE (a JSON array of camera objects with the keys of a scene file's "cameras" entries: the scene is loaded and sent to
// the GPUs once; for entry k the camera --camera selects is replaced in the resident scene through vpt_scene_update, a fresh state is
// rendered and saved as <stem>.<k, four digits><extension> of --output), --progressive N (the headless body of the reference's
// run_interactive, through a vpt_session on GPU 0: the preview of --pratio is written as <stem>.000000<extension>, the device's display after
// every N samples as <stem>.<samples, six digits><extension>, the finished image as --output; --exposure and --filmic are the display's
// tone-mapping parameters; with --denoise the display shows the filtered image.  With --exposure 0 and without --filmic, --output holds
// the bytes of the offline run with the same arguments: the same state, the same host 8-bit stage), --bake-sdf FILE (no scene is
// rendered: the shape file is loaded through the host loader, baked by vpt_bake_sdf on GPU 0 - or by the host mirror with --bake-host,
// same bytes - into a grid of --bake-res voxels per axis fitted around it with --bake-padding voxels to spare, and written to --output
// as the binary .sdf the scene loader reads; `res` and a vol_instances entry that puts the grid where the shape was go to stdout),
// --mesh-sdf FILE (no scene is rendered: the binary .sdf is meshed at --mesh-iso by vpt_mesh_sdf on GPU 0 - or by the host mirror with
// --mesh-host, same bytes - in the grid's own space, origin 0 and step = res * W / (W - 1), and written to --output as a binary PLY of
// positions, normals and quads; the counts go to stdout).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "vpt_host.h"

using namespace vpt;

namespace {

struct option {
  enum kind_t { string_k, int_k, bool_k, shader_k, float_k, posfloat_k, anyfloat_k } kind;   // float_k: finite and >= 0; posfloat_k: finite and > 0; anyfloat_k: finite
  int         lo, hi;   // int_k: inclusive range (lo > hi: unbounded)
  const char* usage;
};
const std::vector<std::pair<string, option>> options = {
    {"scene", {option::string_k, 1, 0, "Scene filename."}},
    {"output", {option::string_k, 1, 0, "Output filename."}},
    {"interactive", {option::bool_k, 1, 0, "Run interactively."}},
    {"resolution", {option::int_k, 1, 4096, "Image resolution."}},
    {"shader", {option::shader_k, 1, 0, "Shader type."}},
    {"samples", {option::int_k, 1, 4096, "Number of samples."}},
    {"bounces", {option::int_k, 1, 128, "Number of bounces."}},
    {"noparallel", {option::bool_k, 1, 0, "Disable threading."}},
    {"noimplicitmis", {option::bool_k, 1, 0, "Disable MIS on implicit shader"}},
    {"stmaxiter", {option::int_k, 1, 512, "Number of maximum iteration while spheretracing"}},
    {"camera", {option::int_k, 0, 1 << 20, "Camera index. (extension)"}},
    {"gpus", {option::int_k, 1, 64, "GPUs to spread the frame's tiles over. (extension)"}},
    {"batch", {option::int_k, 0, 4096, "Samples per kernel launch, 0 = all. (extension)"}},
    {"gpubvh", {option::bool_k, 1, 0, "Build the BVHs on the GPU: same trees. (extension)"}},
    {"highqualitybvh", {option::bool_k, 1, 0, "Use high quality BVH: the reference's SAH build. (extension)"}},
    {"gputess", {option::bool_k, 1, 0, "Subdivision vertex arithmetic on the GPU: same meshes. (extension)"}},
    {"adaptive", {option::float_k, 1, 0, "Adaptive sampling: relative noise at which a pixel stops, 0 = off. (extension)"}},
    {"adaptivemin", {option::int_k, 1, 4096, "Adaptive sampling: fewest samples before a pixel stops. (extension)"}},
    {"adaptivestep", {option::int_k, 1, 4096, "Adaptive sampling: samples per round. (extension)"}},
    {"cameras", {option::string_k, 1, 0, "Render one frame per camera of this JSON array, the scene staying on the GPU. (extension)"}},
    {"denoise", {option::bool_k, 1, 0, "Denoise the render with the guided a-trous filter. (extension)"}},
    {"denoiseiters", {option::int_k, 1, 8, "Denoising: filter passes, pass k has stride 2^k. (extension)"}},
    {"denoiseguides", {option::int_k, 1, 4096, "Denoising: samples of the normal and albedo guides. (extension)"}},
    {"denoisesigmalum", {option::posfloat_k, 1, 0, "Denoising: luminance tolerance in standard deviations. (extension)"}},
    {"denoisesigmanormal", {option::posfloat_k, 1, 0, "Denoising: tolerance of the normal guide. (extension)"}},
    {"denoisesigmaalbedo", {option::posfloat_k, 1, 0, "Denoising: tolerance of the albedo guide. (extension)"}},
    {"progressive", {option::int_k, 1, 4096, "Render progressively on the GPU, a display frame every N samples. (extension)"}},
    {"converge", {option::float_k, 1, 0, "Progressive: stop a pixel at this relative noise and the render when all have stopped; a round per display frame. (extension)"}},
    {"pratio", {option::int_k, 1, 64, "Progressive: preview ratio."}},
    {"exposure", {option::anyfloat_k, 1, 0, "Progressive: display exposure."}},
    {"filmic", {option::bool_k, 1, 0, "Progressive: filmic tone mapping."}},
    {"bake-sdf", {option::string_k, 1, 0, "Bake this shape file (PLY, OBJ) into a signed-distance grid written to --output; renders nothing. (extension)"}},
    {"bake-res", {option::int_k, 1, 1024, "Baking: voxels per axis."}},
    {"bake-padding", {option::int_k, 0, 64, "Baking: voxels to spare around the shape on each side."}},
    {"bake-host", {option::bool_k, 1, 0, "Baking: run the host mirror instead of the GPU: same file."}},
    {"mesh-sdf", {option::string_k, 1, 0, "Mesh this binary .sdf grid into quads written to --output (PLY); renders nothing. (extension)"}},
    {"mesh-iso", {option::anyfloat_k, 1, 0, "Meshing: the iso value, inside is below it."}},
    {"mesh-host", {option::bool_k, 1, 0, "Meshing: run the host mirror instead of the GPU: same file."}},
};
const option* find_option(const string& name) {
  for (auto& [n, o] : options)
    if (n == name) return &o;
  return nullptr;
}

string usage() {
  auto text = string{"usage: ypathtrace [options]\nRaytrace scenes.\n\noptions:\n"};
  for (auto& [name, o] : options) {
    auto line = "  --" + name + (o.kind == option::bool_k  ? "/--no-" + name
                                 : o.kind == option::int_k ? " <integer>"
                                 : o.kind == option::float_k || o.kind == option::posfloat_k || o.kind == option::anyfloat_k ? " <float>"
                                                             : " <string>");
    line.resize(line.size() < 32 ? 32 : line.size() + 1, ' ');
    text += line + o.usage + "\n";
    if (o.kind == option::shader_k) {
      text += "    with choices: ";
      for (auto& s : pathtrace_shader_names) text += s + ", ";
      for (auto& s : pathtrace_extension_shaders) text += s.first + (&s == &pathtrace_extension_shaders.back() ? "\n" : ", ");   // after the reference's names
    }
  }
  text += "  --help                        Prints help. (false)\n  --config <string>             Load configuration. (\"\")\n";
  return text;
}

[[noreturn]] void cli_error(const string& message) {   // handle_errors / print_fatal of the reference: message, usage, status 1
  fprintf(stderr, "error: %s\n%s", message.c_str(), usage().c_str());
  exit(1);
}
[[noreturn]] void print_fatal(const string& message) {
  fprintf(stderr, "error: %s\n", message.c_str());
  exit(1);
}

// the text of one option value, validated against the option's type and range
void check_value(const string& name, const option& o, const string& text) {
  if (o.kind == option::int_k) {
    auto end = (char*)nullptr;
    auto v   = strtol(text.c_str(), &end, 10);
    if (end == text.c_str() || *end != 0) cli_error("bad value for " + name);
    if (o.lo <= o.hi && (v < o.lo || v > o.hi)) cli_error("bad value for " + name);
  } else if (o.kind == option::float_k) {
    auto end = (char*)nullptr;
    auto v   = strtof(text.c_str(), &end);
    if (end == text.c_str() || *end != 0 || !std::isfinite(v) || v < 0) cli_error("bad value for " + name);
  } else if (o.kind == option::posfloat_k) {
    auto end = (char*)nullptr;
    auto v   = strtof(text.c_str(), &end);
    if (end == text.c_str() || *end != 0 || !std::isfinite(v) || !(v > 0)) cli_error("bad value for " + name);
  } else if (o.kind == option::anyfloat_k) {
    auto end = (char*)nullptr;
    auto v   = strtof(text.c_str(), &end);
    if (end == text.c_str() || *end != 0 || !std::isfinite(v)) cli_error("bad value for " + name);
  } else if (o.kind == option::bool_k) {
    if (text != "true" && text != "false") cli_error("bad value for " + name);
  } else if (o.kind == option::shader_k) {
    auto found = false;
    for (auto& s : pathtrace_shader_names) found = found || s == text;
    for (auto& s : pathtrace_extension_shaders) found = found || s.first == text;
    if (!found) cli_error("bad value for " + name);
  }
}

}  // namespace

int main(int argc, const char** argv) {
  auto values = std::map<string, string>{};   // option name -> value text, command line first
  auto config = string{};
  for (auto i = 1; i < argc; i++) {
    auto arg = string{argv[i]};
    if (arg == "--help" || arg == "-h") {
      printf("%s", usage().c_str());
      return 0;
    }
    if (arg == "--config") {
      if (i + 1 >= argc) cli_error("missing value for config");
      config = argv[++i];
      continue;
    }
    if (arg.rfind("--", 0) != 0) cli_error("unknown option " + arg);
    auto name = arg.substr(2);
    auto o    = find_option(name);
    if (!o && name.rfind("no-", 0) == 0 && find_option(name.substr(3)) && find_option(name.substr(3))->kind == option::bool_k) {
      values[name.substr(3)] = "false";
      continue;
    }
    if (!o) cli_error("unknown option " + arg);
    if (o->kind == option::bool_k) {
      values[name] = "true";
      continue;
    }
    if (i + 1 >= argc) cli_error("missing value for " + name);
    values[name] = argv[++i];
  }
  if (!config.empty()) {   // the file's values fill in what the command line left open
    auto members = vector<std::pair<string, string>>{};
    auto error   = string{};
    if (!load_cli_config(config, members, error)) print_fatal(error);
    for (auto& [key, text] : members) {
      if (!find_option(key)) cli_error("unknown option " + key);
      if (!values.count(key)) values[key] = text;
    }
  }
  for (auto& [name, text] : values) check_value(name, *find_option(name), text);

  auto params   = pathtrace_params{};
  auto filename = string{"scene.json"}, output = string{"image.png"};
  auto batch = 0, gpus = 1;
  auto get_int = [&](const char* name, int& v) {
    if (values.count(name)) v = atoi(values[name].c_str());
  };
  auto get_bool = [&](const char* name, bool& v) {
    if (values.count(name)) v = values[name] == "true";
  };
  if (values.count("scene")) filename = values["scene"];
  if (values.count("output")) output = values["output"];
  get_int("resolution", params.resolution), get_int("samples", params.samples), get_int("bounces", params.bounces);
  get_int("stmaxiter", params.spheretrace_maxiter), get_int("camera", params.camera), get_int("batch", batch), get_int("gpus", gpus);
  get_bool("noparallel", params.noparallel), get_bool("noimplicitmis", params.noimplicit_mis);
  auto adaptive = pathtrace_adaptive_params{};
  if (values.count("adaptive")) adaptive.threshold = strtof(values["adaptive"].c_str(), nullptr);
  adaptive.min_samples = std::min(adaptive.min_samples, params.samples);   // the default never exceeds the cap; an explicit value must not
  get_int("adaptivemin", adaptive.min_samples), get_int("adaptivestep", adaptive.step);
  if (adaptive.min_samples > params.samples) cli_error("bad value for adaptivemin");
  if (adaptive.threshold > 0 && gpus > 1) print_fatal("--adaptive renders on one GPU: it cannot be combined with --gpus " + std::to_string(gpus));
  auto interactive = false, gpubvh = false, gputess = false, denoise = false, highqualitybvh = false;
  get_bool("interactive", interactive), get_bool("gpubvh", gpubvh), get_bool("gputess", gputess), get_bool("denoise", denoise);
  get_bool("highqualitybvh", highqualitybvh);
  auto filter = denoise_params{};
  auto guide_samples = 16;
  get_int("denoiseiters", filter.iterations), get_int("denoiseguides", guide_samples);
  auto get_float = [&](const char* name, float& v) {
    if (values.count(name)) v = strtof(values[name].c_str(), nullptr);
  };
  get_float("denoisesigmalum", filter.sigma_luminance), get_float("denoisesigmanormal", filter.sigma_normal);
  get_float("denoisesigmaalbedo", filter.sigma_albedo);
  if (interactive) print_fatal("--interactive is not supported by the GPU build");
  auto progressive = 0;
  get_int("progressive", progressive), get_int("pratio", params.pratio), get_float("exposure", params.exposure), get_bool("filmic", params.filmic);
  if (!progressive)
    for (auto name : {"exposure", "filmic", "pratio", "converge"})
      if (values.count(name)) cli_error(string{"option "} + name + " needs --progressive");
  if (progressive && gpus > 1) cli_error("option progressive renders on one GPU: it cannot be combined with gpus " + std::to_string(gpus));
  if (progressive && adaptive.threshold > 0) cli_error("option progressive cannot be combined with adaptive");
  if (progressive && values.count("cameras")) cli_error("option progressive cannot be combined with cameras");
  if (progressive && params.resolution / params.pratio < 1) cli_error("bad value for pratio");
  if (values.count("shader"))
    for (size_t k = 0; k < pathtrace_shader_names.size(); k++)
      if (pathtrace_shader_names[k] == values["shader"]) params.shader = (pathtrace_shader_type)k;
  if (values.count("shader"))
    for (auto& s : pathtrace_extension_shaders)
      if (s.first == values["shader"]) params.shader = (pathtrace_shader_type)s.second;

  for (auto name : {"bake-res", "bake-padding", "bake-host"})
    if (values.count(name) && !values.count("bake-sdf")) cli_error(string{"option "} + name + " needs --bake-sdf");
  if (values.count("bake-sdf")) {
    auto res = 0, padding = 2;
    auto on_host = false;
    get_int("bake-res", res), get_int("bake-padding", padding), get_bool("bake-host", on_host);
    if (!values.count("bake-res")) cli_error("missing value for bake-res");
    if (res < 2 * padding + 3) cli_error("bad value for bake-res");
    if (!values.count("output")) cli_error("missing value for output");
    try {
      auto error = string{};
      auto shape = shape_data{};
      if (!load_shape(values["bake-sdf"], shape, error, true)) print_fatal(error);
      auto triangles = bake_triangles(shape);
      if (triangles.empty()) print_fatal(values["bake-sdf"] + ": the shape has no triangles or quads");
      auto t0    = std::chrono::steady_clock::now();
      auto baked = bake_volume(shape.positions, triangles, {res, res, res}, padding, on_host ? -1 : 0);
      auto secs  = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (!save_volume(output, baked.volume, error)) print_fatal(error);
      auto& f = baked.instance.frame;
      printf("baked: %zu triangles (%d dropped) into %d x %d x %d voxels in %.3f s (%s)\n", triangles.size(), baked.stats.dropped_triangles, res, res,
          res, secs, on_host ? "host mirror" : "GPU 0");
      printf("res: %.9g\n", baked.volume.res);
      printf("{\"name\": \"baked\", \"volume\": 0, \"material\": 0, \"scale\": %.9g, \"frame\": [%.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g, %.9g]}\n",
          baked.instance.scalef, f.x.x, f.x.y, f.x.z, f.y.x, f.y.y, f.y.z, f.z.x, f.z.y, f.z.z, f.o.x, f.o.y, f.o.z);
      return 0;
    } catch (const std::exception& e) {
      print_fatal(e.what());
    }
  }

  for (auto name : {"mesh-iso", "mesh-host"})
    if (values.count(name) && !values.count("mesh-sdf")) cli_error(string{"option "} + name + " needs --mesh-sdf");
  if (values.count("mesh-sdf")) {
    auto iso     = 0.0f;
    auto on_host = false;
    get_float("mesh-iso", iso), get_bool("mesh-host", on_host);
    if (!values.count("output")) cli_error("missing value for output");
    try {
      auto error  = string{};
      auto volume = volume_data{};
      if (!load_volume(values["mesh-sdf"], volume, true, error)) print_fatal(error);
      // the space the renderer's lookup reads the grid in before scalef: origin 0, step = res * W / (W - 1) per axis
      auto desc = vpt_sdf_mesh_desc{{volume.whd.x, volume.whd.y, volume.whd.z}, {0, 0, 0}, {0, 0, 0}, iso};
      for (auto k = 0; k < 3; k++) desc.step[k] = volume.res * (float)desc.whd[k] / (float)std::max(1, desc.whd[k] - 1);
      auto t0   = std::chrono::steady_clock::now();
      auto mesh = on_host ? mesh_sdf(volume.vol.data(), desc) : mesh_sdf_device(volume.vol.data(), desc, 0);
      auto secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (!save_mesh_ply(output, mesh, error)) print_fatal(error);
      printf("meshed: %d x %d x %d voxels at iso %.9g into %zu vertices and %zu quads in %.3f s (%s)\n", desc.whd[0], desc.whd[1], desc.whd[2], iso,
          mesh.positions.size(), mesh.quads.size(), secs, on_host ? "host mirror" : "GPU 0");
      return 0;
    } catch (const std::exception& e) {
      print_fatal(e.what());
    }
  }

  try {
    auto error = string{};
    auto scene = scene_data{};
    if (!load_scene(filename, scene, error)) print_fatal(error);
    if (params.camera >= (int)scene.cameras.size()) cli_error("bad value for camera");
    if (gputess) tesselate_surfaces_device(scene, 0);
    else tesselate_surfaces(scene);
    auto quality = highqualitybvh ? VPT_BVH_SAH : VPT_BVH_MIDDLE;
    auto bvh     = gpubvh ? make_bvh_device(scene, params, 0, quality) : make_bvh(scene, params, quality);
    auto lights = make_lights(scene, params);
    auto frames = vector<camera_data>{};   // --cameras: one frame each; else the scene's own camera, once
    if (values.count("cameras") && !load_cameras(values["cameras"], frames, error)) print_fatal(error);
    auto base_output = output;
    if (gpus > 1) {
      auto devices = vector<int>{};
      for (auto d = 0; d < gpus; d++) devices.push_back(d);
      pathtrace_set_devices(devices);
    }
    // --denoise: guides, filter on GPU 0, save; the line it prints follows the render's own
    auto denoise_and_save = [&](const color_image& render, const vector<float>& variance) {
      auto t1     = std::chrono::steady_clock::now();
      auto guides = pathtrace_guides(scene, bvh, lights, params, guide_samples);
      auto t2     = std::chrono::steady_clock::now();
      auto clean  = color_image{};
      denoise_render_device(clean, render, guides.albedo, guides.normal, variance, filter, 0);
      auto t3 = std::chrono::steady_clock::now();
      printf("denoised: guides %d spp in %.3f s, filter %d passes (%s variance) in %.3f s\n", guide_samples,
          std::chrono::duration<double>(t2 - t1).count(), filter.iterations, variance.empty() ? "spatial" : "half", std::chrono::duration<double>(t3 - t2).count());
      if (!save_image(output, clean, error)) print_fatal(error);
    };
    // one frame: a fresh state of the selected camera rendered as the options say and saved to `output`
    auto render_frame = [&]() {
      auto state = make_state(scene, params);
      auto t0 = std::chrono::steady_clock::now();
      if (adaptive.threshold > 0) {   // rounds of --adaptivestep samples until every pixel is clean enough or at --samples
        auto stats = pathtrace_adaptive(state, scene, bvh, lights, params, adaptive);
        auto secs  = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        auto full  = (double)state.width * state.height * params.samples;
        printf("adaptive: %d rounds, %lld samples taken of %.0f (%.1f %%) in %.3f s (%.2f Msamples/s)\n", stats.rounds, (long long)stats.samples,
            full, 100.0 * (double)stats.samples / full, secs, (double)stats.samples / secs * 1e-6);
        if (denoise) denoise_and_save(get_render_hits(state), {});   // pixels hold their own sample counts: the spatial seed
        else if (!save_image(output, get_render_hits(state), error)) print_fatal(error);
        return;
      }
      // one launch per `batch` samples (default: all); identical to that many single calls
      if (batch <= 0) batch = params.samples;
      // --denoise stops once at half the samples to keep the radiance sums for the half variance (same final state: batching is exact)
      auto half = denoise ? params.samples / 2 : 0;
      auto sum_half = vector<vec4f>{};
      while (state.samples < half) pathtrace_samples(state, scene, bvh, lights, params, std::min(batch, half - state.samples));
      if (half > 0) sum_half = state.image;
      while (state.samples < params.samples) pathtrace_samples(state, scene, bvh, lights, params, batch);
      auto secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      printf("rendered %dx%d x %d spp in %.3f s (%.2f Msamples/s)\n", state.width, state.height, state.samples, secs,
          (double)state.width * state.height * state.samples / secs * 1e-6);
      if (denoise) {
        auto variance = half > 0 ? half_variance(state.width, state.height, sum_half, half, state.image, state.samples, 0) : vector<float>{};
        denoise_and_save(get_render(state), variance);
      } else if (!save_image(output, get_render(state), error)) print_fatal(error);
    };
    // --progressive: reset_display and the worker's loop of run_interactive on a session; the displays are the device's
    auto numbered = [&](int number) {
      char text[16];
      snprintf(text, sizeof(text), ".%06d", number);
      auto dot = base_output.find_last_of("./\\");
      auto ext = dot != string::npos && base_output[dot] == '.' ? dot : base_output.size();
      return base_output.substr(0, ext) + text + base_output.substr(ext);
    };
    auto save_display = [&](render_session& session, const string& name) {
      auto bytes = session.display();
      auto ldr   = color_image{session.width(), session.height(), false, {}};
      ldr.pixels.resize(bytes.size());
      auto unit = [](uint8_t b) { return ((float)b + 0.5f) / 256; };   // save_image quantises it back to b
      for (size_t i = 0; i < bytes.size(); i++) ldr.pixels[i] = {unit(bytes[i].x), unit(bytes[i].y), unit(bytes[i].z), unit(bytes[i].w)};
      if (!save_image(name, ldr, error)) print_fatal(error);
    };
    if (progressive) {
      auto sp = render_session_params{params, denoise, filter, guide_samples};
      auto t0 = std::chrono::steady_clock::now();
      auto session = render_session{scene, bvh, lights, sp, 0};
      save_display(session, numbered(0));
      auto shown = 0;
      if (values.count("converge")) {   // adaptive rounds of N samples, one per display frame, until every pixel has stopped
        auto converge = pathtrace_adaptive_params{strtof(values["converge"].c_str(), nullptr), adaptive.min_samples, progressive};
        session.set_adaptive(converge);
        while (!session.converged() && session.samples() < params.samples) {
          session.advance(progressive);
          save_display(session, numbered(session.samples())), shown++;
        }
        auto stats = session.progress();
        auto full  = (double)session.width() * session.height() * params.samples;
        printf("converge: %d rounds, %lld samples taken of %.0f (%.1f %%), %d pixels still rendering\n", stats.rounds, (long long)stats.samples,
            full, 100.0 * (double)stats.samples / full, stats.active);
      }
      while (!values.count("converge") && session.samples() < params.samples) {
        session.advance(progressive);
        save_display(session, numbered(session.samples())), shown++;
      }
      auto secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      printf("rendered %dx%d x %d spp progressively in %.3f s (preview 1/%d, %d display frames)\n", session.width(), session.height(),
          session.samples(), secs, params.pratio, shown);
      auto image = session.image(denoise);
      if (params.exposure != 0 || params.filmic) {   // the host tone map; else the offline path's own 8-bit stage
        auto mapped = color_image{image.width, image.height, false, {}};
        tonemap_image(mapped.pixels, image.pixels, params.exposure, params.filmic, true);
        image = mapped;
      }
      if (!save_image(output, image, error)) print_fatal(error);
      return 0;
    }
    if (frames.empty()) render_frame();
    for (size_t frame = 0; frame < frames.size(); frame++) {
      // --cameras: the camera edited in place - pathtrace_samples sends it to the resident scene (vpt_scene_update)
      scene.cameras[params.camera] = frames[frame];
      char number[16];
      snprintf(number, sizeof(number), ".%04d", (int)frame);
      auto dot = base_output.find_last_of("./\\");
      auto ext = dot != string::npos && base_output[dot] == '.' ? dot : base_output.size();
      output   = base_output.substr(0, ext) + number + base_output.substr(ext);
      render_frame();
    }
  } catch (const std::exception& e) {
    print_fatal(e.what());
  }
  return 0;
}
