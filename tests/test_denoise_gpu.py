"""The denoising filter on the MI355X (vpt_denoise, vpt_denoise_device, vpt_half_variance_device; include/vpt.h).  The kernels are
held to the host C++ mirror bit for bit, every pixel: the rule has no libm call, so there is no tolerance to grant.  Then: the plain and
the tiled form of a pass give the same bits, the call leaves its inputs alone and repeats itself, and the filter pays on real renders
measured against a 2048-spp render of the same shader; and ypathtrace --denoise writes what the same steps give through Python.

Quality ratios measured on the MI355X (denoised RMS over the RMS it has to beat; each must be < 1; the CPU oracle's worst was 0.76):
  03_volume, volpathtrace b64:      8 spp denoised / 8 spp 0.484,  8 spp denoised / 16 spp 0.612,  32 spp denoised / 32 spp 0.500
  07_sdfunction_synth, implicit b6: 8 spp denoised / 8 spp 0.479,  8 spp denoised / 16 spp 0.663,  32 spp denoised / 32 spp 0.737,
                                    64 spp: half variance / spatial seed 0.768 (0.0258 / 0.0336; undenoised 0.0353)"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, SCENE_03

pytestmark = pytest.mark.gpu

F = np.float32
SDFN = os.path.join(GOLDEN, "scenes", "07_sdfunction_synth", "sdfunction_synth.json")
CURVES = os.path.join(GOLDEN, "scenes", "09_curves_synth", "curves.json")

# name -> (scene, shader, bounces, resolution, samples)
CASES = {
    "volume_96": (SCENE_03, "volpathtrace", 64, 96, 16),
    "volume_1280": (SCENE_03, "volpathtrace", 64, 1280, 8),
    "sdfunction_implicit": (SDFN, "implicit", 6, 96, 16),
    "curves": (CURVES, "volpathtrace", 8, 96, 16),
}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def differing(a, b):
    return f"{int(np.sum(np.any(a.view(np.uint32) != b.view(np.uint32), axis=-1)))} of {a.shape[0] * a.shape[1]} pixels differ"


def srgb(x):
    x = np.clip(x, 0, 1).astype(np.float64)
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1 / 2.4) - 0.055)


def rms(a, b):
    return float(np.sqrt(np.mean((srgb(a[..., :3]) - srgb(b[..., :3])) ** 2)))


def render_with_half(vpt, scene, dev, params, n):
    """(resolved n-spp render, half variance from its sample chain split at n // 2)"""
    st = scene.make_state(params)
    dev.pathtrace_samples(st, params, n // 2)
    sum_a = st.image.copy()
    dev.pathtrace_samples(st, params, n - n // 2)
    assert st.samples == n
    return vpt.get_render(st), vpt.half_variance(sum_a, n // 2, st.image, n), (sum_a, st.image.copy())


_inputs = {}


def inputs(vpt, case):
    """(color, albedo, normal, variance, (sum_a, sum_n, a, n)) of a case, rendered once per session"""
    if case not in _inputs:
        path, shader, bounces, res, n = CASES[case]
        scene = vpt.HostScene(path)
        dev = vpt.DeviceScene(scene, 0)
        params = vpt.PathtraceParams(resolution=res, samples=n, shader=shader, bounces=bounces)
        color, variance, (sum_a, sum_n) = render_with_half(vpt, scene, dev, params, n)
        normal, albedo = vpt.pathtrace_guides(scene, dev, params, 4)
        dev.close()
        _inputs[case] = (color, albedo, normal, variance, (sum_a, sum_n, n // 2, n))
    return _inputs[case]


def device_call(vpt, color, albedo, normal, variance, **kw):
    """vpt_denoise_device on torch buffers and a stream of its own"""
    import torch
    h, w, _ = color.shape
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_color, d_albedo, d_normal, d_variance = up(color), up(albedo), up(normal), up(variance)
    out = torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda")
    scratch = torch.zeros(vpt.denoise_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        vpt.denoise_device(w, h, ptr(d_color), ptr(d_normal), ptr(d_albedo), ptr(d_variance), out.data_ptr(), scratch.data_ptr(),
                           stream=stream.cuda_stream, **kw)
    stream.synchronize()
    for t, a in ((d_color, color), (d_albedo, albedo), (d_normal, normal), (d_variance, variance)):
        assert t is None or same_bits(t.cpu().numpy(), a), "vpt_denoise_device wrote to an input"
    return out.cpu().numpy()


@pytest.mark.parametrize("case", list(CASES))
def test_the_kernels_give_the_host_mirrors_bits_on_real_renders(vpt, case):
    color, albedo, normal, variance, _ = inputs(vpt, case)
    assert (albedo is None) == (case == "sdfunction_implicit")
    for var in (variance, None):
        want = vpt.denoise_render(color, albedo, normal, var)
        got = vpt.denoise_render(color, albedo, normal, var, device=0)
        assert same_bits(got, want), f"{case}, vpt_denoise: {differing(got, want)}"
        got = device_call(vpt, color, albedo, normal, var)
        assert same_bits(got, want), f"{case}, vpt_denoise_device: {differing(got, want)}"
        assert not same_bits(want[..., :3], color[..., :3]) and same_bits(want[..., 3], color[..., 3])


@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6])
def test_every_stride_and_the_hand_over_between_the_forms(vpt, iterations):
    color, albedo, normal, variance, _ = inputs(vpt, "volume_96")
    for kw in (dict(albedo=albedo, normal=normal, variance=variance), dict(albedo=albedo, normal=normal), dict(normal=normal), dict(albedo=albedo),
               dict()):
        want = vpt.denoise_render(color, iterations=iterations, **kw)
        got = vpt.denoise_render(color, iterations=iterations, device=0, **kw)
        assert same_bits(got, want), f"{sorted(kw)}: {differing(got, want)}"


@pytest.mark.parametrize("w,h", [(1, 1), (3, 7), (63, 9), (65, 8), (131, 45), (200, 17)])
def test_sizes_that_are_no_multiple_of_the_tile(vpt, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    color = (rng.gamma(2.0, 0.3, (h, w, 4))).astype(F)
    albedo = np.round(rng.random((h, w, 4)) * 4).astype(F) / F(4)
    normal = (rng.random((h, w, 4)) * 0.4).astype(F)
    for kw in (dict(albedo=albedo, normal=normal), dict()):
        for iterations, sigmas in ((5, {}), (8, dict(sigma_luminance=2.0, sigma_normal=0.8, sigma_albedo=0.3))):
            want = vpt.denoise_render(color, iterations=iterations, **kw, **sigmas)
            got = vpt.denoise_render(color, iterations=iterations, device=0, **kw, **sigmas)
            assert same_bits(got, want), differing(got, want)
            got = device_call(vpt, color, kw.get("albedo"), kw.get("normal"), None, iterations=iterations, **sigmas)
            assert same_bits(got, want), differing(got, want)


@pytest.mark.parametrize("case", ["volume_96", "volume_1280", "sdfunction_implicit"])
def test_half_variance_on_the_device_gives_the_host_loops_bits(vpt, case):
    import torch
    _, _, _, variance, (sum_a, sum_n, a, n) = inputs(vpt, case)
    h, w, _ = sum_a.shape
    assert same_bits(vpt.half_variance(sum_a, a, sum_n, n, device=0), variance)
    d_a, d_n = torch.from_numpy(sum_a).cuda(), torch.from_numpy(sum_n).cuda()
    d_v = torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        vpt.half_variance_device(w, h, d_a.data_ptr(), a, d_n.data_ptr(), n, d_v.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert same_bits(d_v.cpu().numpy(), variance)
    assert float(variance.max()) > 0


@pytest.mark.parametrize("case", ["volume_96", "volume_1280", "sdfunction_implicit"])
def test_the_plain_and_the_tiled_form_give_the_same_bits(vpt, monkeypatch, case):
    color, albedo, normal, variance, _ = inputs(vpt, case)
    tiled = vpt.denoise_render(color, albedo, normal, variance, iterations=6, device=0)
    blind = vpt.denoise_render(color, iterations=6, device=0)
    monkeypatch.setenv("VPT_DENOISE_PLAIN", "1")
    assert same_bits(vpt.denoise_render(color, albedo, normal, variance, iterations=6, device=0), tiled)
    assert same_bits(vpt.denoise_render(color, iterations=6, device=0), blind)
    monkeypatch.setenv("VPT_DENOISE_PLAIN", "0")
    assert same_bits(vpt.denoise_render(color, albedo, normal, variance, iterations=6, device=0), tiled)


def test_two_calls_give_the_same_bits_and_inputs_stay(vpt):
    color, albedo, normal, variance, _ = inputs(vpt, "volume_96")
    keep = [a.copy() for a in (color, albedo, normal, variance)]
    first = vpt.denoise_render(color, albedo, normal, variance, device=0)
    second = vpt.denoise_render(color, albedo, normal, variance, device=0)
    assert same_bits(first, second)
    assert same_bits(device_call(vpt, color, albedo, normal, variance), first)
    for a, b in zip((color, albedo, normal, variance), keep):
        assert same_bits(a, b)


@pytest.mark.parametrize("name,path,shader,bounces", [("03_volume", SCENE_03, "volpathtrace", 64), ("07_sdfunction_synth", SDFN, "implicit", 6)])
def test_it_pays_on_real_renders(vpt, name, path, shader, bounces):
    """the tracer as its own yardstick: resolution 128, guides at 16 spp, clean image = 2048 spp, default parameters"""
    scene = vpt.HostScene(path)
    dev = vpt.DeviceScene(scene, 0)
    params = vpt.PathtraceParams(resolution=128, samples=2048, shader=shader, bounces=bounces)

    def uniform(n):
        st = scene.make_state(params)
        dev.pathtrace_samples(st, params, n)
        return vpt.get_render(st)

    clean = uniform(2048)
    normal, albedo = vpt.pathtrace_guides(scene, dev, params, 16)
    noisy = {n: uniform(n) for n in (8, 16, 32)}
    spatial = {n: vpt.denoise_render(noisy[n], albedo, normal, device=0) for n in (8, 32)}
    for n in (8, 32):
        ratio = rms(spatial[n], clean) / rms(noisy[n], clean)
        print(f"{name}: {n} spp denoised (spatial seed) {rms(spatial[n], clean):.4f} / {n} spp {rms(noisy[n], clean):.4f} = {ratio:.3f}")
        assert ratio < 1
    ratio = rms(spatial[8], clean) / rms(noisy[16], clean)
    print(f"{name}: 8 spp denoised {rms(spatial[8], clean):.4f} / 16 spp {rms(noisy[16], clean):.4f} = {ratio:.3f}")
    assert ratio < 1
    if name == "07_sdfunction_synth":
        color, variance, _ = render_with_half(vpt, scene, dev, params, 64)
        half = rms(vpt.denoise_render(color, albedo, normal, variance, device=0), clean)
        seed = rms(vpt.denoise_render(color, albedo, normal, device=0), clean)
        print(f"{name}: 64 spp denoised, half variance {half:.4f} / spatial seed {seed:.4f} = {half / seed:.3f} (undenoised {rms(color, clean):.4f})")
        assert half < seed
    dev.close()


# ---- ypathtrace --denoise -------------------------------------------------------------------------------------------------------
BIN = os.path.join(os.path.dirname(GOLDEN), os.pardir, "volumetric-path-tracer_amd", "ypathtrace")


def run(*args):
    import subprocess
    return subprocess.run([os.path.normpath(BIN), *args], capture_output=True, text=True, timeout=600)


def png_pixels(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), np.uint8)


def test_cli_denoise_writes_what_the_python_pipeline_computes(vpt, tmp_path):
    """--denoise: the render split at half its samples for the half variance, guides at --denoiseguides spp, the filter on GPU 0; the
    same steps through the Python binding give the same 8-bit image.  --batch and --gpus 1 do not change it; without --denoise the
    program prints and writes what it did before."""
    common = ["--scene", SCENE_03, "--shader", "volpathtrace", "--samples", "9", "--resolution", "96", "--bounces", "64"]
    a, b, c = str(tmp_path / "a.png"), str(tmp_path / "b.png"), str(tmp_path / "c.png")
    r = run(*common, "--output", a, "--denoise", "--denoiseguides", "4", "--denoiseiters", "4", "--denoisesigmalum", "3")
    assert r.returncode == 0, r.stderr
    assert "rendered 96x40 x 9 spp" in r.stdout and "denoised: guides 4 spp" in r.stdout and "filter 4 passes (half variance)" in r.stdout, r.stdout
    scene = vpt.HostScene(SCENE_03)
    dev = vpt.DeviceScene(scene, 0)
    params = vpt.PathtraceParams(resolution=96, samples=9, shader="volpathtrace", bounces=64)
    color, variance, _ = render_with_half(vpt, scene, dev, params, 9)
    normal, albedo = vpt.pathtrace_guides(scene, dev, params, 4)
    want = vpt.denoise_render(color, albedo, normal, variance, iterations=4, sigma_luminance=3.0)
    assert np.array_equal(png_pixels(a), vpt.linear_to_srgb8(want, 1)[..., :3])
    r = run(*common, "--output", b, "--denoise", "--denoiseguides", "4", "--denoiseiters", "4", "--denoisesigmalum", "3", "--batch", "2", "--gpus", "1")
    assert r.returncode == 0, r.stderr
    assert open(a, "rb").read() == open(b, "rb").read()
    r = run(*common, "--output", c)
    assert r.returncode == 0 and "denoised" not in r.stdout and r.stdout.count("\n") == 1, r.stdout
    assert np.array_equal(png_pixels(c), vpt.linear_to_srgb8(color, 1)[..., :3])
    dev.close()


def test_cli_denoise_after_adaptive_sampling_uses_the_spatial_seed(vpt, tmp_path):
    out = str(tmp_path / "a.png")
    r = run("--scene", SDFN, "--shader", "implicit", "--samples", "32", "--resolution", "96", "--bounces", "6", "--adaptive", "0.1", "--adaptivemin", "8",
            "--adaptivestep", "8", "--output", out, "--denoise", "--denoiseguides", "2")
    assert r.returncode == 0, r.stderr
    assert "adaptive:" in r.stdout and "denoised: guides 2 spp" in r.stdout and "(spatial variance)" in r.stdout, r.stdout
    scene = vpt.HostScene(SDFN)
    dev = vpt.DeviceScene(scene, 0)
    params = vpt.PathtraceParams(resolution=96, samples=32, shader="implicit", bounces=6)
    st = scene.make_state(params)
    dev.pathtrace_adaptive(st, params, 0.1, 8, 8)
    normal, albedo = vpt.pathtrace_guides(scene, dev, params, 2)
    assert albedo is None
    want = vpt.denoise_render(vpt.get_render_hits(st), None, normal)
    assert np.array_equal(png_pixels(out), vpt.linear_to_srgb8(want, 1)[..., :3])
    dev.close()
