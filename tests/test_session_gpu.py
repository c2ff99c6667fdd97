"""Progressive rendering on the MI355X (include/vpt.h: vpt_session and its three device stages).  The criterion is
equality of bits wherever the rule holds no libm call: make_state on the device against the host's, the tone map without the sRGB curve
against the host mirror (which tests/test_session_host.py holds to the reference's own table), a session against the sequence of calls
it stands for - make_state + vpt_render, the upscale of a vpt_render preview, the host denoising pipeline.  With the sRGB curve the
device's powf stands where the mirror has glibc's: bytes within one count on fewer than 1e-3 of the channels (the project's own
conditions for the same powf, tests/test_gpu_parity.py), floats within a measured ULP distance."""
import os
import subprocess

import numpy as np
import pytest

import scene_edits as E
from conftest import GOLDEN, ROOT, SCENE_03

pytestmark = pytest.mark.gpu

F = np.float32
TABLE = os.path.join(GOLDEN, "tonemap_table.npz")
GRID = os.path.join(GOLDEN, "scenes", "06_gridsdf_synth", "gridsdf_synth.json")
CURVES = os.path.join(GOLDEN, "scenes", "09_curves_synth", "curves.json")
BIN = os.path.join(ROOT, "volumetric-path-tracer_amd", "ypathtrace")
GRID6 = [(e, f) for e in (0.0, -2.5, 1.25) for f in (False, True)]   # the table's exposure x filmic grid

# name -> (scene file, shader, resolution, bounces); every session renders up to 8 samples with a preview of 1 / 8
SESSIONS = {"volume": (SCENE_03, "volpathtrace", 128, 8), "gridsdf": (GRID, "implicit", 96, 4), "curves": (CURVES, "volpathtrace", 96, 8)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def same_state(a, b):
    return a.samples == b.samples and same_bits(a.image, b.image) and np.array_equal(a.hits, b.hits) and np.array_equal(a.rngs, b.rngs)


def ulp_distance(a, b):
    """largest distance between two float32 arrays in units in the last place (finite values; -0 and +0 are 0 apart)"""
    def key(x):
        i = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max())


# ---- make_state on the device ---------------------------------------------------------------------------------------------------
def device_state(torch, slots, fill):
    """(image, hits, rng) device buffers of `slots` slots filled with a pattern no state holds"""
    return (torch.full((slots, 4), fill, dtype=torch.float32, device="cuda"), torch.full((slots,), -7, dtype=torch.int32, device="cuda"),
            torch.full((slots, 2), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda"))


@pytest.mark.parametrize("resolution", [1280, 100, 3840])
def test_state_init_device_equals_make_state(vpt, scene03, resolution):
    import torch
    want = scene03.make_state(vpt.PathtraceParams(resolution=resolution))
    layout = vpt.VptLayout(want.width, want.height, 8, 8, 0, 1)
    slots = vpt.layout_slots(layout)
    img, hits, rng = device_state(torch, slots, 3.5)
    vpt.state_init_device(layout, img.data_ptr(), hits.data_ptr(), rng.data_ptr())
    got = want.copy()
    got.image[:], got.hits[:], got.rngs[:] = 1, 1, 1
    vpt.state_download(layout, img.data_ptr(), hits.data_ptr(), rng.data_ptr(), got)
    assert same_state(got, want)
    pad = torch.from_numpy(vpt.layout_pixel_index(layout) < 0).cuda()   # padding slots stay as they were
    assert bool((img[pad] == 3.5).all()) and bool((hits[pad] == -7).all()) and bool((rng[pad] == 0x5A5A5A5A5A5A5A5A).all())


@pytest.mark.parametrize("nranks", [2, 4])
@pytest.mark.parametrize("resolution,tile", [(100, 8), (1280, 16)])
def test_state_init_device_writes_this_ranks_pixels_only(vpt, scene03, nranks, resolution, tile):
    import torch
    want = scene03.make_state(vpt.PathtraceParams(resolution=resolution))
    got = want.copy()
    got.image[:], got.hits[:], got.rngs[:] = 9, 9, 9   # prefilled: a pixel no rank wrote would keep this
    owner = np.full(want.width * want.height, -1)
    for rank in range(nranks):
        layout = vpt.VptLayout(want.width, want.height, tile, tile, rank, nranks)
        slots = vpt.layout_slots(layout)
        img, hits, rng = device_state(torch, slots, 3.5)
        vpt.state_init_device(layout, img.data_ptr(), hits.data_ptr(), rng.data_ptr())
        index = vpt.layout_pixel_index(layout)
        pad = torch.from_numpy(index < 0).cuda()
        assert bool((img[pad] == 3.5).all()) and bool((hits[pad] == -7).all()) and bool((rng[pad] == 0x5A5A5A5A5A5A5A5A).all())
        assert (owner[index[index >= 0]] == -1).all()
        owner[index[index >= 0]] = rank
        before = got.copy()
        vpt.state_download(layout, img.data_ptr(), hits.data_ptr(), rng.data_ptr(), got)
        mine = (owner == rank).reshape(want.height, want.width)
        assert same_bits(got.image[~mine], before.image[~mine]) and np.array_equal(got.rngs[~mine], before.rngs[~mine])   # others' pixels untouched
    assert (owner >= 0).all() and same_state(got, want)


# ---- the tone map -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def render320(vpt, scene03, dev03):
    """the input of tests/test_gpu_parity.py::test_device_output_stage_matches_host_quantisation: 03_volume, 320 wide, 8 spp"""
    p = vpt.PathtraceParams(resolution=320, samples=8, shader="volpathtrace", bounces=8)
    st = scene03.make_state(p)
    dev03.pathtrace_samples(st, p, 8)
    return vpt.get_render(st)


def test_tonemap_without_srgb_equals_the_host_mirror_bit_for_bit(vpt, render320):
    table = np.load(TABLE)["inputs"].reshape(32, 32, 4)
    for name, image in (("table", table), ("render", render320)):
        for exposure, filmic in GRID6:
            want, want8 = vpt.tonemap_image(image, exposure, filmic, False), vpt.tonemap_image(image, exposure, filmic, False, as_bytes=True)
            got, got8 = vpt.tonemap_image(image, exposure, filmic, False, device=0), vpt.tonemap_image(image, exposure, filmic, False, as_bytes=True, device=0)
            assert same_bits(got, want), (name, exposure, filmic, int((bits(got) != bits(want)).sum()))
            assert np.array_equal(got8, want8), (name, exposure, filmic)


def test_tonemap_device_writes_both_displays_at_once(vpt, render320):
    import torch
    h, w, _ = render320.shape
    src = torch.from_numpy(render320).cuda()
    out_f, out_b = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda"), torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    vpt.tonemap_device(w, h, src.data_ptr(), out_f.data_ptr(), out_b.data_ptr(), vpt.DisplayParams(1.25, True, False))
    torch.cuda.synchronize()
    assert same_bits(out_f.cpu().numpy(), vpt.tonemap_image(render320, 1.25, True, False))
    assert np.array_equal(out_b.cpu().numpy(), vpt.tonemap_image(render320, 1.25, True, False, as_bytes=True))


def test_tonemap_with_srgb_bytes_stay_within_one_count_of_the_host_mirror(vpt, render320):
    """the conditions of tests/test_gpu_parity.py:382-383 for the same powf, on that test's input and its filmic and exposure variants"""
    for exposure, filmic in GRID6:
        got = vpt.tonemap_image(render320, exposure, filmic, True, as_bytes=True, device=0).astype(np.int32)
        ref = vpt.tonemap_image(render320, exposure, filmic, True, as_bytes=True).astype(np.int32)
        diff = np.abs(got - ref)
        print(f"srgb bytes, exposure {exposure}, filmic {filmic}: max {diff.max()}, share {(diff != 0).mean():.2e}")
        assert diff.max() <= 1, (exposure, filmic)
        assert (diff != 0).mean() < 1e-3, (exposure, filmic)


SRGB_FLOAT_MAX_ULP = 4   # measured on MI355X over the inputs below (ocml's powf against glibc's through the curve); DESIGN.md §13


def test_tonemap_with_srgb_floats_stay_within_twice_the_measured_distance(vpt, render320):
    """ULP distance of the float display to the host mirror on fixed inputs; the bound is twice the measured maximum, the margin being
    for another build of ocml"""
    table = np.load(TABLE)["inputs"].reshape(32, 32, 4)
    worst = 0
    for image in (table, render320):
        for exposure, filmic in GRID6:
            got, ref = vpt.tonemap_image(image, exposure, filmic, True, device=0), vpt.tonemap_image(image, exposure, filmic, True)
            assert same_bits(got[..., 3], ref[..., 3])
            worst = max(worst, ulp_distance(got[..., :3], ref[..., :3]))
    print("srgb float display: largest ULP distance to the host mirror", worst)
    assert worst <= 2 * SRGB_FLOAT_MAX_ULP


def test_upscale_device_equals_the_host_upscale(vpt):
    import torch
    for pratio, (pw, ph), (w, h) in ((1, (37, 11), (37, 11)), (3, (43, 17), (131, 53)), (8, (16, 6), (131, 53)), (64, (2, 1), (131, 53))):
        preview = np.random.default_rng(pratio).random((ph, pw, 4)).astype(F)
        src, out = torch.from_numpy(preview).cuda(), torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        vpt.upscale_device(pratio, pw, ph, src.data_ptr(), w, h, out.data_ptr())
        torch.cuda.synchronize()
        assert same_bits(out.cpu().numpy(), vpt.upscale_preview(preview, pratio, w, h)), pratio


# ---- a session against the sequence of calls it stands for --------------------------------------------------------------------------
def params_of(vpt, name, samples=8, resolution=None):
    _, shader, res, bounces = SESSIONS[name]
    return vpt.PathtraceParams(resolution=resolution or res, samples=samples, shader=shader, bounces=bounces)


def preview_image(vpt, scene, dev, params, pratio, size):
    """reset_display's preview through the host-state path: make_state at resolution / pratio, one vpt_render pass with samples = 1
    (the pixel-centre branch), get_render, replicated to `size`"""
    pp = vpt.PathtraceParams(params.camera, params.resolution // pratio, params.shader, 1, params.bounces, params.noparallel,
                             params.noimplicit_mis, params.spheretrace_maxiter)
    st = scene.make_state(pp)
    dev.pathtrace_samples(st, pp, 1)
    return vpt.upscale_preview(vpt.get_render(st), pratio, *size)


def rendered(vpt, scene, dev, params, n):
    st = scene.make_state(params)
    dev.pathtrace_samples(st, params, n)
    return st


@pytest.mark.parametrize("name", list(SESSIONS))
def test_a_session_equals_the_calls_it_stands_for(vpt, name):
    scene = vpt.HostScene(SESSIONS[name][0])
    dev = vpt.DeviceScene(scene, 0)
    params, pratio = params_of(vpt, name), 8
    s = vpt.RenderSession(dev, params, pratio=pratio, display=vpt.DisplayParams(0.0, False, True))
    fresh = scene.make_state(params)
    assert s.size == (fresh.width, fresh.height) and s.samples == 0
    # after a reset: the state of make_state, the image of the preview, the display its tone map
    image0, state0, bytes0, floats0 = s.image(), s.state(), s.display(), s.display(as_bytes=False)
    assert same_state(state0, fresh)
    assert same_bits(image0, preview_image(vpt, scene, dev, params, pratio, s.size))
    assert np.array_equal(bytes0, vpt.tonemap_image(image0, as_bytes=True, device=0)) and same_bits(floats0, vpt.tonemap_image(image0, device=0))
    # 3 + 5 samples in two advances: the state of 8 samples of vpt_render, get_render as the image
    assert s.advance(3) == 3 and s.advance(5) == 8
    state8, image8, bytes8 = s.state(), s.image(), s.display()
    want = rendered(vpt, scene, dev, params, 8)
    assert same_state(state8, want)
    assert same_bits(image8, vpt.get_render(want))
    assert np.array_equal(bytes8, vpt.tonemap_image(image8, as_bytes=True, device=0))
    # the cap: nothing happens
    assert s.advance(100) == 8 and s.stats() == (0, 0, 0)
    assert same_state(s.state(), want) and np.array_equal(s.display(), bytes8)
    # another display: the display changes, the state and the image do not
    s.set_display(vpt.DisplayParams(1.25, True, True))
    assert s.samples == 8 and same_state(s.state(), want) and same_bits(s.image(), image8)
    assert np.array_equal(s.display(), vpt.tonemap_image(image8, 1.25, True, True, as_bytes=True, device=0))
    assert not np.array_equal(s.display(), bytes8)
    # a reset starts over: the same preview, and the same 8 samples in another batching
    s.reset()
    assert s.samples == 0 and same_bits(s.image(), image0) and same_state(s.state(), fresh)
    for n in (1, 1, 2, 4):
        s.advance(n)
    assert same_state(s.state(), want)
    s.close()


def test_a_session_edit_equals_a_fresh_scene_and_a_refused_edit_changes_nothing(vpt):
    params = params_of(vpt, "volume")
    edited = vpt.HostScene(SCENE_03)
    dev = vpt.DeviceScene(vpt.HostScene(SCENE_03), 0)
    s = vpt.RenderSession(dev, params)
    s.advance(2)
    E.edit_camera(edited)
    s.edit(edited.update_bvh())
    fresh = vpt.DeviceScene(edited, 0)
    assert s.samples == 0 and same_bits(s.image(), preview_image(vpt, edited, fresh, params, 8, s.size))
    s.advance(3), s.advance(5)
    want = rendered(vpt, edited, fresh, params, 8)
    assert same_state(s.state(), want) and same_bits(s.image(), vpt.get_render(want))
    # an edit vpt_scene_update refuses: the session stays where it was
    s.reset()
    s.advance(4)
    before = (s.state(), s.image(), s.display())
    with pytest.raises(vpt.VptError):
        s.edit(vpt.SceneEdit(cameras={99: edited.camera(0)}))
    assert s.samples == 4 and same_state(s.state(), before[0]) and same_bits(s.image(), before[1]) and np.array_equal(s.display(), before[2])
    s.advance(4)
    assert same_state(s.state(), want)
    s.close()


def test_a_reset_with_another_resolution_resizes_the_session(vpt, scene03, dev03):
    s = vpt.RenderSession(dev03, params_of(vpt, "volume"), pratio=8)
    assert s.size == (128, 53)
    small = params_of(vpt, "volume", resolution=72)
    s.reset(params=small, pratio=3)
    assert s.size == (72, 30) and s.samples == 0
    assert same_bits(s.image(), preview_image(vpt, scene03, dev03, small, 3, s.size))
    s.advance(8)
    assert same_state(s.state(), rendered(vpt, scene03, dev03, small, 8))
    with pytest.raises(vpt.VptError):
        s.reset(pratio=65)
    with pytest.raises(vpt.VptError):
        s.reset(pratio=64, params=params_of(vpt, "volume", resolution=32))   # 32 / 64 < 1
    assert s.size == (72, 30) and s.samples == 8 and s.pratio == 3   # refused resets left it alone
    s.close()


def test_session_create_refuses_bad_parameters(vpt, dev03):
    with pytest.raises(vpt.VptError, match="pratio"):
        vpt.RenderSession(dev03, params_of(vpt, "volume"), pratio=0)
    with pytest.raises(vpt.VptError, match="pratio"):
        vpt.RenderSession(dev03, params_of(vpt, "volume", resolution=4), pratio=8)
    import ctypes as C
    abi = vpt.VptSessionParams(params_of(vpt, "volume").to_abi(), 8, vpt.VptDisplay(0.0, 0, 1), 0, vpt.VptDenoise(5, 4.0, 0.35, 0.1), 16)
    abi.render.shader = 9
    out = C.c_void_p()
    assert vpt.hip.vpt_session_create(dev03.handle, C.byref(abi), C.byref(out)) == -4   # VPT_ERR_UNKNOWN_SHADER


# ---- the denoised display ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["volume", "gridsdf"])
def test_the_denoised_display_equals_the_host_pipeline(vpt, name):
    """advances of 4, 4 and 8 samples walk the snapshot rule: the spatial seed, then a = 4 of n = 8, then a = 8 of n = 16"""
    scene = vpt.HostScene(SESSIONS[name][0])
    dev = vpt.DeviceScene(scene, 0)
    params = params_of(vpt, name, samples=16, resolution=96)
    s = vpt.RenderSession(dev, params, denoise=True, guide_samples=4)
    with pytest.raises(vpt.VptError):
        s.image(denoised=True)   # the preview frame is never filtered
    preview = s.image()
    assert np.array_equal(s.display(), vpt.tonemap_image(preview, as_bytes=True, device=0))
    got = []
    for n in (4, 4, 8):
        s.advance(n)
        got.append((s.samples, s.image(), s.image(denoised=True), s.display()))
    normal, albedo = vpt.pathtrace_guides(scene, dev, params, samples=4)
    assert (albedo is None) == (name == "gridsdf")
    st = scene.make_state(params)
    sums = {}
    for (n, image, filtered, display), a in zip(got, (0, 4, 8)):
        dev.pathtrace_samples(st, params, n - st.samples)
        sums[n] = st.image.copy()
        assert same_bits(image, vpt.get_render(st)), n   # get_image stays unfiltered
        variance = vpt.half_variance(sums[a], a, sums[n], n) if a else None
        want = vpt.denoise_render(vpt.get_render(st), albedo, normal, variance)
        assert same_bits(filtered, want), (n, int(np.any(bits(filtered) != bits(want), axis=-1).sum()))
        assert np.array_equal(display, vpt.tonemap_image(filtered, as_bytes=True, device=0)), n
    s.reset()
    with pytest.raises(vpt.VptError):
        s.image(denoised=True)
    s.close()


# ---- what a call moves ------------------------------------------------------------------------------------------------------------
def test_session_stats_count_what_crosses_the_bus(vpt, dev03):
    s = vpt.RenderSession(dev03, params_of(vpt, "volume"))
    w, h = s.size
    s.advance(4)
    launches, up, down = s.stats()
    assert launches >= 3 and up == 0 and down == 0   # render, resolve, tone map: nothing of the state or the image moves
    s.display()
    assert s.stats() == (0, 0, 4 * w * h)
    s.display(as_bytes=False)
    assert s.stats() == (0, 0, 16 * w * h)
    s.image()
    assert s.stats() == (0, 0, 16 * w * h)
    s.state()
    assert s.stats() == (1, 0, 36 * w * h)
    s.set_display(vpt.DisplayParams(0.5, False, True))
    assert s.stats() == (1, 0, 0)
    s.close()


# ---- the command line -------------------------------------------------------------------------------------------------------------
def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("ext", [".png", ".jpg"])
def test_cli_progressive_writes_the_preview_the_frames_and_the_offline_file(tmp_path, ext):
    common = ["--scene", SCENE_03, "--shader", "volpathtrace", "--samples", "6", "--resolution", "96", "--bounces", "8"]
    offline, out = tmp_path / ("offline" + ext), tmp_path / ("prog" + ext)
    r = run(*common, "--output", str(offline))
    assert r.returncode == 0, r.stderr
    r = run(*common, "--output", str(out), "--progressive", "4", "--pratio", "4")
    assert r.returncode == 0, r.stderr
    assert "rendered 96x40 x 6 spp progressively" in r.stdout
    written = sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("prog"))
    assert written == ["prog.000000" + ext, "prog.000004" + ext, "prog.000006" + ext, "prog" + ext]
    assert open(out, "rb").read() == open(offline, "rb").read()
    from PIL import Image
    preview = np.asarray(Image.open(tmp_path / ("prog.000000" + ext)).convert("RGB"))
    assert preview.shape == (40, 96, 3)
    if ext == ".png":   # the preview is 24 x 10 pixels replicated four times each way
        assert np.array_equal(preview, np.repeat(np.repeat(preview[::4, ::4], 4, axis=0), 4, axis=1))


def test_cli_progressive_tone_maps_and_denoises(tmp_path, vpt):
    common = ["--scene", SCENE_03, "--shader", "volpathtrace", "--samples", "8", "--resolution", "96", "--bounces", "8", "--progressive", "4"]
    a, b, c = tmp_path / "plain.png", tmp_path / "mapped.png", tmp_path / "clean.png"
    for out, extra in ((a, []), (b, ["--exposure", "1.25", "--filmic"]), (c, ["--denoise", "--denoiseguides", "4"])):
        r = run(*common, "--output", str(out), *extra)
        assert r.returncode == 0, r.stderr
    from PIL import Image
    plain, mapped, clean = (np.asarray(Image.open(p)) for p in (a, b, c))
    assert plain.shape == mapped.shape == clean.shape == (40, 96, 4)
    assert not np.array_equal(plain, mapped) and not np.array_equal(plain, clean)
    # the last display frame is the device's tone map of the same image the final file holds through the host's: within one count
    last = np.asarray(Image.open(tmp_path / "mapped.000008.png")).astype(np.int32)
    assert np.abs(last - mapped.astype(np.int32)).max() <= 1
