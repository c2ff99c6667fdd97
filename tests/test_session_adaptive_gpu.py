"""Adaptive sampling in a render session on the MI355X (include/vpt.h: vpt_adaptive_run, vpt_session_set_adaptive).
The criterion is equality of bits with the calls a session stands for: make_state + vpt_render_adaptive in any batching of the
advances, the per-pixel resolve, the noise planes against a numpy float32 replay of the rule from the kernel's own inputs, the
filter's output against the host mirror handed that variance; then the limits, the edits, the run object on device buffers, the
refusals and the command line."""
import os
import re
import subprocess

import numpy as np
import pytest

import scene_edits as E
from conftest import GOLDEN, ROOT, SCENE_03
from test_denoise_host import box3

pytestmark = pytest.mark.gpu

F = np.float32
RES = 96
CAP, STEP, MIN = 64, 4, 8
GRID = os.path.join(GOLDEN, "scenes", "06_gridsdf_synth", "gridsdf_synth.json")
CURVES = os.path.join(GOLDEN, "scenes", "09_curves_synth", "curves.json")
BIN = os.path.join(ROOT, "volumetric-path-tracer_amd", "ypathtrace")
CASES = {"volume": (SCENE_03, "volpathtrace", 64), "gridsdf": (GRID, "implicit", 4), "curves": (CURVES, "volpathtrace", 8)}
THRESHOLDS = (0.05, 0.1, 0.2, 0.03, 0.4, 0.02)   # the list tests/test_adaptive_gpu.py picks from

_cache = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def same_state(a, b):
    return a.samples == b.samples and same_bits(a.image, b.image) and np.array_equal(a.hits, b.hits) and np.array_equal(a.rngs, b.rngs)


def params_of(vpt, name, samples=CAP, resolution=RES):
    _, shader, bounces = CASES[name]
    return vpt.PathtraceParams(resolution=resolution, samples=samples, shader=shader, bounces=bounces)


def adaptive_render(vpt, scene, dev, params, threshold, min_samples=MIN, step=STEP):
    st = scene.make_state(params)
    rounds, taken = dev.pathtrace_adaptive(st, params, threshold, min_samples, step)
    return st, rounds, taken


def case(vpt, name):
    """(scene, device scene, params, threshold, the state pathtrace_adaptive leaves at that threshold, its rounds, its samples): the
    first threshold of the list that leaves at least three distinct sample counts, found once per scene by the existing entry point"""
    if name not in _cache:
        scene = vpt.HostScene(CASES[name][0])
        dev = vpt.DeviceScene(scene, 0)
        params = params_of(vpt, name)
        for threshold in THRESHOLDS:
            st, rounds, taken = adaptive_render(vpt, scene, dev, params, threshold)
            if len(np.unique(st.hits)) >= 3:
                break
        else:
            pytest.fail(f"{name}: no threshold left three distinct sample counts: {np.unique(st.hits)}")
        print(f"{name}: threshold {threshold}, {rounds} rounds, {taken} samples of {st.hits.size * CAP}, hits {np.unique(st.hits).tolist()}")
        _cache[name] = (scene, dev, params, threshold, st, rounds, taken)
    return _cache[name]


# ---- 1: any batching -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_any_batching_of_the_advances_gives_the_adaptive_render(vpt, name):
    scene, dev, params, threshold, want, rounds, taken = case(vpt, name)
    s = vpt.RenderSession(dev, params, adaptive=(threshold, MIN, STEP))
    assert s.samples == 0 and s.progress() == (0, 0, want.hits.size) and (s.hits() == 0).all()
    for batching in ((64,), (4,) * 16, (12, 1, 64)):
        s.reset()
        for n in batching:
            s.advance(n)
        assert same_state(s.state(), want), batching
        assert s.progress() == (rounds, taken, 0) and s.converged() and s.samples == want.samples
    # exactly five rounds: the adaptive render whose cap is 20
    s.reset()
    assert s.advance(20) == 20
    p20 = params_of(vpt, name, samples=20)
    want20, rounds20, taken20 = adaptive_render(vpt, scene, dev, p20, threshold)
    assert same_state(s.state(), want20) and s.progress()[:2] == (5, taken20) and rounds20 == 5
    assert s.progress()[2] == int((want.hits > 20).sum())   # the pixels that go on are those the full render takes further
    # one round is fewer samples than min_samples: a uniform render of 4
    s.reset()
    assert s.advance(3) == 4
    uniform = scene.make_state(params)
    dev.pathtrace_samples(uniform, params, 4)
    assert same_state(s.state(), uniform) and s.progress() == (1, 4 * want.hits.size, want.hits.size)
    s.close()


# ---- 2, 3: the per-pixel resolve and the noise planes on a frame with partial tiles ----------------------------------------------
@pytest.fixture(scope="module")
def frame100(vpt):
    """03_volume at 100 x 42: partial 8x8 tiles on the right and bottom edges; the guides of the denoising session"""
    scene, dev, _, threshold, _, _, _ = case(vpt, "volume")
    params = params_of(vpt, "volume", resolution=100)
    normal, albedo = vpt.pathtrace_guides(scene, dev, params, samples=4)
    return scene, dev, params, threshold, normal, albedo


def test_the_image_is_the_per_pixel_resolve_on_partial_tiles(vpt, frame100):
    scene, dev, params, threshold, _, _ = frame100
    want, rounds, taken = adaptive_render(vpt, scene, dev, params, threshold)
    s = vpt.RenderSession(dev, params, adaptive=(threshold, MIN, STEP))
    assert s.size == (100, 42)
    s.advance(CAP)
    state = s.state()
    assert same_state(state, want) and len(np.unique(state.hits)) >= 2
    assert same_bits(s.image(), vpt.get_render_hits(state))
    assert np.array_equal(s.hits(), state.hits) and s.hits().dtype == np.int32
    assert np.array_equal(s.display(), vpt.tonemap_image(s.image(), as_bytes=True, device=0))
    s.close()


def replay_se2(m2, hits, step):
    """the rule of vpt_adaptive_run_noise_device in numpy float32"""
    n = (hits + step - 1) // step
    with np.errstate(divide="ignore", invalid="ignore"):
        se2 = m2 / (n.astype(F) * (n - 1).astype(F))
    return np.where(n >= 2, se2, F(0)).astype(F)


def test_the_noise_planes_replay_the_rule_and_reach_the_filter(vpt, frame100):
    scene, dev, params, threshold, normal, albedo = frame100
    s = vpt.RenderSession(dev, params, denoise=True, guide_samples=4, adaptive=(threshold, MIN, STEP))
    with pytest.raises(vpt.VptError):
        s.noise()   # nothing has rendered
    with pytest.raises(vpt.VptError):
        s.adaptive_stats()
    s.advance(5 * STEP)
    assert s.progress()[0] == 5
    (mean, m2), hits = s.adaptive_stats(), s.hits()
    assert len(np.unique(hits)) >= 2 and (m2 >= 0).all() and (mean >= 0).all()
    want_se2 = replay_se2(m2, hits, STEP)
    want_var = box3(want_se2)
    se2, var = s.noise()
    assert same_bits(se2, want_se2), int((bits(se2) != bits(want_se2)).sum())
    assert same_bits(var, want_var), int((bits(var) != bits(want_var)).sum())
    assert (se2 > 0).any()
    image = s.image()
    want = vpt.denoise_render(image, albedo, normal, var)
    assert same_bits(s.image(denoised=True), want)
    assert not same_bits(want, vpt.denoise_render(image, albedo, normal, None))   # the variance handed over is used
    assert np.array_equal(s.display(), vpt.tonemap_image(want, as_bytes=True, device=0))
    # one round: no estimate yet, the filter takes its spatial seed
    s.reset()
    s.advance(STEP)
    assert s.progress()[0] == 1
    se2, var = s.noise()
    assert not se2.any() and not var.any()
    assert same_bits(s.image(denoised=True), vpt.denoise_render(s.image(), albedo, normal, None))
    s.close()


# ---- 4: limits ---------------------------------------------------------------------------------------------------------------------
def test_limits(vpt):
    scene, dev, params, threshold, _, _, _ = case(vpt, "volume")
    s = vpt.RenderSession(dev, params)
    with pytest.raises(vpt.VptError):
        s.progress()   # the mode is off
    with pytest.raises(vpt.VptError):
        s.hits()
    pixels = s.size[0] * s.size[1]
    # a huge threshold: every pixel stops once n >= 2 and hits >= min_samples, in whole rounds; then an advance is a no-op
    for min_samples, step in ((10, 4), (3, 4), (8, 3)):
        s.set_adaptive(1e6, min_samples, step)
        s.advance(CAP)
        expect = min(CAP, max(-(-min_samples // step) * step, 2 * step))
        assert (s.hits() == expect).all(), (min_samples, step, np.unique(s.hits()))
        assert s.progress() == (expect // step, expect * pixels, 0) and s.samples == expect
        state, display = s.state(), s.display()
        assert s.advance(8) == expect and s.stats() == (0, 0, 0)
        assert same_state(s.state(), state) and np.array_equal(s.display(), display)
    # threshold 0: the session without the mode, advanced to the cap
    s.set_adaptive(0.0, MIN, STEP)
    s.advance(24), s.advance(CAP)
    plain = vpt.RenderSession(dev, params)
    plain.advance(CAP)
    assert same_state(s.state(), plain.state()) and same_bits(s.image(), plain.image())
    assert np.array_equal(s.display(), plain.display()) and same_bits(s.display(as_bytes=False), plain.display(as_bytes=False))
    assert s.progress() == (CAP // STEP, CAP * pixels, 0)
    # the mode switched off: the session of before
    s.set_adaptive(None)
    assert s.samples == 0
    with pytest.raises(vpt.VptError):
        s.progress()
    assert s.advance(3) == 3
    plain.reset()
    plain.advance(3)
    assert same_state(s.state(), plain.state()) and same_bits(s.image(), plain.image())
    s.close(), plain.close()


# ---- 5: edits ----------------------------------------------------------------------------------------------------------------------
def test_an_edit_drops_the_run_and_the_render_restarts_on_the_edited_scene(vpt):
    _, _, params, threshold, _, _, _ = case(vpt, "volume")
    edited = vpt.HostScene(SCENE_03)
    dev = vpt.DeviceScene(vpt.HostScene(SCENE_03), 0)
    s = vpt.RenderSession(dev, params, adaptive=(threshold, MIN, STEP))
    s.advance(3 * STEP)
    assert s.progress()[0] == 3
    E.edit_camera(edited)
    s.edit(edited.update_bvh())
    assert s.progress()[:2] == (0, 0) and s.samples == 0 and (s.hits() == 0).all()
    s.advance(CAP)
    fresh = vpt.RenderSession(vpt.DeviceScene(edited, 0), params, adaptive=(threshold, MIN, STEP))
    fresh.advance(CAP)
    assert same_state(s.state(), fresh.state()) and same_bits(s.image(), fresh.image()) and s.progress() == fresh.progress()
    # an edit the scene refuses: the run goes on where it was
    s.reset()
    s.advance(3 * STEP)
    with pytest.raises(vpt.VptError):
        s.edit(vpt.SceneEdit(cameras={99: edited.camera(0)}))
    assert s.progress()[0] == 3
    s.advance(CAP)
    assert same_state(s.state(), fresh.state())
    s.close(), fresh.close()


# ---- 6: the run object on device buffers -------------------------------------------------------------------------------------------
def device_state(vpt, st):
    import torch
    layout = vpt.VptLayout(st.width, st.height, 8, 8, 0, 1)
    slots = vpt.layout_slots(layout)
    bufs = (torch.zeros((slots, 4), dtype=torch.float32, device="cuda"), torch.zeros((slots,), dtype=torch.int32, device="cuda"),
            torch.zeros((slots, 2), dtype=torch.int64, device="cuda"))
    vpt.state_upload(layout, st, *(b.data_ptr() for b in bufs))
    return layout, bufs


@pytest.mark.parametrize("stacks", ["plain", "spilled"])
def test_a_run_in_pieces_equals_the_one_call_form(vpt, monkeypatch, stacks):
    import torch
    _, _, params, threshold, _, _, _ = case(vpt, "volume")
    if stacks == "spilled":
        monkeypatch.setenv("VPT_STACK_LDS", "4")   # read when the scene is created: the traversal stacks spill to HBM
    scene = vpt.HostScene(SCENE_03)
    dev = vpt.DeviceScene(scene, 0)
    layout, bufs = device_state(vpt, scene.make_state(params))
    run = dev.adaptive_run(params, layout, *(b.data_ptr() for b in bufs), threshold, MIN, STEP)
    assert run.progress() == (0, 0, layout.width * layout.height, 0)
    parts = [run.rounds(2), run.rounds(1), run.rounds(10**6)]
    torch.cuda.synchronize()
    assert parts[0][0] == 2 and parts[1][0] == 1 and parts[2][2] == 0
    assert run.rounds() == (0, 0, 0) and run.rounds(5) == (0, 0, 0)
    total = (sum(p[0] for p in parts), sum(p[1] for p in parts))
    assert run.progress()[:3] == (total[0], total[1], 0)
    assert dev.last_kernel_ms() > 0
    layout2, bufs2 = device_state(vpt, scene.make_state(params))
    whole = dev.render_device_adaptive(params, layout2, *(b.data_ptr() for b in bufs2), threshold, MIN, STEP)
    torch.cuda.synchronize()
    assert whole == total
    a, b = scene.make_state(params), scene.make_state(params)
    vpt.state_download(layout, *(x.data_ptr() for x in bufs), a)
    vpt.state_download(layout2, *(x.data_ptr() for x in bufs2), b)
    for x, y in ((a.image, b.image), (a.hits, b.hits), (a.rngs, b.rngs)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert len(np.unique(a.hits)) >= 3
    # the planes of the run against the state it left
    se2 = torch.full((a.height, a.width), -1.0, dtype=torch.float32, device="cuda")
    hits = torch.full((a.height, a.width), -1, dtype=torch.int32, device="cuda")
    mean, m2, var = torch.zeros_like(se2), torch.zeros_like(se2), torch.zeros_like(se2)
    run.noise_device(se2.data_ptr(), hits.data_ptr())
    run.stats_device(mean.data_ptr(), m2.data_ptr())
    vpt.box3_device(a.width, a.height, se2.data_ptr(), var.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(hits.cpu().numpy(), a.hits)
    want = replay_se2(m2.cpu().numpy(), a.hits, STEP)
    assert same_bits(se2.cpu().numpy(), want) and same_bits(var.cpu().numpy(), box3(want))
    run.close()


# ---- 7: refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_session_alone(vpt):
    _, dev, params, threshold, _, _, _ = case(vpt, "volume")
    s = vpt.RenderSession(dev, params, adaptive=(threshold, MIN, STEP))
    s.advance(2 * STEP)
    before = (s.samples, s.progress(), s.display())
    assert before[0] == 2 * STEP and before[1][0] == 2
    for bad in ((float("nan"), MIN, STEP), (float("inf"), MIN, STEP), (-0.1, MIN, STEP), (threshold, MIN, 0), (threshold, 0, STEP),
                (threshold, CAP + 1, STEP)):
        with pytest.raises(vpt.VptError):
            s.set_adaptive(*bad)
        assert (s.samples, s.progress()) == before[:2] and np.array_equal(s.display(), before[2]), bad
    with pytest.raises(vpt.VptError, match="min_samples"):
        s.reset(params=params_of(vpt, "volume", samples=MIN - 1))
    assert (s.samples, s.progress()) == before[:2] and np.array_equal(s.display(), before[2]) and s.params.samples == CAP
    assert s.adaptive == (threshold, MIN, STEP)
    s.advance(STEP)
    assert s.progress()[0] == 3   # and it goes on
    s.close()


# ---- 8: the command line -----------------------------------------------------------------------------------------------------------
def test_cli_converge_stops_early_and_writes_its_frames(vpt, tmp_path):
    _, _, _, threshold, want, rounds, taken = case(vpt, "volume")
    out = tmp_path / "conv.png"
    r = subprocess.run([BIN, "--scene", SCENE_03, "--shader", "volpathtrace", "--resolution", str(RES), "--bounces", "64", "--samples", str(CAP),
                        "--progressive", str(STEP), "--converge", repr(threshold), "--adaptivemin", str(MIN), "--output", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    m = re.search(r"converge: (\d+) rounds, (\d+) samples taken of (\d+) \([0-9.]+ %\), (\d+) pixels still rendering", r.stdout)
    assert m, r.stdout
    got = tuple(int(x) for x in m.groups())
    assert got[2] == 96 * 40 * CAP and got[1] < got[2] and got[3] == 0
    assert got[:2] == (rounds, taken)   # the session of the command line is the adaptive render of test 1
    written = sorted(p.name for p in tmp_path.iterdir())
    assert written == sorted(["conv.png"] + ["conv.%06d.png" % (k * STEP) for k in range(rounds + 1)])
    from PIL import Image
    assert np.asarray(Image.open(out)).shape == (40, 96, 4)
