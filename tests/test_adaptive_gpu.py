"""Adaptive sampling on the MI355X (vpt_render_adaptive / vpt_render_device_adaptive / vpt_resolve_hits_device, include/vpt.h):
a pixel that stops after k samples holds the state k uniform samples leave, bit for bit, on K1, K2, the curves instance, spilled
stacks and the kernels' own forms; the stop decisions are the documented rule, replayed in numpy float32; the limits (threshold 0,
a huge threshold, the launch schedule left alone); the per-pixel resolve; and that it pays against a uniform render of the same
sample count."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, SCENE_03

pytestmark = pytest.mark.gpu

RES = 96
SDFN = os.path.join(GOLDEN, "scenes", "07_sdfunction_synth", "sdfunction_synth.json")
CURVES = os.path.join(GOLDEN, "scenes", "09_curves_synth", "curves.json")
CAP, STEP, MIN = 64, 4, 8

# name -> (scene, shader, bounces, environment switches)
CASES = {
    "volume": (SCENE_03, "volpathtrace", 64, {}),
    "sdfunction_implicit": (SDFN, "implicit", 6, {}),
    "curves": (CURVES, "volpathtrace", 8, {}),
    "volume_spilled": (SCENE_03, "volpathtrace", 64, {"VPT_STACK_LDS": "4"}),
    "volume_own_forms": (SCENE_03, "volpathtrace", 64, {"VPT_NO_GROUP_FORMS": "1"}),
}


def _scene(vpt, path):
    scene = vpt.HostScene(path)
    return scene, vpt.DeviceScene(scene, 0)


def _uniform(scene, dev, params, k):
    st = scene.make_state(params)
    dev.pathtrace_samples(st, params, k)
    return st


def _adaptive(scene, dev, params, threshold, min_samples=MIN, step=STEP):
    st = scene.make_state(params)
    rounds, taken = dev.pathtrace_adaptive(st, params, threshold, min_samples, step)
    return st, rounds, taken


def _spread(scene, dev, params):
    """an adaptive render whose threshold leaves at least three distinct sample counts"""
    for threshold in (0.05, 0.1, 0.2, 0.03, 0.4, 0.02):
        st, rounds, taken = _adaptive(scene, dev, params, threshold)
        if len(np.unique(st.hits)) >= 3:
            return st, threshold, rounds, taken
    pytest.fail(f"no threshold left three distinct sample counts: {np.unique(st.hits)}")


@pytest.mark.parametrize("case", list(CASES))
def test_each_pixel_replays_the_uniform_chain(vpt, monkeypatch, case):
    path, shader, bounces, switches = CASES[case]
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    scene, dev = _scene(vpt, path)
    params = vpt.PathtraceParams(resolution=RES, samples=CAP, shader=shader, bounces=bounces)
    st, threshold, rounds, taken = _spread(scene, dev, params)
    ks = np.unique(st.hits)
    print(f"{case}: threshold {threshold}, {rounds} rounds, {taken} samples of {st.hits.size * CAP}, hits {ks.tolist()}")
    assert taken == int(st.hits.sum()) and st.samples == int(ks.max())
    assert rounds == -(-int(ks.max()) // STEP)
    assert ks.min() >= MIN and ks.max() <= CAP and all(k % STEP == 0 for k in ks)
    for k in ks:
        ref = _uniform(scene, dev, params, int(k))
        sel = st.hits == k
        assert np.array_equal(st.image[sel].view(np.uint32), ref.image[sel].view(np.uint32)), f"hits {k}: radiance sums differ"
        assert np.array_equal(st.rngs[sel], ref.rngs[sel]), f"hits {k}: RNG states differ"


def test_pixels_follow_the_oracle_at_their_own_count(vpt, oracle):
    scene, dev = _scene(vpt, SCENE_03)
    params = vpt.PathtraceParams(resolution=RES, samples=CAP, shader="volpathtrace", bounces=64)
    st, _, _, _ = _spread(scene, dev, params)
    flat_hits = st.hits.reshape(-1)
    pick = np.random.default_rng(7).choice(flat_hits.size, 64, replace=False)
    same = 0
    for k in np.unique(flat_hits[pick]):
        idx = np.ascontiguousarray(pick[flat_hits[pick] == k], np.int32)
        cpu = scene.make_state(params)
        oracle.oracle_render(scene, params, cpu, int(k), pixels=idx)
        same += int(np.all(st.rngs.reshape(-1, 2)[idx] == cpu.rngs.reshape(-1, 2)[idx], axis=-1).sum())
    print(f"pixels with the oracle's RNG end state at their own sample count: {same} / 64")
    # float32 libm differences (ocml vs glibc) may flip a discrete path decision in a rare pixel (smoke(): >= 0.995)
    assert same >= 63


def _replay(lums, entry, threshold, min_samples, step, cap):
    """the rule of include/vpt.h in numpy float32 over the luminance sums after each uniform call of `step` samples: predicted hits,
    and a mask of the pixels whose decision value came within 1e-5 relative of the threshold"""
    f = np.float32
    shape = lums[0].shape
    lum_prev, mean, m2 = entry.copy(), np.zeros(shape, f), np.zeros(shape, f)
    active, hits, close = np.ones(shape, bool), np.zeros(shape, np.int32), np.zeros(shape, bool)
    h, n = 0, 0
    for L in lums:
        m = min(step, cap - h)
        h, n = h + m, n + 1
        b = (L - lum_prev) / f(m)
        delta = b - mean
        new_mean = mean + delta / f(n)
        new_m2 = m2 + delta * (b - new_mean)
        lum_prev = np.where(active, L, lum_prev)
        mean, m2 = np.where(active, new_mean, mean), np.where(active, new_m2, m2)
        hits = np.where(active, h, hits)
        done = np.full(shape, h >= cap)
        if threshold > 0 and n >= 2 and h >= min_samples:
            var = m2 / (f(n) * f(n - 1))
            tol = f(threshold) * np.maximum(mean, f(1.0 / 256.0))
            tol2 = tol * tol
            done |= var <= tol2
            close |= active & (np.abs(var - tol2) <= f(1e-5) * tol2)
        active &= ~done
        if h >= cap:
            break
    return hits, close


def test_decisions_follow_the_documented_rule(vpt):
    scene, dev = _scene(vpt, SCENE_03)
    params = vpt.PathtraceParams(resolution=RES, samples=CAP, shader="volpathtrace", bounces=64)
    st, threshold, _, _ = _spread(scene, dev, params)
    uni = scene.make_state(params)
    lum = lambda s: (s.image[..., 0] + s.image[..., 1] + s.image[..., 2]) / np.float32(3)
    entry, lums = lum(uni), []
    while uni.samples < CAP:
        dev.pathtrace_samples(uni, params, STEP)
        lums.append(lum(uni))
    want, close = _replay(lums, entry, threshold, MIN, STEP, CAP)
    print(f"threshold {threshold}: {int(close.sum())} pixels within 1e-5 of the threshold, "
          f"{int((want != st.hits)[~close].sum())} decisions differ")
    assert np.array_equal(st.hits[~close], want[~close])


def test_limits(vpt):
    scene, dev = _scene(vpt, SCENE_03)
    params = vpt.PathtraceParams(resolution=RES, samples=CAP, shader="volpathtrace", bounces=64)
    # threshold 0: the uniform render of the cap, hits included
    st, rounds, taken = _adaptive(scene, dev, params, 0.0)
    ref = _uniform(scene, dev, params, CAP)
    assert st.samples == CAP and rounds == CAP // STEP and taken == st.hits.size * CAP
    for a, b in ((st.image, ref.image), (st.hits, ref.hits), (st.rngs, ref.rngs)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # a huge threshold: every pixel stops once n >= 2 and hits >= min_samples, in whole rounds
    for min_samples, step in ((10, 4), (3, 4), (8, 3)):
        st, _, _ = _adaptive(scene, dev, params, 1e6, min_samples, step)
        expect = min(CAP, max(-(-min_samples // step) * step, 2 * step))
        assert (st.hits == expect).all(), (min_samples, step, np.unique(st.hits))
    # preview (samples == 1): one round of the pixel-centre branch
    prev = vpt.PathtraceParams(resolution=RES, samples=1, shader="volpathtrace", bounces=64)
    st, rounds, _ = _adaptive(scene, dev, prev, 0.1, 1, STEP)
    ref = _uniform(scene, dev, prev, 1)
    assert rounds == 1 and np.array_equal(st.image.view(np.uint32), ref.image.view(np.uint32)) and np.array_equal(st.rngs, ref.rngs)
    # bad arguments and a state whose hits differ are refused before anything renders
    bad = scene.make_state(params)
    bad.hits[0, 0] = 1
    with pytest.raises(vpt.VptError):
        dev.pathtrace_adaptive(bad, params, 0.1, MIN, STEP)
    assert bad.hits[0, 0] == 1 and (bad.hits.reshape(-1)[1:] == 0).all()


def _device_state(vpt, st):
    import torch
    layout = vpt.VptLayout(st.width, st.height, 8, 8, 0, 1)
    slots = vpt.layout_slots(layout)
    bufs = (torch.zeros((slots, 4), dtype=torch.float32, device="cuda"), torch.zeros((slots,), dtype=torch.int32, device="cuda"),
            torch.zeros((slots, 2), dtype=torch.int64, device="cuda"))
    vpt.state_upload(layout, st, *(b.data_ptr() for b in bufs))
    return layout, bufs


def test_device_entry_point_and_schedule(vpt):
    import torch
    scene, dev = _scene(vpt, SCENE_03)
    params = vpt.PathtraceParams(resolution=RES, samples=CAP, shader="volpathtrace", bounces=64)
    host, threshold, rounds, taken = _spread(scene, dev, params)
    # the device-resident entry point gives the host one's state
    layout, bufs = _device_state(vpt, scene.make_state(params))
    got = dev.render_device_adaptive(params, layout, *(b.data_ptr() for b in bufs), threshold, MIN, STEP)
    torch.cuda.synchronize()
    assert got == (rounds, taken)
    out = scene.make_state(params)
    vpt.state_download(layout, *(b.data_ptr() for b in bufs), out)
    for a, b in ((out.image, host.image), (out.hits, host.hits), (out.rngs, host.rngs)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert dev.last_kernel_ms() > 0
    # uniform device renders on this handle and layout afterwards equal those of a fresh handle (the schedule record is untouched)
    _, fresh = _scene(vpt, SCENE_03)
    results = []
    for d in (dev, fresh):
        layout, bufs = _device_state(vpt, scene.make_state(params))
        for _ in range(2):
            d.render_device(params, layout, 16, *(b.data_ptr() for b in bufs))
        torch.cuda.synchronize()
        s = scene.make_state(params)
        vpt.state_download(layout, *(b.data_ptr() for b in bufs), s)
        results.append(s)
    for a, b in ((results[0].image, results[1].image), (results[0].hits, results[1].hits), (results[0].rngs, results[1].rngs)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_resolve_hits(vpt):
    import torch
    scene, dev = _scene(vpt, SCENE_03)
    params = vpt.PathtraceParams(resolution=RES, samples=CAP, shader="volpathtrace", bounces=64)
    st, _, _, _ = _spread(scene, dev, params)
    for state in (st, _uniform(scene, dev, params, 12)):
        layout, (img, hit, _) = _device_state(vpt, state)
        rows = torch.zeros((state.height, state.width, 4), dtype=torch.float32, device="cuda")
        vpt.resolve_hits_device(layout, img.data_ptr(), hit.data_ptr(), rows.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(rows.cpu().numpy().view(np.uint32), vpt.get_render_hits(state).view(np.uint32))
    uni = torch.zeros_like(rows)
    vpt.resolve_device(layout, img.data_ptr(), 12, uni.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(rows.cpu().numpy().view(np.uint32), uni.cpu().numpy().view(np.uint32))


def _srgb(linear):
    x = np.clip(linear[..., :3].astype(np.float64), 0, None)
    return np.clip(np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1 / 2.4) - 0.055), 0, 1)


def test_it_pays(vpt):
    scene, dev = _scene(vpt, SCENE_03)
    cap = 256
    params = vpt.PathtraceParams(resolution=128, samples=cap, shader="volpathtrace", bounces=64)
    ref_params = vpt.PathtraceParams(resolution=128, samples=1024, shader="volpathtrace", bounces=64)
    ref = _srgb(vpt.get_render(_uniform(scene, dev, ref_params, 1024)))
    pixels = ref.shape[0] * ref.shape[1]
    for threshold in (0.02, 0.03, 0.05, 0.08, 0.12, 0.2):
        st, rounds, taken = _adaptive(scene, dev, params, threshold, 16, 16)
        if taken <= 0.6 * pixels * cap:
            break
    assert taken <= 0.6 * pixels * cap
    spp = taken // pixels
    uni = _uniform(scene, dev, params, spp)
    rms = lambda img: float(np.sqrt(np.mean((_srgb(img) - ref) ** 2)))
    a, u = rms(vpt.get_render_hits(st)), rms(vpt.get_render(uni))
    print(f"threshold {threshold}: {rounds} rounds, {taken / (pixels * cap):.3f} of the cap's samples ({spp} spp uniform); "
          f"RMS vs 1024 spp: adaptive {a:.5f}, uniform {u:.5f}")
    assert a <= u
