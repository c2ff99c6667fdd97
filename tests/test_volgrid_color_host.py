"""Coloured extinction of the volgrid shader (include/vpt.h: vpt_scene_set_volgrid_color), the host side of csrc/vpt_volgrid_rule.h: the
chroma rows against float64 -log(clip(color)), and the event of a carrier collision against float64 on a small table."""
import numpy as np
import pytest

from test_volgrid_host import F, load

EPS = 2.0 ** -24   # half an ulp of float32, relative: the bound of one rounding


def chroma_of(vpt, colors):
    """the chroma rows of `overlap` with `colors` on its grid instances' materials"""
    scene = load(vpt, "overlap")
    for g, color in enumerate(colors):
        m = scene.material(scene.volume_instance(g).material)
        m.color[:] = [float(c) for c in color]
        scene.set_material(scene.volume_instance(g).material, m)
    scene.update_bvh()
    return scene, scene.volgrid_chroma()


def k64(color):
    c = np.asarray(color, np.float64)
    return -np.log(np.clip(np.where(np.isnan(c), 1e-4, c.astype(F).astype(np.float64)), np.float64(F(1e-4)), 1.0))


@pytest.mark.parametrize("c", [0.5, 0.2, 0.9999, 0.37, 1e-4, 3e-5, 0.0, -1.0, np.nan, 1.0 - 2.0 ** -24])
def test_k_is_within_two_ulp_of_float64(vpt, c):
    """colour (c, 1, 1): kmax is k of the one absorbing channel; colours below 1e-4 and NaN clamp to 1e-4"""
    _, rows = chroma_of(vpt, [(c, 1.0, 1.0), (1.0, c, 2.0)])
    want = k64([c])[0]
    for row, lead in zip(rows, (0, 1)):
        assert abs(np.float64(row["kmax"]) - want) <= 2 * np.spacing(F(want)), (row, want)
        assert row["kmax"] > 0 and np.array_equal(row["a"], np.eye(3, dtype=F)[lead]) and not np.any(np.signbit(row["a"]))


def test_structure_of_the_rows(vpt):
    scene, rows = chroma_of(vpt, [(0.5, 0.7, 0.9), (1.0, 1.5, np.inf)])
    k = k64([0.5, 0.7, 0.9])
    assert rows[0]["a"][0] == 1 and np.all(np.abs(rows[0]["a"] - k / k[0]) <= 6 * EPS * (k / k[0]))   # logf 2 ulp twice, one division
    trdepth = F(scene.material(scene.volume_instance(0).material).trdepth)
    assert rows[0]["trdepth_eff"] == trdepth / rows[0]["kmax"] and np.all(rows[0]["whd"] > 0)         # one float32 division
    # transparent: colour >= 1 in every channel
    assert rows[1]["kmax"] == 0 and np.all(rows[1]["a"] == 0) and np.all(rows[1]["whd"] == 0)
    assert rows[1]["trdepth_eff"] == F(scene.material(scene.volume_instance(1).material).trdepth)


def event(vpt, a, w, u):
    rows = np.ascontiguousarray(np.concatenate([np.asarray(a, F), np.asarray(w, F), np.asarray(u, F)[:, None]], axis=1))
    n = len(rows)
    kind, draws, out, prob = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 3), F), np.zeros(n, F)
    vpt.host.vpth_volgrid_event(n, rows.ctypes.data, kind.ctypes.data, out.ctypes.data, prob.ctypes.data, draws.ctypes.data)
    return kind, out, prob, draws


A = np.array([(1, 0.5, 0.2), (1, 0.5, 0.2), (0.3, 1, 0.9), (0.25, 0.25, 1), (1, 0.999, 0.001), (1, 0.5, 0.2)], F)
W = np.array([(1, 1, 1), (0.1, 2.5, 7), (3, 0.5, 0.25), (1e-3, 4, 2e-2), (1, 1, 1), (0, 1.5, 0)], F)


def test_the_event_against_float64(vpt):
    """P, the scatter weights (u = 0) and the pass weights (u just below 1) within the bound of their roundings - s 1, n 2, s + n 3, P 5
    relative roundings of EPS; a / P 6 and w a / P 7; 1 - P loses 5 P / (1 - P) + 1, the pass weight 4 more - and P w_scatter +
    (1 - P) w_pass = w channel by channel: the estimator is unbiased"""
    a, w = A.astype(np.float64), W.astype(np.float64)
    s, n = (w * a).max(axis=1), (w * (1 - a)).max(axis=1)
    P = s / (s + n)
    assert np.all((P > 0.05) & (P < 0.95))
    kind, scat, p32, draws = event(vpt, A, W, np.zeros(len(A)))
    assert np.all(kind == 1) and np.all(draws == 1) and np.all(np.abs(p32 - P) <= 5 * EPS * P)
    assert np.all(np.abs(scat - w * a / P[:, None]) <= 7 * EPS * (w * a / P[:, None]))
    kind, passed, p_again, _ = event(vpt, A, W, np.full(len(A), F(1) - F(2.0 ** -24)))
    assert np.all(kind == 0) and np.array_equal(p_again, p32)
    want = w * (1 - a) / (1 - P)[:, None]
    assert np.all(np.abs(passed - want) <= (5 * P / (1 - P) + 5)[:, None] * EPS * want)
    mean = p32.astype(np.float64)[:, None] * scat + (1 - p32.astype(np.float64))[:, None] * passed
    assert np.all(np.abs(mean - w) <= 8 * EPS * w)
    # u decides at P itself: u < P scatters, u == P passes
    kind, _, _, _ = event(vpt, np.repeat(A[:1], 2, axis=0), np.repeat(W[:1], 2, axis=0), [np.nextafter(p32[0], F(0)), p32[0]])
    assert list(kind) == [1, 0]


def test_an_event_without_chromatic_nulls_reads_no_number_and_a_dead_path_ends(vpt):
    a = np.array([(1, 1, 1), (1, 1, 1), (1, 0.5, 0.2), (0.3, 1, 0.9)], F)
    w = np.array([(1, 1, 1), (0.3, 7, 1e-6), (2, 0, 0), (0, 0.4, 0)], F)    # equal channels; weight only where a_c == 1
    for u in (0.0, 0.999):
        kind, out, prob, draws = event(vpt, a, w, np.full(4, u))
        assert np.all(kind == 1) and np.all(draws == 0) and np.all(prob == 1) and np.array_equal(out.view(np.uint32), (w * a).view(np.uint32))
    assert np.array_equal(event(vpt, a[:2], w[:2], np.zeros(2))[1].view(np.uint32), w[:2].view(np.uint32))   # a = 1: the weight's own bits
    bad = np.array([(0, 0, 0), (np.nan, np.nan, np.nan), (0, -0.0, 0)], F)
    kind, out, _, draws = event(vpt, a[:3], bad, np.zeros(3))
    assert np.all(kind == 2) and np.all(draws == 0) and np.array_equal(out.view(np.uint32), bad.view(np.uint32))
