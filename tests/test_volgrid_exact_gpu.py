"""The volgrid kernel (K3, csrc/vpt_volgrid_kernel.hip.h) against the float64 references of tests/volgrid_exact.py.

Ray level: DeviceScene.volgrid_track flies the kernel's own vg_start / vg_track_step (compiled in K3's unit) on given rays, once per
stream of make_state at 256 x 256 (S = 65 536 flights per ray, a whole ray set in one call).  The flights of every ray are held to
the unconditional distribution 1 - exp(-tau(t)) of the exact optical depth by Kolmogorov's statistic, sqrt(S) D <= 2.2 (the host test
shows the same statistic rejecting a medium 5 % denser on every one of these rays), to exact facts about collisions and escapes, and
the probe itself to K3 in place: one-sample renders replayed bit for bit.

Path level: renders at 48 x 48, at most 1 024 spp, against reference_paths - analytic free flights, plain weights, no roulette, no MIS -
over the pixels whose footprint lies in x, y in [0.25, 0.75]: z = (gpu - ref) / sqrt(se_gpu^2 + se_ref^2) per channel, |z| <= 5, both
standard errors <= 0.5 % of the reference mean.

Measured on an MI355X (brick walk / one majorant per volume):
  worst sqrt(S) D per scene   ramp 1.221 / 1.355, sparse 1.191 / 1.434, rotated 1.550 / 1.565, overlap 1.080 / 1.080 (limit 2.2)
  share of instance 0         17 rays, all within 1.55 binomial standard errors (limit 5)
  two slabs, z                g = +0.6: +0.35 / +0.19; g = -0.6: +1.17 / +1.38; g = 0: -0.90 / -0.58
  coloured, 64 bounces, z     no MIS (+0.99, +0.11, -0.39) / (-0.14, -0.49, -0.79); MIS (+0.35, +0.08, +0.50) / (+0.33, -0.07, +0.25)
  truncation, z               1: -0.05 (closed form: +0.64 standard errors); 2: (-1.24, -1.60, -1.91); 4: (-0.98, -1.00, -0.63) /
                              (-0.98, -0.96, -0.80); 5: (-0.06, +0.30, +0.58) / (-0.18, -0.28, -0.19)
  two environments, z         MIS on against off -0.21 / -0.38
(`constant` and `overlap` have one brick per volume: both walks fly the same flights there but for rounding at the box's faces.)
"""
import functools

import numpy as np
import pytest

import volgrid_exact as X
from test_volgrid_exact_host import (EMISSION, KS_LIMIT, S, SCENES, coloured, edge_ray_of_the_sparse_grid, rays_for, region, two_slabs, unit)
from test_volgrid_gpu import CAM_BOX, exterior, interior, medium, need_gpu, params_of, render, walk  # noqa: F401 (walk: a fixture)
from test_volgrid_host import F, load

pytestmark = pytest.mark.gpu

MAX_STEPS = 1 << 20   # VPT_VOLGRID_MAX_STEPS
KAT_CAMERA = 3


def streams(vpt, scene):
    """the 65 536 (state, inc) pairs of make_state at 256 x 256"""
    rng = scene.make_state(vpt.PathtraceParams(camera=CAM_BOX, resolution=256)).rngs.reshape(-1, 2).copy()
    assert rng.shape == (S, 2)
    return rng


def fly(dev, rays, rng):
    """every ray once per stream, in one call: per ray (event, instance, t, steps, rng_out) of S flights each"""
    o = np.repeat(np.array([np.concatenate([o, d]) for _, o, d in rays], F), len(rng), axis=0)
    out = dev.volgrid_track(o, np.tile(rng, (len(rays), 1)))
    return [tuple(a[i * len(rng):(i + 1) * len(rng)] for a in out) for i in range(len(rays))]


def point_at(o, d, t):
    """o + d t in float32: the product, then the sum, as the kernel forms it with contraction off"""
    return (o[None, :] + (d[None, :] * t[:, None]).astype(F)).astype(F)


# ---- 1. - 3. the free flight, ray by ray ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_free_flights_follow_the_exact_optical_depth(vpt, walk, name):
    """sqrt(S) D <= 2.2 for every ray against 1 - exp(-tau(t)); on `overlap` tau is the sum over both instances and the share of
    collisions in instance 0 is within 5 binomial standard errors of its exact value; every collision lies where the medium is"""
    need_gpu(vpt)
    make, count = SCENES[name]
    scene = make(vpt)
    dev = vpt.DeviceScene(scene, 0)
    instances = X.describe(scene, count)
    rays = rays_for(name, instances)
    rng = streams(vpt, scene)
    steps_before = dev.volgrid_stats()["steps"]
    worst = 0.0
    for (label, o, d), (event, instance, t, steps, rng_out) in zip(rays, fly(dev, rays, rng)):
        tau, total = X.optical_depth(instances, o, d)
        assert total >= 0.5
        hit = event == 1
        assert np.all((event == 0) | hit) and np.all(steps >= 1) and np.all(steps < MAX_STEPS), label     # the step bound is never reached
        assert np.all(instance[~hit] == -1) and np.all(t[~hit] == np.finfo(F).max) and np.all((instance[hit] >= 0) & (instance[hit] < count))
        ks = X.ks_sqrt_n(t[hit], S, tau.cdf)
        worst = max(worst, ks)
        print(f"{name} {label}: tau {total:.4f}, collided {hit.mean():.4f} (exact {-np.expm1(-total):.4f}), sqrt(S) D {ks:.3f}")
        assert ks <= KS_LIMIT, f"{name} {label}: sqrt(S) D = {ks:.3f}"
        # a collision lies where the medium is
        sigma, first = dev.volgrid_density(point_at(o, d, t[hit]))
        assert np.all(sigma > 0) and np.all((first >= 0) & (first <= instance[hit])), label
        for g in range(count):
            mine = t[hit & (instance == g)].astype(np.float64)
            t0, t1 = X.box_interval(instances[g], o, d) or (np.inf, -np.inf)    # a box the ray misses holds no collision
            assert np.all((mine >= t0 * (1 - 1e-5)) & (mine <= t1 * (1 + 1e-5))), label
        if count == 2:
            share, n = tau.share(0), int(hit.sum())
            got = float((instance[hit] == 0).mean())
            print(f"   share of instance 0: {got:.4f}, exact {share:.4f}, {(got - share) / np.sqrt(share * (1 - share) / n):+.2f} standard errors")
            assert abs(got - share) <= 5 * np.sqrt(share * (1 - share) / n), label
        assert not np.array_equal(rng_out[hit], rng[hit])
    print(f"{name}: worst sqrt(S) D {worst:.3f} over {len(rays)} rays")
    assert dev.volgrid_stats()["steps"] == steps_before      # the probe does not count into the render's step word


def test_rays_that_meet_no_medium_escape_without_a_draw(vpt, walk):
    need_gpu(vpt)
    scene = SCENES["sparse"][0](vpt)
    dev = vpt.DeviceScene(scene, 0)
    instances = X.describe(scene, 1)
    rng = streams(vpt, scene)[:4096]
    missing = [("past_the_box", np.array([1.5, 0.5, 3.0], F), np.array([0, 0, -1], F)), ("away_from_it", np.array([0.5, 0.5, 3.0], F), np.array([0, 0, 1], F)),
               ("beside_obliquely", np.array([-1.0, -1.0, 0.5], F), unit((1.0, -0.2, 0.1)).astype(F))]
    assert all(X.box_interval(instances[0], o, d) is None for _, o, d in missing)
    if not walk:   # with bricks: a chord through bricks of majorant 0 only is crossed without a draw; one majorant per volume draws there
        o, d = edge_ray_of_the_sparse_grid(instances)
        assert X.box_interval(instances[0], o, d) is not None and X.optical_depth(instances, o, d)[1] == 0.0
        missing.append(("majorant_0_bricks", o, d))
    for (label, o, d), (event, instance, t, steps, rng_out) in zip(missing, fly(dev, missing, rng)):
        assert np.all(event == 0) and np.all(instance == -1) and np.all(t == np.finfo(F).max) and np.array_equal(rng_out, rng), label
        assert np.all(steps >= 1) and np.all(steps < 64), label
    if not walk:
        assert np.all(fly(dev, missing[-1:], rng)[0][3] >= 3)    # it did walk the bricks of its chord
    # an all-zero grid: every ray through it escapes, and no stream moves
    scene.set_volume(0, np.zeros((32, 32, 32), F))
    scene.update_volumes()
    empty = vpt.DeviceScene(scene, 0)
    through = rays_for("sparse", instances)
    for (label, o, d), (event, instance, t, steps, rng_out) in zip(through, fly(empty, through, rng)):
        assert np.all(event == 0) and np.array_equal(rng_out, rng) and np.all(steps >= 1), label


def test_the_probe_refuses_what_it_cannot_fly(vpt):
    need_gpu(vpt)
    scene = load(vpt, "constant")
    dev = vpt.DeviceScene(scene, 0)
    rng = streams(vpt, scene)[:2]
    good = np.array([[0.5, 0.5, 3, 0, 0, -1], [0.5, 0.5, 3, 0, 0, -1]], F)
    assert dev.volgrid_track(good, rng)[0].shape == (2,) and dev.volgrid_track(np.zeros((0, 6), F), np.zeros((0, 2), np.uint64))[0].shape == (0,)
    for bad in ([0.5, np.nan, 3, 0, 0, -1], [0.5, 0.5, np.inf, 0, 0, -1], [0.5, 0.5, 3, 0, 0, -1.01], [0.5, 0.5, 3, 0, 0, 0], [0.5, 0.5, 3, 0, np.nan, -1]):
        rays = good.copy()
        rays[1] = bad
        with pytest.raises(vpt.VptError, match=r"\(-1\)"):
            dev.volgrid_track(rays, rng)
    out = np.zeros(8, np.int32)
    h, p = vpt.hip.vpt_scene_volgrid_track, out.ctypes.data
    assert h(dev.handle, -1, good.ctypes.data, rng.ctypes.data, p, p, p, p, None) == -1
    assert h(dev.handle, 2, None, rng.ctypes.data, p, p, p, p, None) == -1 and h(dev.handle, 2, good.ctypes.data, rng.ctypes.data, p, None, p, p, None) == -1
    assert h(dev.handle, 0, None, None, None, None, None, None, None) == 0
    m = scene.material(0)
    m.trdepth = 0.0
    scene.set_material(0, m)
    dev.update(scene.update_bvh())
    with pytest.raises(vpt.VptError, match=r"\(-1\).*vol_instance 0"):
        dev.volgrid_track(good, rng)


# ---- 4. the probe is what the render runs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["constant", "volgrid"])
def test_one_sample_renders_replay_the_probe_bit_for_bit(vpt, walk, name):
    """albedo 0, no MIS, samples = 1 (the preview branch: pixel centres, two lens draws): the probe on the pixel's camera ray with the
    pixel's stream after its two lens draws collides exactly where the render's alpha is 1, and leaves the stream where the render left
    it - three draws further (rn.x, rn.y, rnl) where the flight collided - on every one of the 4 096 pixels"""
    need_gpu(vpt)
    scene = medium(vpt, name, albedo=0.0, trdepth=0.25 if name == "volgrid" else 1.0 / np.log(2.0))
    dev = vpt.DeviceScene(scene, 0)
    p = vpt.PathtraceParams(camera=CAM_BOX, resolution=64, shader="volgrid", samples=1, bounces=8, noimplicit_mis=True)
    st = scene.make_state(p)
    rng = st.rngs.reshape(-1, 2).copy()
    dev.pathtrace_samples(st, p, 1)
    h, w = st.height, st.width
    assert (h, w) == (64, 64)
    rng, lens_u = X.rand1f(rng)
    rng, lens_v = X.rand1f(rng)
    rec = np.zeros((h, w, 5), F)
    rec[..., 0] = CAM_BOX
    rec[..., 1] = ((np.arange(w, dtype=F) + F(0.5)) / F(w))[None, :]
    rec[..., 2] = ((np.arange(h, dtype=F) + F(0.5)) / F(h))[:, None]
    rec[..., 3], rec[..., 4] = lens_u.reshape(h, w), lens_v.reshape(h, w)
    rays = dev.kat(KAT_CAMERA, rec.reshape(-1, 5))
    event, instance, t, steps, rng_out = dev.volgrid_track(rays, rng)
    alpha = st.image[..., 3].reshape(-1)
    assert np.all((alpha == 0) | (alpha == 1)) and 100 < alpha.sum() < h * w - 100
    assert np.array_equal(event == 1, alpha == 1) and np.all(event != 2)
    after = np.where((event == 1)[:, None], X.rng_skip(rng_out, 3), rng_out)
    assert np.array_equal(after, st.rngs.reshape(-1, 2))
    assert np.array_equal(st.image[..., 0].reshape(-1), np.where(event == 1, F(0), F(0.5)))


# ---- 5. paths against the float64 path tracer --------------------------------------------------------------------------------------------------
def edit_material(scene, index, albedo, g, trdepth, emission=(0, 0, 0)):
    m = scene.material(index)
    m.scattering[:] = [float(a) for a in np.ones(3) * albedo]
    m.scanisotropy, m.trdepth = float(g), float(trdepth)
    m.emission[:] = [float(e) for e in emission]
    scene.set_material(index, m)


@functools.lru_cache(maxsize=None)
def reference(case, arg, paths):
    """(mean (3,), standard error (3,)) of reference_paths for a case, over the rectangle of the compared pixels; computed once"""
    _, rect = region()
    boxes, env, bounces = (two_slabs(arg), 0.0, 8) if case == "slabs" else coloured(arg)
    return X.mean_and_se(X.reference_paths(boxes, env, bounces, paths, 17, rect)[0])


def gpu_mean(st, n):
    """(mean (3,), standard error (3,)) over the compared pixels: their sums are independent"""
    mask, _ = region()
    assert mask.shape == st.image.shape[:2] and mask.sum() >= 200
    means = st.image[mask][:, :3].astype(np.float64) / n
    return means.mean(axis=0), means.std(axis=0, ddof=1) / np.sqrt(len(means))


def assert_agree(what, got, ref):
    (gm, gs), (rm, rs) = got, ref
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (gm - rm) / np.sqrt(gs ** 2 + rs ** 2)
    print(f"{what}: gpu {gm} +- {gs}, reference {rm} +- {rs}, z {z}")
    for c in range(3):
        if rm[c] == 0 and rs[c] == 0:
            assert gm[c] == 0, what          # nothing can reach this channel
        else:
            assert gs[c] <= 0.005 * rm[c] and rs[c] <= 0.005 * rm[c], f"{what}: channel {c} says nothing"
            assert abs(z[c]) <= 5, f"{what}: channel {c}: z = {z[c]:+.2f}"
    return z


def test_emission_of_a_black_medium_is_exact(vpt, walk):
    """albedo 0: a sample is the environment (it escaped) or the emission (it collided), image[c] == 0.5 (N - alpha) + e_c alpha bit for
    bit: all terms are multiples of 0.25 below 2^14"""
    need_gpu(vpt)
    N = 4096
    scene = medium(vpt, "constant", albedo=0.0, trdepth=1.0 / np.log(2.0), emission=EMISSION)
    st = render(vpt, scene, vpt.DeviceScene(scene, 0), params_of(vpt, 64, N, 8, mis=False))
    alpha = st.image[..., 3].astype(np.float64)
    for c in range(3):
        assert np.array_equal(st.image[..., c].astype(np.float64), 0.5 * (N - alpha) + EMISSION[c] * alpha)
    assert np.all(alpha[interior(CAM_BOX, 64, 0.0, 1.0)] > 0) and np.all(alpha[exterior(CAM_BOX, 64, 0.0, 1.0)] == 0)
    inside = alpha[interior(CAM_BOX, 64, 0.0, 1.0)] / N
    assert abs(inside.mean() - 0.5) < 5 * 0.5 / np.sqrt(N * inside.size)     # optical depth ln 2


def slab_scene(vpt, g):
    scene = load(vpt, "overlap")
    scene.set_volume_instance(1, frame=[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1.5])      # behind instance 0: z in [-1.5, -0.5]
    scene.update_volumes()
    scene.set_environment(0, emission=(0, 0, 0))
    scene.update_textures()
    edit_material(scene, 0, 1.0, g, 1.0)
    edit_material(scene, 1, 0.0, 0.0, 0.25, EMISSION)
    scene.update_bvh()
    return scene


@pytest.mark.parametrize("g", [0.6, -0.6, 0.0])
def test_the_direction_of_scattering(vpt, walk, g):
    """a white slab over a black emitter under a black sky: what reaches the emitter depends on which way g scatters (the reference's
    g = +0.6 and -0.6 are > 100 standard errors apart: test_volgrid_exact_host.py)"""
    need_gpu(vpt)
    scene = slab_scene(vpt, g)
    inst = X.describe(scene, 2)
    assert X.box_interval(inst[1], (0.5, 0.5, 3.0), (0, 0, -1.0)) == pytest.approx((3.5, 4.5))
    st = render(vpt, scene, vpt.DeviceScene(scene, 0), params_of(vpt, 48, 1024, 8, mis=False))
    assert_agree(f"two slabs, g = {g:+.1f}", gpu_mean(st, 1024), reference("slabs", g, 1 << 19))


def coloured_scene(vpt):
    scene = load(vpt, "constant")
    edit_material(scene, 0, (0.9, 0.5, 0.2), 0.6, 0.5, (0.0, 0.1, 0.0))
    scene.update_bvh()
    return scene


@pytest.mark.parametrize("mis", [False, True], ids=["no_mis", "mis"])
def test_colour_roulette_and_long_paths(vpt, walk, mis):
    """albedo (0.9, 0.5, 0.2), g = 0.6, emission, 64 bounces: the roulette (from bounce 4 on) and, with MIS on, weights f / (0.5 f + 0.5 p)
    that are not 1 - both held to a reference that has neither"""
    need_gpu(vpt)
    scene = coloured_scene(vpt)
    assert len(scene.lights()[0]) == 1
    st = render(vpt, scene, vpt.DeviceScene(scene, 0), params_of(vpt, 48, 1024, 64, mis=mis))
    assert_agree(f"coloured, 64 bounces, {'MIS' if mis else 'no MIS'}", gpu_mean(st, 1024), reference("coloured", 64, 1 << 19))


@pytest.mark.parametrize("bounces", [0, 1, 2, 4, 5])
def test_truncation_at_the_bounce_limit(vpt, walk, bounces):
    """the same medium cut at 0, 1, 2, 4 and 5 collisions, around the roulette's first bounce (> 3) and the `bounce >= bounces` exit"""
    need_gpu(vpt)
    scene = coloured_scene(vpt)
    st = render(vpt, scene, vpt.DeviceScene(scene, 0), params_of(vpt, 48, 1024, bounces, mis=False))
    if bounces == 0:
        assert np.all(st.image == 0) and np.all(st.hits == 1024)
        return
    got = gpu_mean(st, 1024)
    assert_agree(f"coloured, {bounces} bounces", got, reference("coloured", bounces, 1 << 19))
    if bounces == 1:   # 0.5 T + e (1 - T): the first flight alone
        T = np.exp(-1.0 / float(scene.material(0).trdepth) * X.bbox_of(X.describe(scene, 1)[0])[2])
        want = 0.5 * T + np.array([0.0, 0.1, 0.0]) * (1 - T)
        print(f"   closed form {want}, {(got[0] - want) / got[1]} standard errors")
        assert np.all(np.abs(got[0] - want) <= 5 * got[1])


def test_two_environments_white_furnace_is_exact(vpt, walk):
    """two untextured environments of 0.25 each: vg_env_light(k = 1) and the summed vg_env_pdf.  0.25 + 0.25 and the pdf (a + a) / 2 are
    exact, so f / (0.5 f + 0.5 f) = 1 and every sample is 0.5"""
    need_gpu(vpt)
    scene = medium(vpt, "two_env", albedo=1.0, g=0.0, trdepth=1.0)
    assert len(scene.lights()[0]) == 2
    st = render(vpt, scene, vpt.DeviceScene(scene, 0), params_of(vpt, 64, 64, 1024, mis=True))
    assert np.all(st.image[..., :3] == F(32.0)) and st.image[..., 3].max() > 0


def test_two_environments_with_mis_agree_with_the_same_scene_without(vpt, walk):
    """A consistency check of the kernel with itself: MIS on against MIS off of the same scene, admissible only because the MIS-off path
    is held to the float64 reference in the tests above.  Camera 1, zoomed on the block; every pixel is compared."""
    need_gpu(vpt)
    scene = medium(vpt, "two_env", albedo=0.8, g=0.6, trdepth=0.25)
    dev = vpt.DeviceScene(scene, 0)
    out = []
    for mis in (True, False):
        st = render(vpt, scene, dev, params_of(vpt, 48, 1024, 16, camera=1, mis=mis))
        means = st.image[..., :3].reshape(-1, 3).astype(np.float64) / 1024
        out.append((means.mean(axis=0), means.std(axis=0, ddof=1) / np.sqrt(len(means))))
    assert_agree("two environments, MIS on against off", out[0], out[1])
