"""Next-event estimation in the volgrid shader (include/vpt.h: vpt_scene_set_volgrid_nee): the switch on against the switch
off bit for bit where the rule says no light half runs, the bitwise invariants of every shader here with it on, the shadow flight's probe
against the exact optical depth of volgrid_exact.py ray by ray, and paths with the switch on against the float64 reference paths."""
import numpy as np
import pytest

import volgrid_exact as X
from test_volgrid_exact_gpu import assert_agree, coloured_scene, gpu_mean, reference, streams
from test_volgrid_exact_host import SCENES, rays_for
from test_volgrid_gpu import medium, need_gpu, params_of, render, same_state, walk  # noqa: F401 (walk: a fixture)
from test_volgrid_host import F, load

pytestmark = pytest.mark.gpu

MAX_STEPS = 1 << 20   # VPT_VOLGRID_MAX_STEPS
SKY_SAMPLES = 1024    # the directional sky: the count at which both sides meet assert_agree's 0.5 % (measured: DESIGN.md §34)


def handle(vpt, scene, on):
    dev = vpt.DeviceScene(scene, 0)
    dev.set_volgrid_nee(on)
    assert dev.volgrid_nee == on
    return dev


def black_sky(vpt):
    scene = medium(vpt, "constant", albedo=0.8, g=0.6, trdepth=0.25, emission=(0.25, 1.0, 2.0))
    scene.set_environment(0, emission=(0, 0, 0))
    scene.update_textures()
    assert len(scene.lights()[0]) == 0   # E is empty
    return scene


def zero_grid(vpt):
    scene = load(vpt, "volgrid")
    scene.set_volume(0, np.zeros((32, 32, 32), F))
    scene.update_volumes()
    return scene


def scattering_scene(vpt):
    return medium(vpt, "volgrid", albedo=0.8, g=0.6, trdepth=0.25)


# (scene, parameters of the render with the switch on, parameters of the one with it off, whether the medium is hit at all)
NO_LIGHT_HALF = {
    "black_sky": (black_sky, dict(bounces=8), dict(bounces=8), True),
    "noimplicit_mis": (scattering_scene, dict(bounces=8, mis=False), dict(bounces=8, mis=False), True),
    "zero_grid": (zero_grid, dict(bounces=8), dict(bounces=8), False),
    "one_bounce": (scattering_scene, dict(bounces=1, mis=True), dict(bounces=1, mis=False), True),
}


@pytest.mark.parametrize("case", list(NO_LIGHT_HALF))
def test_without_a_light_half_the_switch_changes_no_bit(vpt, walk, case):
    need_gpu(vpt)
    make, on, off, hit = NO_LIGHT_HALF[case]
    scene = make(vpt)
    dev = handle(vpt, scene, True)
    got = render(vpt, scene, dev, params_of(vpt, 48, 16, **on))
    want = render(vpt, scene, handle(vpt, scene, False), params_of(vpt, 48, 16, **off))
    assert same_state(got, want) and (got.image[..., 3].max() > 0) == hit
    assert dev.volgrid_nee_stats() == {"flights": 0, "steps": 0}


@pytest.fixture(scope="module")
def lit(vpt):
    need_gpu(vpt)
    scene = scattering_scene(vpt)
    return scene, handle(vpt, scene, True)


def test_on_differs_from_off_counts_its_flights_and_off_again_is_never_on(vpt, walk, lit):
    scene, dev = lit
    p = params_of(vpt, 48, 8, 8)
    before, track_steps = dev.volgrid_nee_stats(), dev.volgrid_stats()["steps"]
    on = render(vpt, scene, dev, p)
    after = dev.volgrid_nee_stats()
    never = render(vpt, scene, handle(vpt, scene, False), p)
    assert not np.array_equal(on.image, never.image) and np.array_equal(on.hits, never.hits)
    assert after["flights"] > before["flights"] and after["steps"] - before["steps"] > after["flights"] - before["flights"]   # >= 2 steps each
    assert dev.volgrid_stats()["steps"] > track_steps
    dev.set_volgrid_nee(False)
    again = render(vpt, scene, dev, p)
    dev.set_volgrid_nee(True)
    assert same_state(again, never) and same_state(render(vpt, scene, dev, p), on)


def test_three_plus_five_samples_and_a_session_equal_eight(vpt, walk, lit):
    scene, dev = lit
    p = params_of(vpt, 48, 8, 8)
    whole = render(vpt, scene, dev, p, 8)
    parts = scene.make_state(p)
    dev.pathtrace_samples(parts, p, 3)
    dev.pathtrace_samples(parts, p, 5)
    assert same_state(whole, parts)
    s = vpt.RenderSession(dev, p, pratio=4)
    assert s.advance(3) == 3 and s.advance(5) == 8 and same_state(s.state(), whole)
    s.set_volgrid_nee(False)   # the session's own switch: the scene's, then a reset
    assert not dev.volgrid_nee and s.advance(8) == 8
    assert same_state(s.state(), render(vpt, scene, handle(vpt, scene, False), p, 8))
    s.set_volgrid_nee(True)
    assert s.advance(8) == 8 and same_state(s.state(), whole)


def test_adaptive_equals_a_uniform_render_of_each_pixels_own_count(vpt, walk, lit):
    scene, dev = lit
    p = params_of(vpt, 48, 64, 8)
    st = scene.make_state(p)
    rounds, taken = dev.pathtrace_adaptive(st, p, 0.05, min_samples=8, step=8)
    counts = np.unique(st.hits)
    assert len(counts) > 1 and counts.min() >= 8 and counts.max() <= 64 and taken == int(st.hits.sum())
    uniform = scene.make_state(p)
    for n in range(8, 65, 8):
        dev.pathtrace_samples(uniform, p, 8)
        at = st.hits == n
        assert np.array_equal(st.image[at].view(np.uint32), uniform.image[at].view(np.uint32)) and np.array_equal(st.rngs[at], uniform.rngs[at])


def test_the_two_switches_together_are_refused_in_either_order(vpt, lit):
    scene, dev = lit
    p = params_of(vpt, 48, 4, 8)
    want = render(vpt, scene, dev, p)
    with pytest.raises(vpt.VptError, match=r"\(-5\)"):
        dev.set_volgrid_color(True)
    assert dev.volgrid_nee and not dev.volgrid_color and same_state(render(vpt, scene, dev, p), want)
    other = vpt.DeviceScene(scene, 0)
    other.set_volgrid_color(True)
    want = render(vpt, scene, other, p)
    with pytest.raises(vpt.VptError, match=r"\(-5\)"):
        other.set_volgrid_nee(True)
    assert other.volgrid_color and not other.volgrid_nee and same_state(render(vpt, scene, other, p), want)


# ---- the probe ---------------------------------------------------------------------------------------------------------------------------------
def fly(dev, rays, rng):
    """every ray once per stream, in one call: per ray (T, steps, rng_out)"""
    o = np.repeat(np.array([np.concatenate([o, d]) for _, o, d in rays], F), len(rng), axis=0)
    out = dev.volgrid_transmittance(o, np.tile(rng, (len(rays), 1)))
    return [tuple(a[i * len(rng):(i + 1) * len(rng)] for a in out) for i in range(len(rays))]


def test_a_shadow_flight_that_meets_no_medium_is_one_without_a_draw(vpt, walk):
    need_gpu(vpt)
    scene = SCENES["sparse"][0](vpt)
    dev = vpt.DeviceScene(scene, 0)
    instances = X.describe(scene, 1)
    rng = streams(vpt, scene)[:4096]
    missing = [("past_the_box", np.array([1.5, 0.5, 3.0], F), np.array([0, 0, -1], F)), ("away_from_it", np.array([0.5, 0.5, 3.0], F), np.array([0, 0, 1], F))]
    if not walk:   # a chord through bricks of majorant 0 only (one majorant per volume draws there)
        from test_volgrid_exact_host import edge_ray_of_the_sparse_grid
        missing.append(("majorant_0_bricks", *edge_ray_of_the_sparse_grid(instances)))
    for (label, o, d), (T, steps, rng_out) in zip(missing, fly(dev, missing, rng)):
        assert np.all(T == 1.0) and np.array_equal(rng_out, rng) and np.all((steps >= 1) & (steps < 64)), label
    scene.set_volume(0, np.zeros((32, 32, 32), F))
    scene.update_volumes()
    through = rays_for("sparse", instances)
    for (label, o, d), (T, steps, rng_out) in zip(through, fly(vpt.DeviceScene(scene, 0), through, rng)):
        assert np.all(T == 1.0) and np.array_equal(rng_out, rng), label


def test_the_probe_refuses_what_it_cannot_fly(vpt):
    need_gpu(vpt)
    scene = load(vpt, "constant")
    dev = vpt.DeviceScene(scene, 0)
    rng = streams(vpt, scene)[:2]
    good = np.array([[0.5, 0.5, 3, 0, 0, -1], [0.5, 0.5, 3, 0, 0, -1]], F)
    assert dev.volgrid_transmittance(good, rng)[0].shape == (2,) and dev.volgrid_transmittance(np.zeros((0, 6), F), np.zeros((0, 2), np.uint64))[0].shape == (0,)
    for bad in ([0.5, np.nan, 3, 0, 0, -1], [0.5, 0.5, np.inf, 0, 0, -1], [0.5, 0.5, 3, 0, 0, -1.01], [0.5, 0.5, 3, 0, 0, 0], [0.5, 0.5, 3, 0, np.nan, -1]):
        rays = good.copy()
        rays[1] = bad
        with pytest.raises(vpt.VptError, match=r"\(-1\)"):
            dev.volgrid_transmittance(rays, rng)
    out = np.zeros(8, np.int32)
    h, p = vpt.hip.vpt_scene_volgrid_transmittance, out.ctypes.data
    assert h(dev.handle, -1, good.ctypes.data, rng.ctypes.data, p, p, None) == -1
    assert h(dev.handle, 2, None, rng.ctypes.data, p, p, None) == -1 and h(dev.handle, 2, good.ctypes.data, rng.ctypes.data, None, p, None) == -1
    assert h(dev.handle, 0, None, None, None, None, None) == 0
    m = scene.material(0)
    m.trdepth = 0.0
    scene.set_material(0, m)
    dev.update(scene.update_bvh())
    with pytest.raises(vpt.VptError, match=r"\(-1\).*vol_instance 0"):
        dev.volgrid_transmittance(good, rng)


@pytest.mark.parametrize("name", list(SCENES))
def test_the_mean_of_shadow_flights_is_beer_lambert(vpt, walk, name):
    """T lies in [0, 1] with mean exp(-tau), so its variance is at most T (1 - T): at tau = 3 the standard error over 65 536 streams is at
    most 1.7 % of the reference.  |z| <= 5 per ray; on `overlap` tau is the sum over both instances - the product of their transmittances"""
    need_gpu(vpt)
    make, count = SCENES[name]
    scene = make(vpt)
    dev = vpt.DeviceScene(scene, 0)
    instances = X.describe(scene, count)
    rays = [r for r in rays_for(name, instances) if 0.25 <= X.optical_depth(instances, r[1], r[2])[1] <= 3]
    assert len(rays) >= 8
    rng = streams(vpt, scene)
    before = dev.volgrid_stats()["steps"], dev.volgrid_nee_stats()
    for (label, o, d), (T, steps, rng_out) in zip(rays, fly(dev, rays, rng)):
        ref = np.exp(-X.optical_depth(instances, o, d)[1])
        assert np.all((T >= 0) & (T <= 1)) and np.all((steps >= 1) & (steps < MAX_STEPS)), label
        mean, se = T.astype(np.float64).mean(), T.astype(np.float64).std(ddof=1) / np.sqrt(len(T))
        z = (mean - ref) / se
        print(f"{name} {label}: exp(-tau) {ref:.5f}, mean T {mean:.5f}, se {se / ref:.3%} of it, z {z:+.2f}")
        assert se <= 0.02 * ref, label
        assert abs(z) <= 5, f"{name} {label}: z = {z:+.2f}"
        assert not np.array_equal(rng_out, rng)
    assert (dev.volgrid_stats()["steps"], dev.volgrid_nee_stats()) == before   # the probe counts into no stats word


# ---- paths -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounces", [2, 5, 64])
def test_paths_with_the_switch_on_agree_with_the_float64_reference(vpt, walk, bounces):
    """albedo (0.9, 0.5, 0.2), g 0.6, emission, a constant environment, MIS on: 2 bounces is the gate with exactly one light sample, 5 the
    roulette's first bounce, 64 long paths.  Measured z (MI355X, bricks / one majorant): DESIGN.md §34"""
    need_gpu(vpt)
    scene = coloured_scene(vpt)
    dev = handle(vpt, scene, True)
    st = render(vpt, scene, dev, params_of(vpt, 48, 1024, bounces, mis=True))
    assert dev.volgrid_nee_stats()["flights"] > 0
    assert_agree(f"coloured with NEE, {bounces} bounces", gpu_mean(st, 1024), reference("coloured", bounces, 1 << 19))


def test_a_directional_sky_on_agrees_with_off(vpt, walk):
    """A textured (CDF) environment with a bright patch, albedo 0.8, g 0.6: the switch on against off over every pixel of camera 1 -
    admissible because the off path is held to float64 in test_volgrid_exact_gpu.py"""
    need_gpu(vpt)
    scene = medium(vpt, "furnace_tex", albedo=0.8, g=0.6, trdepth=0.25)
    sky = np.full((64, 128, 4), 0.5, F)
    sky[8:24, 16:48, :3] = 4.0
    scene.set_texture(0, sky, linear=True)
    scene.set_environment(0, emission_tex=0)
    scene.update_textures()
    assert scene.lights()[0][0]["cdf_len"] == 64 * 128
    out = []
    for on in (True, False):
        st = render(vpt, scene, handle(vpt, scene, on), params_of(vpt, 48, SKY_SAMPLES, 16, camera=1, mis=True))
        means = st.image[..., :3].reshape(-1, 3).astype(np.float64) / SKY_SAMPLES
        out.append((means.mean(axis=0), means.std(axis=0, ddof=1) / np.sqrt(len(means))))
    assert_agree("a directional sky, NEE on against off", out[0], out[1])
