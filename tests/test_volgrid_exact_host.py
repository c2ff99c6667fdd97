"""The float64 references of tests/volgrid_exact.py on the CPU, and the scenes, rays and path cases that test_volgrid_exact_gpu.py holds the
volgrid kernel to with them.  What is checked here is what makes the GPU tests able to fail:

  - the optical depth against closed forms (1e-12), against itself with every piece halved (1e-9) and against a midpoint sum of the
    host mirror's density lookup (the float32 bound of test_volgrid_host.py);
  - for EVERY test ray: tau_total >= 0.5, and 65 536 flights drawn from the reference's own distribution pass sqrt(S) D <= 2.2 while the
    same flights fail it against a medium 5 % denser (Kolmogorov's limit: P(sqrt(S) D > 2.2) ~ 2 exp(-2 2.2^2) = 1.3e-4 per ray);
  - the path tracer against a white furnace, Beer-Lambert, the one-bounce closed form, and g = +0.6 against g = -0.6 on the two slabs.
Measured here (seeds as committed): self against self at most 1.642 (rotated), 5 % denser at least 3.754 (ramp); g = +0.6 against -0.6: 127 standard errors."""
import numpy as np
import pytest

import volgrid_exact as X
from test_volgrid_gpu import CAM_BOX, medium, spans
from test_volgrid_host import F, U, density_bound, load

S = 65536
KS_LIMIT = 2.2
EMISSION = (0.25, 1.0, 2.0)


# ---- the scenes of the ray-level tests, made with the project's own edit API --------------------------------------------------------------
def rotation_frame(axis, angle, origin):
    """(12,) float32 x, y, z, o: Rodrigues' rotation about `axis` by `angle`, then the translation"""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    return np.concatenate([R[:, 0], R[:, 1], R[:, 2], np.asarray(origin, np.float64)]).astype(F)


def scene_ramp(vpt):
    return medium(vpt, "ramp", trdepth=0.5)


def scene_sparse(vpt):
    return medium(vpt, "volgrid", trdepth=0.1)


def scene_rotated(vpt):
    """11 x 26 x 19 nodes (z, y, x): bricks 2 x 4 x 3, every last brick partial; rotated, translated, scaled"""
    scene = load(vpt, "constant")
    voxels = np.random.default_rng(29).uniform(0.0, 2.0, (11, 26, 19)).astype(F)
    scene.set_volume(0, voxels, res=1.0 / 26)
    scene.set_volume_instance(0, frame=rotation_frame((1, 2, 3), 0.7, (0.2, -0.1, 0.3)), scalef=0.9)
    scene.update_volumes()
    m = scene.material(0)
    m.trdepth = 0.3
    scene.set_material(0, m)
    scene.update_bvh()
    return scene


def scene_overlap(vpt):
    return load(vpt, "overlap")


SCENES = {"ramp": (scene_ramp, 1), "sparse": (scene_sparse, 1), "rotated": (scene_rotated, 1), "overlap": (scene_overlap, 2)}


# ---- the rays ---------------------------------------------------------------------------------------------------------------------------------
def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def world_ray(inst, pl, dl):
    """the float32 world ray of a local point and direction; the direction is a unit vector to float32 rounding"""
    p, d = X.to_world(inst, pl, unit(dl))
    d = d.astype(F)
    return p.astype(F), (d / F(np.sqrt((d.astype(np.float64) ** 2).sum()))).astype(F)


def node32(pl, bbox, w):
    """vpt_volgrid_node_coord in float32, operation for operation"""
    pl, bbox = F(pl), F(bbox)
    c = F(F(F(F(pl * F(2)) / bbox) - F(1)) + F(1)) * F(0.5)
    return F(min(max(c, F(0)), F(1)) * F(w - 1))


def coordinate_on_node(bbox, w, node):
    """a float32 local coordinate whose float32 node coordinate is exactly `node`"""
    up = down = F(np.float64(node) * np.float64(bbox) / (w - 1))
    cand = [up]
    for _ in range(8):   # the neighbours of the rounded quotient, nearest first
        up, down = np.nextafter(up, F(2)), np.nextafter(down, F(-1))
        cand += [up, down]
    hits = [c for c in cand if node32(c, bbox, w) == F(node)]
    assert hits, "no float32 coordinate lands on the node"
    return np.float64(hits[0])


def rays_for(name, instances):
    """the rays of scene `name`: a list of (label, origin, direction), float32 world vectors"""
    inst = instances[0]
    bbox = X.bbox_of(inst)
    c = bbox * np.array([0.513, 0.479, 0.517])       # near the centre, on no node plane
    if name == "overlap":
        c = np.array([0.637, 0.604, 0.517])          # inside both boxes
    out = []

    def through(label, point, dl, back=2.0):
        out.append((label, *world_ray(inst, np.asarray(point) - unit(dl) * back, dl)))

    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                through(f"octant{sx:+d}{sy:+d}{sz:+d}", c, (sx * 1.0, sy * 0.8, sz * 0.6))
    for k, axis in enumerate("xyz"):
        for s in (1, -1):
            through(f"{'+' if s > 0 else '-'}{axis}", c, np.eye(3)[k] * s)
    through("one_zero_component", c, (1.0, 0.0, -0.7))
    through("origin_inside", bbox * np.array([0.45, 0.3, 0.55]) if name != "sparse" else bbox * np.array([0.5, 0.45, 0.52]), (0.3, 1.0, 0.2), back=0.0)
    if name != "sparse":   # the sparse grid is empty there: that ray is an exact fact of the GPU test (majorant-0 bricks only)
        through("edge_region", bbox * np.array([0.06 - 0.3, -0.5, 0.9]), bbox * np.array([0.6, 1.0, 0.0]), back=0.0)
    if name in ("ramp", "sparse"):   # identity frames: an origin exactly on a brick face (node 8 of 17, node 16 of 32 on x)
        w = inst["voxels"].shape[2]
        x_face = coordinate_on_node(bbox[0], w, 8 if name == "ramp" else 16)
        through("in_face_plane", (x_face, 0.2, 0.1), (0.0, 0.6, 0.8), back=0.0)
        through("leaving_face_downwards", (x_face, 0.45, 0.35), (-0.3, 0.1, 0.9), back=0.0)
    return out


def edge_ray_of_the_sparse_grid(instances):
    """the edge-region ray on the sparse grid: it crosses bricks of majorant 0 only"""
    bbox = X.bbox_of(instances[0])
    return world_ray(instances[0], bbox * np.array([0.06 - 0.3, -0.5, 0.9]), bbox * np.array([0.6, 1.0, 0.0]))


@pytest.fixture(scope="module")
def cases(vpt):
    """per scene: (instances, rays, [(tau, tau_total)])"""
    out = {}
    for name, (make, count) in SCENES.items():
        instances = X.describe(make(vpt), count)
        rays = rays_for(name, instances)
        out[name] = (instances, rays, [X.optical_depth(instances, o, d) for _, o, d in rays])
    return out


def test_the_ray_sets_hold_what_the_issue_lists(cases):
    assert {n: len(c[1]) for n, c in cases.items()} == {"ramp": 19, "sparse": 18, "rotated": 17, "overlap": 17}
    for name in ("ramp", "sparse"):
        instances, rays, _ = cases[name]
        inst = instances[0]
        w, node = inst["voxels"].shape[2], (8 if name == "ramp" else 16)
        for label, o, d in rays[-2:]:
            assert node32(o[0], X.bbox_of(inst)[0], w) == F(node), label      # exactly on the brick face, in the kernel's own float32
        assert rays[-2][2][0] == 0 and rays[-1][2][0] < 0                     # inside the face plane; leaving it downwards
    for name in ("ramp", "rotated"):   # the edge-region chord crosses at least three bricks
        instances, rays, taus = cases[name]
        (label, o, d), (tau, _) = [(r, t) for r, t in zip(rays, taus) if r[0] == "edge_region"][0]
        part = tau.parts[0]
        bricks = {tuple(cell // 8) for cell in part.cells}
        assert len(bricks) >= 3, (name, bricks)
    # the rotated grid: 2 x 4 x 3 bricks, the last one partial on every axis
    assert cases["rotated"][0][0]["voxels"].shape == (11, 26, 19) and all((n - 1) % 8 for n in (11, 26, 19))


# ---- tau: closed forms, itself halved, the host mirror ------------------------------------------------------------------------------------------
def test_tau_of_the_constant_grid_is_chord_length_over_trdepth(vpt):
    scene = medium(vpt, "constant", trdepth=0.7)
    instances = X.describe(scene, 1)
    g = np.random.default_rng(3)
    for _ in range(32):
        o, d = g.uniform(-1, 2, 3), unit(g.normal(size=3))
        d = d if g.uniform() < 0.8 else np.eye(3)[g.integers(3)] * g.choice([-1, 1])
        iv = X.box_interval(instances[0], o, d)
        tau, total = X.optical_depth(instances, o, d)
        want = 0.0 if iv is None else (iv[1] - iv[0]) / np.float64(F(0.7))
        assert abs(total - want) <= 1e-12 * max(1.0, want)
        if iv is not None:
            mid = (iv[0] + iv[1]) / 2
            assert abs(tau(np.array([mid]))[0] - (mid - iv[0]) / np.float64(F(0.7))) <= 1e-12


def test_tau_of_the_ramp_along_z_and_of_the_sparse_block(vpt):
    ramp = X.describe(medium(vpt, "ramp", trdepth=0.5), 1)
    for x, y in ((0.31, 0.77), (0.5, 0.5), (0.02, 0.97)):
        for o, d in (((x, y, 3.0), (0, 0, -1.0)), ((x, y, -2.0), (0, 0, 1.0))):
            assert abs(X.optical_depth(ramp, o, d)[1] - 1.0 * X.bbox_of(ramp[0])[2] / 0.5) <= 1e-12   # mean 1 over the box's side (1 in float32)
    sparse = X.describe(medium(vpt, "volgrid", trdepth=0.25), 1)
    for x, y in ((0.5, 0.5), (12.5 / 31, 18.9 / 31)):
        assert abs(X.optical_depth(sparse, (x, y, 3.0), (0, 0, -1.0))[1] - (8.0 / 31.0) * X.bbox_of(sparse[0])[2] / 0.25) <= 1e-12
    assert X.optical_depth(sparse, (0.1, 0.1, 3.0), (0, 0, -1.0))[1] == 0.0


def test_tau_agrees_with_itself_when_every_piece_is_halved(cases):
    for name, (instances, rays, taus) in cases.items():
        for (label, o, d), (tau, total) in zip(rays, taus):
            halved, total2 = X.optical_depth(instances, o, d, halve=True)
            t = np.linspace(0, tau.cuts()[-1] * 1.05, 257)
            assert np.abs(tau(t) - halved(t)).max() <= 1e-9 and abs(total - total2) <= 1e-9, (name, label)


@pytest.mark.parametrize("name", ["ramp", "sparse"])
def test_tau_agrees_with_a_midpoint_sum_of_the_host_mirror(vpt, name):
    """2^16 midpoints along an oblique chord.  The allowance: the lookup's float32 bound (test_volgrid_host.py) over the chord; the points
    are float32, each coordinate off the ray by <= 2 u |p| <= 4 u, which the steepest gradient (3 axes, D per cell, W - 1 cells per unit
    length of these unit boxes) turns into density; the midpoint rule's own error: h^2 / 24 times the second derivative inside a piece
    (<= 6 D (W - 1)^2: the mixed terms of a trilerp) and h^2 / 8 times the jump of the first derivative at a cut (<= 2 sqrt(3) D (W - 1))"""
    scene = SCENES[name][0](vpt)
    instances = X.describe(scene, 1)
    voxels, trdepth = instances[0]["voxels"], float(instances[0]["trdepth"])
    o, d = np.array([-0.3, 0.1, 0.05]), unit((1.0, 0.45, 0.55))
    t0, t1 = X.box_interval(instances[0], o, d)
    tau, total = X.optical_depth(instances, o, d)
    N = 1 << 16
    h = (t1 - t0) / N
    t = t0 + (np.arange(N) + 0.5) * h
    sigma, _ = scene.volgrid_density((o + d * t[:, None]).astype(F))
    got = float(sigma.astype(np.float64).sum() * h)
    D = max(np.abs(np.diff(voxels, axis=a)).max() for a in range(3))
    W = max(voxels.shape)
    lookup = density_bound(voxels.astype(F), trdepth) * (t1 - t0)
    position = 3 * D * (W - 1) / trdepth * 4 * U * (t1 - t0)
    midpoint = (h * h / 24 * 6 * D * (W - 1) ** 2 * (t1 - t0) + h * h / 8 * 2 * np.sqrt(3) * D * (W - 1) * len(tau.cuts())) / trdepth
    print(f"{name}: tau {total:.9f}, midpoint sum {got:.9f}, difference {abs(got - total):.3e}, allowed {lookup + position + midpoint:.3e}")
    assert total > 0.5 and abs(got - total) <= lookup + position + midpoint


# ---- the KS threshold: acceptance and power, on every test ray -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_every_ray_is_deep_enough_and_the_threshold_separates_a_medium_five_percent_denser(cases, name):
    worst_self, least_denser = 0.0, np.inf
    for si, (instances, rays, taus) in [(list(SCENES).index(name), cases[name])]:
        for ri, ((label, o, d), (tau, total)) in enumerate(zip(rays, taus)):
            assert total >= 0.5, f"{name} {label}: tau_total {total:.3f}: the test could not fail on this ray"
            target = -np.log1p(-np.random.default_rng(1000 * si + ri).uniform(0, 1, S))
            collided = target < total
            t = tau.invert(target[collided])
            assert np.abs(tau(t) - target[collided]).max() <= 1e-9
            own = X.ks_sqrt_n(t, S, tau.cdf)
            denser = X.ks_sqrt_n(t, S, lambda x: tau.cdf(x, 1.05))
            worst_self, least_denser = max(worst_self, own), min(least_denser, denser)
            assert own <= KS_LIMIT and denser > KS_LIMIT, f"{name} {label}: tau {total:.3f}, self {own:.3f}, 5 % denser {denser:.3f}"
    print(f"{name}: sqrt(S) D over its rays: self against self at most {worst_self:.3f}, 5 % denser at least {least_denser:.3f}")


def test_the_superposed_tau_is_the_sum_and_the_shares_add_up(cases):
    instances, rays, taus = cases["overlap"]
    for (label, o, d), (tau, total) in zip(rays, taus):
        a, b = X.optical_depth(instances, o, d, only=0), X.optical_depth(instances, o, d, only=1)
        assert abs(a[1] + b[1] - total) <= 1e-12
        assert abs(tau.share(0) + tau.share(1) - 1) <= 1e-10, label
    # one homogeneous box alone and two of them overlapping fully: shares by sigma
    same = [X.grid_instance(np.ones((9, 9, 9)), 1 / 9, [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], 1.0, td) for td in (2.0, 0.5)]
    tau, _ = X.optical_depth(same, (0.4, 0.6, 3.0), (0, 0, -1.0))
    assert abs(tau.share(0) - 0.2) <= 1e-12 and abs(tau.share(1) - 0.8) <= 1e-12


# ---- PCG32 -------------------------------------------------------------------------------------------------------------------------------------
def test_pcg32_in_numpy_draws_the_known_first_floats(vpt, scene03):
    """the first floats of pixels 0 and 1 of make_state at 1280 (test_host_pipeline.py: measured on the reference)"""
    rng = scene03.make_state(vpt.PathtraceParams(resolution=1280)).rngs.reshape(-1, 2)[:2]
    rng, a = X.rand1f(rng)
    rng2, b = X.rand1f(rng)
    assert [float(a[0]), float(b[0])] == [float.fromhex("0x1.25745p-3"), float.fromhex("0x1.9893ep-1")]
    assert [float(a[1]), float(b[1])] == [float.fromhex("0x1.1d3f4p-1"), float.fromhex("0x1.b88944p-1")]
    assert np.array_equal(X.rng_skip(rng, 1), rng2) and np.array_equal(rng[:, 1], rng2[:, 1])


# ---- the path tracer on its own ----------------------------------------------------------------------------------------------------------------
def region(resolution=48, camera=CAM_BOX, lo=0.25, hi=0.75):
    """the pixels of a frame whose whole footprint lies in x, y in [lo, hi] ((h, w) bool), and the rectangle they cover (x0, x1, y0, y1)"""
    (ra, rb), (ca, cb) = spans(camera, resolution, True), spans(camera, resolution, False)
    rows, cols = (ra >= lo) & (rb <= hi), (ca >= lo) & (cb <= hi)
    return np.outer(rows, cols), (ca[cols].min(), cb[cols].max(), ra[rows].min(), rb[rows].max())


UNIT_BOX = ((0, 0, 0), (1, 1, 1))


def two_slabs(g):
    """the direction-of-scattering case: a white slab of optical depth 1 over a black emitter of optical depth 4, under a black sky"""
    return [X.box_medium(*UNIT_BOX, 1.0, 1.0, g), X.box_medium((0, 0, -1.5), (1, 1, -0.5), 4.0, 0.0, 0.0, EMISSION)]


def coloured(bounces):
    """the colour / roulette / truncation case: (boxes, environment, bounces)"""
    return [X.box_medium(*UNIT_BOX, 2.0, (0.9, 0.5, 0.2), 0.6, (0.0, 0.1, 0.0))], 0.5, bounces


def test_the_henyey_greenstein_cosine_has_mean_g_and_the_right_density():
    xi = (np.arange(1 << 20) + 0.5) / (1 << 20)
    for g in (0.6, -0.6, 0.0, 0.9):
        c = X.hg_cosine(g, xi)
        assert abs(c.mean() - g) <= 1e-6 and c.min() >= -1 and c.max() <= 1
        # the distribution function of the cosine at 0: the integral of (1 - g^2) / (2 (1 + g^2 - 2 g c)^1.5) over c in [-1, 0]
        want = 0.5 if g == 0 else (1 - g * g) / (2 * g) * (1 / np.sqrt(1 + g * g) - 1 / (1 + g))
        assert abs((c < 0).mean() - want) <= 2e-6


def test_reference_paths_white_furnace_is_exactly_the_environment():
    _, rect = region()
    rad, hit = X.reference_paths([X.box_medium(*UNIT_BOX, 1.0, 1.0, 0.6)], 0.5, 4096, 20000, 5, rect)
    assert np.all(rad == 0.5) and 0 < hit.mean() < 1


def test_reference_paths_black_medium_is_beer_lambert():
    _, rect = region()
    rad, hit = X.reference_paths([X.box_medium(*UNIT_BOX, 1.7, 0.0, 0.0)], 0.5, 8, 1 << 19, 6, rect)
    mean, se = X.mean_and_se(rad)
    assert np.all(np.abs(mean - 0.5 * np.exp(-1.7)) <= 5 * se) and np.all(se < 1e-3)
    assert abs(hit.mean() - (1 - np.exp(-1.7))) <= 5 * np.sqrt(0.25 / len(hit))


def test_reference_paths_one_bounce_with_emission_is_the_closed_form():
    _, rect = region()
    boxes, env, _ = coloured(1)
    rad, _ = X.reference_paths(boxes, env, 1, 1 << 19, 7, rect)
    mean, se = X.mean_and_se(rad)
    T = np.exp(-2.0)
    want = 0.5 * T + np.array([0.0, 0.1, 0.0]) * (1 - T)
    print("one bounce:", mean, want, se)
    assert np.all(np.abs(mean - want) <= 5 * se)
    rad0, hit0 = X.reference_paths(boxes, env, 0, 1000, 7, rect)
    assert np.all(rad0 == 0) and np.all(hit0 == 0)


def test_reference_paths_tell_forward_from_backward_scattering():
    """the two slabs, g = +0.6 against -0.6: a kernel that scatters the wrong way round is > 20 combined standard errors off"""
    _, rect = region()
    (fm, fs), (bm, bs) = [X.mean_and_se(X.reference_paths(two_slabs(g), 0.0, 8, 1 << 19, 11, rect)[0]) for g in (0.6, -0.6)]
    z = (fm - bm) / np.sqrt(fs ** 2 + bs ** 2)
    print(f"green: forward {fm[1]:.4f} +- {fs[1]:.1e}, backward {bm[1]:.4f} +- {bs[1]:.1e}, z {z}")
    assert np.all(z > 20)
    assert np.allclose(fm / fm[1], np.array(EMISSION), rtol=0, atol=1e-12)   # one emitter, a white slab: the channels are its colour


def test_the_package_exports_the_probe(vpt):
    assert callable(vpt.DeviceScene.volgrid_track) and hasattr(vpt.hip, "vpt_scene_volgrid_track")
