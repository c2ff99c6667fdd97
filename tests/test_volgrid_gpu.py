"""The volgrid shader on the GPU (include/vpt.h: VPT_SHADER_VOLGRID; K3, csrc/vpt_volgrid_kernel.hip.h): voxel grids rendered as
heterogeneous media by delta tracking over brick majorants.  The reference has no such shader, so the yardsticks are closed forms -
several exact to the last bit by construction (an empty medium, white furnaces), the rest statistical with deterministic streams
(Beer-Lambert transmittance of known optical depths) - and the project's bitwise invariants (batching, session, layout, adaptive,
edit-then-render = fresh-then-render).  state.hits counts samples, as in every shader here; the alpha channel sums a sample's `hit`.

Frames are 32 x 32 to 64 x 64.  "Interior pixels" lie at least two pixels inside a silhouette."""
import ctypes as C

import numpy as np
import pytest

from test_volgrid_host import F, load, numpy_majorants

pytestmark = pytest.mark.gpu

CAM_BOX, CAM_CENTRE = 0, 1                   # make_volgrid_scene.py: the box with a margin (1.25 wide), zoomed on its centre (0.25 wide)
EXTENT = {CAM_BOX: 1.25, CAM_CENTRE: 0.25}   # both centred on (0.5, 0.5), looking down -z


def need_gpu(vpt):
    if vpt.device_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible (the HIP path has no CPU fallback)")


def medium(vpt, name, material=0, albedo=None, g=None, trdepth=None, emission=None):
    """the fixture scene `name` with fields of one material replaced"""
    scene = load(vpt, name)
    m = scene.material(material)
    if albedo is not None:
        m.scattering[:] = [float(albedo)] * 3
    if g is not None:
        m.scanisotropy = float(g)
    if trdepth is not None:
        m.trdepth = float(trdepth)
    if emission is not None:
        m.emission[:] = [float(e) for e in emission]
    scene.set_material(material, m)
    scene.update_bvh()   # hands the pending edit out: the descriptor carries the material
    return scene


def params_of(vpt, resolution=64, samples=64, bounces=8, camera=CAM_BOX, mis=True):
    return vpt.PathtraceParams(camera=camera, resolution=resolution, shader="volgrid", samples=samples, bounces=bounces, noimplicit_mis=not mis)


def render(vpt, scene, dev, params, n=None):
    st = scene.make_state(params)
    dev.pathtrace_samples(st, params, params.samples if n is None else n)
    return st


def same_state(a, b):
    return (a.samples == b.samples and np.array_equal(a.image.view(np.uint32), b.image.view(np.uint32)) and np.array_equal(a.hits, b.hits)
            and np.array_equal(a.rngs, b.rngs))


def spans(camera, resolution, mirrored):
    """the world interval each pixel column (mirrored: each row) covers, jitter included: pixel k of a column spans
    0.5 + ((k .. k + 1) / resolution - 0.5) * extent along x; rows run down while y runs up, so a row spans the interval mirrored at 0.5"""
    edges = 0.5 + (np.arange(resolution + 1) / resolution - 0.5) * EXTENT[camera]
    a, b = edges[:-1], edges[1:]
    return (1 - b, 1 - a) if mirrored else (a, b)


def inside_1d(camera, resolution, lo, hi, margin, mirrored):
    a, b = spans(camera, resolution, mirrored)
    k = np.flatnonzero((a >= lo) & (b <= hi))
    keep = np.zeros(resolution, bool)
    keep[k.min() + margin:k.max() + 1 - margin] = True
    return keep


def interior(camera, resolution, lo, hi, margin=2):
    """the pixels whose whole footprint lies inside the square silhouette [lo, hi]^2, at least `margin` pixels inside: (h, w) bool"""
    return np.outer(inside_1d(camera, resolution, lo, hi, margin, True), inside_1d(camera, resolution, lo, hi, margin, False))


def exterior(camera, resolution, lo, hi):
    """the pixels whose footprint does not touch [lo, hi]^2"""
    (ra, rb), (ca, cb) = spans(camera, resolution, True), spans(camera, resolution, False)
    return ((rb < lo) | (ra > hi))[:, None] | ((cb < lo) | (ca > hi))[None, :]


@pytest.fixture(params=[False, True], ids=["bricks", "one_majorant"])
def walk(request, monkeypatch):
    """the brick walk, and the same rule behind VPT_VOLGRID_NO_BRICKS=1: one majorant per volume"""
    if request.param:
        monkeypatch.setenv("VPT_VOLGRID_NO_BRICKS", "1")
    else:
        monkeypatch.delenv("VPT_VOLGRID_NO_BRICKS", raising=False)
    return request.param


# ---- 5. tables and lookups against the host mirror, fresh and stale -------------------------------------------------------------------------
def sphere_stamp(vpt, centre, radius):
    f = vpt.VptSdf(type=vpt.SDF_TYPES.index("sphere"), material=0)
    f.frame.x[:], f.frame.y[:], f.frame.z[:] = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    f.frame.o[:] = [-float(c) for c in centre]
    f.p[:] = (float(radius), 0, 0, 0)
    return vpt.Stamp(f, 0, 0.0)   # SCULPT_REPLACE


def points_for(seed=5, n=4096):
    g = np.random.default_rng(seed)
    p = g.uniform(-0.25, 1.25, (n, 3)).astype(F)
    p[: n // 4] = g.uniform(0.2, 0.7, (n // 4, 3)).astype(F)
    return p


def assert_tables_equal(host, dev, volumes):
    for v in volumes:
        got, want = dev.volgrid_majorants(v), host.volgrid_majorants(v)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"majorants of volume {v}"
    pts = points_for()
    (gs, gi), (ws, wi) = dev.volgrid_density(pts), host.volgrid_density(pts)
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)) and np.array_equal(gi, wi)
    return gs


def test_device_majorants_and_densities_equal_the_host_mirror_and_follow_edits(vpt):
    need_gpu(vpt)
    host = load(vpt, "messy")
    dev = vpt.DeviceScene(host, 0)
    assert dev.volgrid_stats()["table_builds"] == 0            # a scene that never renders volgrid never builds the tables
    before = assert_tables_equal(host, dev, (0, 1))
    assert np.count_nonzero(before) > 200 and dev.volgrid_stats()["table_builds"] == 1
    render(vpt, host, dev, params_of(vpt, 32, 2))
    assert dev.volgrid_stats()["table_builds"] == 1            # nothing changed: nothing is rebuilt
    # a stroke on the resident sparse grid (volume 1): distances of a sphere written over a box of its voxels
    host.sculpt_volume(1, [sphere_stamp(vpt, (0.3, 0.3, 0.3), 0.1)], region=((4, 4, 4), (12, 12, 12)))
    dev.sculpt_volumes(host.update_sculpts())
    after = assert_tables_equal(host, dev, (0, 1))
    assert dev.volgrid_stats()["table_builds"] == 2 and not np.array_equal(before, after)
    assert np.array_equal(host.volgrid_majorants(1), numpy_majorants(host.volume(1)[0]))
    # a set_volume on the resident scene: the messy grid replaced by one of another size (its table moves and changes shape)
    voxels = np.random.default_rng(3).uniform(-0.5, 1.5, (11, 26, 19)).astype(F)
    host.set_volume(0, voxels, res=1.0 / 26)
    dev.update_volumes(host.update_volumes())
    assert_tables_equal(host, dev, (0, 1))
    assert dev.volgrid_majorants(0).shape == (2, 4, 3) and dev.volgrid_stats()["table_builds"] == 3


# ---- 6. - 8. exact renders -----------------------------------------------------------------------------------------------------------------
def test_an_empty_medium_renders_the_environment_exactly(vpt, walk):
    need_gpu(vpt)
    host = load(vpt, "volgrid")
    host.set_volume(0, np.zeros((32, 32, 32), F))
    host.update_volumes()
    p = params_of(vpt, 64, 64, 8)
    st = render(vpt, host, vpt.DeviceScene(host, 0), p)
    assert np.all(st.image[..., :3] == F(64 * 0.5))
    assert np.all(st.image[..., 3] == 0)        # no sample hit the medium
    assert np.all(st.hits == 64) and st.samples == 64


def test_white_furnace_with_phase_sampling_is_exact(vpt, walk):
    """albedo 1, g = 0.6, no MIS, on the sparse grid with trdepth 1: the optical side length is <= 1, so a path escapes after any
    collision with probability >= exp(-sqrt(3)) and none of 64 x 64 x 64 is truncated at 1024 bounces; every weight stays 1"""
    need_gpu(vpt)
    host = medium(vpt, "volgrid", albedo=1.0, g=0.6, trdepth=1.0)
    st = render(vpt, host, vpt.DeviceScene(host, 0), params_of(vpt, 64, 64, 1024, mis=False))
    assert np.all(st.image[..., :3] == F(32.0))
    assert st.image[..., 3].max() > 0           # the medium was there: some first flights collided


def test_white_furnace_with_the_environment_in_the_light_list_is_exact(vpt, walk):
    """g = 0, MIS on: the weight is f / (0.5 f + 0.5 f) with f = 1 / (4 pi) on both sides - exactly 1 in float32"""
    need_gpu(vpt)
    host = medium(vpt, "volgrid", albedo=1.0, g=0.0, trdepth=1.0)
    assert len(host.lights()[0]) == 1           # the grey environment is in the light list
    st = render(vpt, host, vpt.DeviceScene(host, 0), params_of(vpt, 64, 64, 1024, mis=True))
    assert np.all(st.image[..., :3] == F(32.0))
    assert st.image[..., 3].max() > 0


# ---- 9. bitwise invariants on a scattering medium ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scattering(vpt):
    need_gpu(vpt)
    host = medium(vpt, "volgrid", albedo=0.8, g=0.6, trdepth=0.25)
    return host, vpt.DeviceScene(host, 0)


def test_eight_samples_in_one_call_equal_three_plus_five(vpt, scattering):
    host, dev = scattering
    p = params_of(vpt, 48, 8, 8)
    whole = render(vpt, host, dev, p, 8)
    parts = host.make_state(p)
    dev.pathtrace_samples(parts, p, 3)
    dev.pathtrace_samples(parts, p, 5)
    assert same_state(whole, parts)
    assert len(np.unique(whole.image[..., 0])) > 100   # a picture, not a constant


def test_a_session_equals_make_state_and_render(vpt, scattering):
    host, dev = scattering
    p = params_of(vpt, 48, 8, 8)
    s = vpt.RenderSession(dev, p, pratio=4)
    assert s.advance(3) == 3 and s.advance(5) == 8
    want = render(vpt, host, dev, p, 8)
    assert same_state(s.state(), want)
    assert np.array_equal(s.image().view(np.uint32), vpt.get_render(want).view(np.uint32))
    s.set_display(vpt.DisplayParams(1.0, True, True))
    assert s.display().shape[:2] == (want.height, want.width)


def test_two_virtual_ranks_equal_one(vpt, scattering):
    import torch
    host, dev = scattering
    p = params_of(vpt, 48, 1 << 20, 8)
    st = host.make_state(p)
    ref = st.copy()
    dev.pathtrace_samples(ref, p, 4)
    device = torch.device("cuda", 0)
    slots = vpt.layout_slots(vpt.VptLayout(st.width, st.height, 8, 8, 0, 2))
    back = st.copy()
    for r in range(2):
        lay = vpt.VptLayout(st.width, st.height, 8, 8, r, 2)
        img = torch.zeros((slots, 4), dtype=torch.float32, device=device)
        hit = torch.zeros((slots,), dtype=torch.int32, device=device)
        rng = torch.zeros((slots, 2), dtype=torch.int64, device=device)
        vpt.state_upload(lay, st, img.data_ptr(), hit.data_ptr(), rng.data_ptr())
        dev.render_device(p, lay, 4, img.data_ptr(), hit.data_ptr(), rng.data_ptr(), 0)
        torch.cuda.synchronize()
        vpt.state_download(lay, img.data_ptr(), hit.data_ptr(), rng.data_ptr(), back)   # this rank's pixels
    back.samples = 4
    assert same_state(back, ref)


def test_adaptive_equals_a_uniform_render_of_each_pixels_own_count(vpt, scattering):
    host, dev = scattering
    p = params_of(vpt, 48, 64, 8)
    st = host.make_state(p)
    rounds, taken = dev.pathtrace_adaptive(st, p, 0.05, min_samples=8, step=8)
    counts = np.unique(st.hits)
    assert len(counts) > 1 and counts.min() >= 8 and counts.max() <= 64 and taken == int(st.hits.sum())
    uniform = host.make_state(p)
    for n in range(8, 65, 8):
        dev.pathtrace_samples(uniform, p, 8)
        at = st.hits == n
        assert np.array_equal(st.image[at].view(np.uint32), uniform.image[at].view(np.uint32)) and np.array_equal(st.rngs[at], uniform.rngs[at])


def test_a_render_after_resident_edits_equals_a_fresh_scene(vpt):
    need_gpu(vpt)
    host = medium(vpt, "volgrid", albedo=0.8, g=0.6, trdepth=0.25)
    p = params_of(vpt, 48, 8, 8)
    A = vpt.DeviceScene(host, 0)
    first = render(vpt, host, A, p)            # the tables exist: every edit below has to make them stale
    host.sculpt_volume(0, [sphere_stamp(vpt, (0.3, 0.6, 0.5), 0.12)], region=((3, 10, 8), (14, 16, 16)))
    A.sculpt_volumes(host.update_sculpts())
    second = render(vpt, host, A, p)
    host.set_volume_instance(0, frame=[1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1, -0.05, 0.0], scalef=0.9)
    A.update_volumes(host.update_volumes())
    m = host.material(0)
    m.trdepth = 0.4
    host.set_material(0, m)
    A.update(host.update_bvh())
    third = render(vpt, host, A, p)
    assert same_state(third, render(vpt, host, vpt.DeviceScene(host, 0), p))
    assert not same_state(first, second) and not same_state(second, third)


def test_the_multi_device_path_renders_the_same_bits_and_follows_a_sculpt(vpt):
    """vpt_multi_render accepts the shader; the device's own handle builds its tables and makes them anew after an edit"""
    need_gpu(vpt)
    host = medium(vpt, "volgrid", albedo=0.8, g=0.6, trdepth=0.25)
    p = params_of(vpt, 48, 8, 8)
    multi, single = vpt.MultiDeviceScene(host, [0]), vpt.DeviceScene(host, 0)
    a = host.make_state(p)
    multi.pathtrace_samples(a, p, 8)
    assert same_state(a, render(vpt, host, single, p))
    host.sculpt_volume(0, [sphere_stamp(vpt, (0.3, 0.6, 0.5), 0.12)], region=((3, 10, 8), (14, 16, 16)))
    multi.sculpt_volumes(host.update_sculpts())
    b = host.make_state(p)
    multi.pathtrace_samples(b, p, 8)
    assert same_state(b, render(vpt, host, vpt.DeviceScene(host, 0), p)) and not same_state(a, b)


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_a_medium_without_trdepth_is_refused_and_the_state_stays(vpt):
    need_gpu(vpt)
    host = load(vpt, "volgrid")
    dev = vpt.DeviceScene(host, 0)
    p = params_of(vpt, 32, 4, 4)
    st = render(vpt, host, dev, p, 2)
    m = host.material(0)
    m.trdepth = 0.0
    host.set_material(0, m)
    dev.update(host.update_bvh())
    before = st.copy()
    with pytest.raises(vpt.VptError, match=r"\(-1\).*vol_instance 0"):
        dev.pathtrace_samples(st, p, 2)
    assert same_state(st, before)
    with pytest.raises(vpt.VptError, match=r"\(-1\).*vol_instance 0"):
        dev.volgrid_density(np.zeros((1, 3), F))
    implicit = vpt.PathtraceParams(resolution=32, shader="implicit", samples=2, bounces=2)
    render(vpt, host, dev, implicit)             # the other shaders do not care


def test_ids_nine_to_fifteen_stay_unknown(vpt, scattering):
    host, dev = scattering
    p = params_of(vpt, 32, 2, 2)
    st = host.make_state(p)
    for ident in range(9, 16):
        abi = p.to_abi()
        abi.shader = ident
        samples = C.c_int(0)
        rc = vpt.hip.vpt_render(dev.handle, C.byref(abi), 1, st.width, st.height, st.image.ctypes.data, st.hits.ctypes.data, st.rngs.ctypes.data,
                                C.byref(samples))
        assert rc == -4 and vpt.hip.vpt_last_error().decode() == "sampler unknown"


def test_a_volgrid_session_refuses_pick_ids_guides_and_the_denoised_display(vpt, scattering):
    host, dev = scattering
    p = params_of(vpt, 32, 4, 4)
    s = vpt.RenderSession(dev, p, pratio=4)
    s.advance(2)
    for call in (lambda: s.pick(3, 3), lambda: s.pick_sdf(3, 3), lambda: s.ids(), lambda: s.sdf_ids(), lambda: s.image(denoised=True)):
        with pytest.raises(vpt.VptError, match=r"\(-5\)"):
            call()
    with pytest.raises(vpt.VptError):
        s.guides()
    with pytest.raises(vpt.VptError, match=r"\(-5\)"):
        vpt.RenderSession(dev, p, pratio=4, denoise=True)
    assert s.advance(2) == 4 and same_state(s.state(), render(vpt, host, dev, p, 4))   # the refusals left the session as it was


def test_implicit_renders_keep_their_bits_around_a_volgrid_render(vpt):
    need_gpu(vpt)
    host = load(vpt, "messy")
    dev = vpt.DeviceScene(host, 0)
    shaders = [vpt.PathtraceParams(resolution=48, shader=s, samples=4, bounces=4) for s in ("implicit", "implicit_normal")]
    before = [render(vpt, host, dev, p) for p in shaders]
    render(vpt, host, dev, params_of(vpt, 48, 4, 4))
    after = [render(vpt, host, dev, p) for p in shaders]
    assert all(same_state(a, b) for a, b in zip(before, after))


# ---- 11. - 13. Beer-Lambert transmittance -----------------------------------------------------------------------------------------------------
N = 4096


def assert_transmittance(st, mask, T, what):
    """albedo 0 and N samples: a sample is worth 0.5 (it escaped) or 0.  Every pixel sum / 0.5 is an integer; every pixel of `mask` has
    its mean within 5 standard errors of 0.5 T, SE = 0.5 sqrt(T (1 - T) / N); the mean z-score over the M >= 100 pixels is within 5 / sqrt(M)"""
    counts = st.image[..., 0].astype(np.float64) / 0.5
    assert np.array_equal(counts, np.round(counts)) and np.array_equal(st.image[..., 0], st.image[..., 1]) and np.all(st.hits == N)
    M = int(mask.sum())
    assert M >= 100
    z = (counts[mask] / N - T) / np.sqrt(T * (1 - T) / N)     # the same z as (mean - 0.5 T) / SE
    print(f"{what}: T {T:.6f}, M {M}, max |z| {np.abs(z).max():.3f}, mean z {z.mean():+.4f} (allowed {5 / np.sqrt(M):.4f}), std z {z.std():.3f}")
    assert np.abs(z).max() <= 5
    assert abs(z.mean()) <= 5 / np.sqrt(M)
    # alpha counts the samples whose first flight collided: with albedo 0 all that did not escape
    assert np.array_equal(st.image[..., 3].astype(np.float64), N - counts)


def test_constant_density_of_optical_depth_ln_2(vpt, walk):
    need_gpu(vpt)
    host = medium(vpt, "constant", albedo=0.0, trdepth=1.0 / np.log(2.0))
    tau = 1.0 / float(host.material(0).trdepth)   # voxel value 1, a box of side 1, the float32 trdepth the device divides by
    st = render(vpt, host, vpt.DeviceScene(host, 0), params_of(vpt, 64, N, 8))
    assert_transmittance(st, interior(CAM_BOX, 64, 0.0, 1.0), np.exp(-tau), "constant")
    outside = exterior(CAM_BOX, 64, 0.0, 1.0)
    assert outside.sum() > 100 and np.all(st.image[outside][:, 0] == F(N * 0.5))   # rays past the box see the environment


def test_ramp_along_z_where_null_collisions_dominate(vpt, walk):
    need_gpu(vpt)
    host = medium(vpt, "ramp", albedo=0.0, trdepth=1.0)
    voxels, _ = host.volume(0)
    mean = float(voxels[:, 0, 0].astype(np.float64).mean())   # the trapezoid rule over equal cells of a linear ramp: its mean
    assert mean == 1.0 and voxels.max() == 2.0
    st = render(vpt, host, vpt.DeviceScene(host, 0), params_of(vpt, 64, N, 8))
    assert_transmittance(st, interior(CAM_BOX, 64, 0.0, 1.0), np.exp(-mean * 1.0 / 1.0), "ramp")


def test_sparse_grid_through_its_central_block(vpt, walk):
    need_gpu(vpt)
    host = medium(vpt, "volgrid", albedo=0.0, trdepth=0.25)
    voxels, _ = host.volume(0)
    column = voxels[:, 16, 16].astype(np.float64)
    depth = ((column[:-1] + column[1:]) / 2).sum() / 31.0     # the trapezoid rule over the node values: 31 cells along a side of 1
    assert abs(depth - 8.0 / 31.0) < 1e-12
    m = vpt.DeviceScene(host, 0)
    assert np.count_nonzero(host.volgrid_majorants(0)) == 8 and host.volgrid_majorants(0).size == 64   # nodes 12 .. 19 touch bricks 1 and 2 per axis: 56 of 64 bricks are empty
    st = render(vpt, host, m, params_of(vpt, 64, N, 8, camera=CAM_CENTRE))
    # the pixels over the block's interior, nodes 12 .. 19: there the column is the same whatever x and y
    assert_transmittance(st, interior(CAM_CENTRE, 64, 12.0 / 31.0, 19.0 / 31.0), np.exp(-depth / 0.25), "sparse")


def test_two_overlapping_instances_multiply_their_transmittances(vpt, walk):
    need_gpu(vpt)
    host = medium(vpt, "overlap", material=0, albedo=0.0)
    m = host.material(1)
    m.scattering[:] = (0.0, 0.0, 0.0)
    host.set_material(1, m)
    host.update_bvh()
    T = np.exp(-1.0 / float(host.material(0).trdepth)) * np.exp(-1.0 / float(host.material(1).trdepth))
    st = render(vpt, host, vpt.DeviceScene(host, 0), params_of(vpt, 64, N, 8))
    mask = interior(CAM_BOX, 64, 0.25, 1.0)                   # both boxes: x and y in [0.25, 1]
    assert_transmittance(st, mask, T, "overlap")


# ---- 14. furnaces with MIS, statistical -------------------------------------------------------------------------------------------------------
def assert_furnace(st, n, what):
    means = st.image[..., :3].astype(np.float64).mean(axis=2) / n
    M = means.size
    se = means.std(ddof=1) / np.sqrt(M)
    print(f"{what}: mean {means.mean():.6f}, SE {se:.2e} ({se / 0.5:.3%} of 0.5), z {(means.mean() - 0.5) / se:+.3f}")
    assert se <= 0.01 * 0.5          # or the test says nothing
    assert abs(means.mean() - 0.5) <= 5 * se


def test_furnace_with_mis_and_a_forward_phase_function(vpt):
    need_gpu(vpt)
    host = medium(vpt, "volgrid", albedo=1.0, g=0.6, trdepth=0.25)
    st = render(vpt, host, vpt.DeviceScene(host, 0), params_of(vpt, 32, 256, 256, mis=True))
    assert_furnace(st, 256, "constant environment")


def test_furnace_with_mis_and_a_textured_environment_of_one_colour(vpt):
    need_gpu(vpt)
    host = medium(vpt, "furnace_tex", albedo=1.0, g=0.6, trdepth=0.25)
    host.set_texture(0, np.ones((64, 128, 4), F), linear=True)
    host.set_environment(0, emission_tex=0)
    host.update_textures()
    lights, cdf = host.lights()
    assert len(lights) == 1 and lights[0]["cdf_len"] == 64 * 128    # a CDF light
    st = render(vpt, host, vpt.DeviceScene(host, 0), params_of(vpt, 32, 256, 256, mis=True))
    assert_furnace(st, 256, "textured environment")
