"""The first-collision pass of the volgrid shader on the GPU (include/vpt.h: vpt_render_volgrid_aov_device) and the
session's pick over it.  Exact: the pass against the free-flight probe on the pixel-centre rays, against K3's alpha, against itself in
other batches, against the host rule's normal, device planes against host arrays, the session's pick against its id frame and against
a sculpt made by hand.  Statistical, with deterministic streams: opacity and mean collision distance of the `constant` slab against
their closed forms (test_volgrid_aov_host.py shows the same check passing on the reference distribution and rejecting a medium 5 % denser).
Frames are 32 x 32 to 48 x 48."""
import numpy as np
import pytest

import volgrid_exact as X
from test_volgrid_aov_host import PIXELS, SAMPLES, SLAB, slab_passes, slab_scores
from test_volgrid_exact_host import scene_rotated
from test_volgrid_gpu import CAM_BOX, interior, medium, need_gpu, params_of, render, sphere_stamp, walk  # noqa: F401 (walk: a fixture)
from test_volgrid_host import F, load

pytestmark = pytest.mark.gpu

ALL = ("opacity", "albedo", "depth", "normal", "ids", "hit")
KAT_CAMERA = 3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def aov_pass(host, dev, params, batches, planes=ALL):
    """the pass over a fresh make_state in the given batches: ({name: (n, k) array}, state)"""
    st, out = host.make_state(params), None
    for n in batches:
        out = dev.render_volgrid_aovs(st, params, n, planes, into=out)
    return {k: a.reshape(st.width * st.height, -1) for k, a in out.items()}, st


def centre_rays(dev, camera, w, h):
    rec = np.zeros((h, w, 5), F)
    rec[..., 0] = camera
    rec[..., 1] = ((np.arange(w, dtype=F) + F(0.5)) / F(w))[None, :]
    rec[..., 2] = ((np.arange(h, dtype=F) + F(0.5)) / F(h))[:, None]
    return dev.kat(KAT_CAMERA, rec.reshape(-1, 5))   # eval_camera on the device


def centre_flights(host, dev, params):
    """the probe on the pixel-centre rays with the streams the pass flies them with (two lens draws in): (rays, event, instance, t, rng_out)"""
    st = host.make_state(params)
    rays = centre_rays(dev, params.camera, st.width, st.height)[:, :6].astype(F)
    event, instance, t, _, rng_out = dev.volgrid_track(rays, X.rng_skip(st.rngs.reshape(-1, 2), 2))
    return rays, event, instance, t, rng_out


# ---- exact ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["constant", "volgrid", "overlap"])
def test_a_one_sample_pass_is_the_probe_on_the_pixel_centre_rays(vpt, walk, name):
    need_gpu(vpt)
    host = load(vpt, name)
    dev = vpt.DeviceScene(host, 0)
    p = params_of(vpt, 32, 1)
    rays, event, instance, t, rng_out = centre_flights(host, dev, p)
    got, st = aov_pass(host, dev, p, [1])
    hit = event == 1
    assert 0 < hit.sum() < hit.size and np.all(event < 2)            # collisions (few on the thin block of `volgrid`), and rays past every box
    volume = np.array([host.volume_instance(int(g)).volume if g >= 0 else -1 for g in instance])
    assert np.array_equal(got["ids"], np.stack([np.where(hit, instance, -1), volume], axis=1))
    tt = np.where(hit, t, 0).astype(F)
    position = np.where(hit[:, None], rays[:, :3] + (rays[:, 3:] * tt[:, None]).astype(F), 0).astype(F)   # the product, then the sum
    assert np.array_equal(bits(got["hit"]), bits(np.concatenate([position, tt[:, None]], axis=1)))
    assert np.array_equal(got["opacity"], np.repeat(hit.astype(F)[:, None], 4, axis=1))
    assert np.array_equal(bits(got["depth"]), bits(np.stack([tt, 0 * tt, 0 * tt, hit.astype(F)], axis=1)))
    assert np.array_equal(st.rngs.reshape(-1, 2), rng_out) and np.all(st.hits == 1) and st.samples == 1


@pytest.mark.parametrize("bounces", [1, 8])
def test_opacity_is_the_alpha_k3_adds_from_equal_state(vpt, walk, bounces):
    need_gpu(vpt)
    host = load(vpt, "overlap")
    dev = vpt.DeviceScene(host, 0)
    p = params_of(vpt, 40, 4, bounces)
    got, _ = aov_pass(host, dev, p, [1], ("opacity",))
    alpha = render(vpt, host, dev, p, 1).image.reshape(-1, 4)[:, 3]
    assert 0 < alpha.sum() < alpha.size and np.array_equal(got["opacity"][:, 3], alpha)


@pytest.mark.parametrize("name", ["overlap", "messy"])
def test_batching_changes_no_bit_of_any_plane(vpt, walk, name):
    need_gpu(vpt)
    host = load(vpt, name)
    dev = vpt.DeviceScene(host, 0)
    p = params_of(vpt, 40, 8)
    (a, sa), (b, sb) = aov_pass(host, dev, p, [3, 5]), aov_pass(host, dev, p, [8])
    for n in ALL:
        assert np.array_equal(bits(a[n]), bits(b[n])), n
    assert np.array_equal(sa.rngs, sb.rngs) and np.all(sa.hits == 8) and np.array_equal(sa.hits, sb.hits)
    first = aov_pass(host, dev, p, [1], ("ids",))[0]["ids"][:, 0]
    later = (first < 0) & (a["ids"][:, 0] >= 0)
    assert later.sum() > 0 and np.all(a["ids"][first >= 0, 0] == first[first >= 0])   # the first collision stays; a later flight fills a gap
    assert np.array_equal(a["ids"][:, 0] >= 0, a["opacity"][:, 3] > 0)


def test_albedo_is_opacity_times_the_records_albedo(vpt, walk):
    need_gpu(vpt)
    host = medium(vpt, "volgrid", albedo=0.75)      # multiples of 0.75 are exact: the sums carry no rounding
    got, _ = aov_pass(host, vpt.DeviceScene(host, 0), params_of(vpt, 32, 8), [8], ("opacity", "albedo"))
    want = got["opacity"] * np.array([0.75, 0.75, 0.75, 1], F)
    assert got["opacity"].max() >= 4 and np.array_equal(bits(got["albedo"]), bits(want))


def test_an_empty_medium_gives_zeros_and_draws_only_the_camera(vpt, walk):
    need_gpu(vpt)
    host = load(vpt, "volgrid")
    host.set_volume(0, np.zeros((32, 32, 32), F))
    host.update_volumes()
    p = params_of(vpt, 32, 4)
    got, st = aov_pass(host, vpt.DeviceScene(host, 0), p, [3])
    assert all(np.all(got[n] == 0) for n in ALL if n != "ids") and np.all(got["ids"] == -1)
    assert np.array_equal(st.rngs.reshape(-1, 2), X.rng_skip(host.make_state(p).rngs.reshape(-1, 2), 12)) and np.all(st.hits == 3)   # u, v, lens x 3


@pytest.mark.parametrize("name", ["ramp", "rotated"])
def test_the_normal_plane_is_the_host_rules_normal_at_the_reported_position(vpt, walk, name):
    need_gpu(vpt)
    host = scene_rotated(vpt) if name == "rotated" else load(vpt, name)
    got, _ = aov_pass(host, vpt.DeviceScene(host, 0), params_of(vpt, 32, 1), [1], ("normal", "ids", "hit"))
    hit = got["ids"][:, 0] == 0
    _, n, inside = host.volgrid_gradient(0, got["hit"][hit, :3])
    assert hit.sum() > 50 and inside.all() and np.abs(n).max() > 0.5
    want = np.zeros((hit.size, 4), F)
    want[hit] = np.concatenate([n * F(0.5) + F(0.5), np.ones((hit.sum(), 1), F)], axis=1)
    assert np.array_equal(bits(got["normal"]), bits(want))
    # the session's pick packs the same normal on the device, and pathtrace_volgrid_aovs resolves the same sums
    s = vpt.RenderSession(vpt.DeviceScene(host, 0), params_of(vpt, 32, 4, 4), pratio=4, guide_samples=1)
    k = int(np.flatnonzero(hit)[len(n) // 2])
    assert np.array_equal(bits(s.pick_volgrid(k % 32, k // 32)["normal"]), bits(n[len(n) // 2]))
    mean = vpt.pathtrace_volgrid_aovs(host, vpt.DeviceScene(host, 0), params_of(vpt, 32, 1), 1, ("normal", "depth"))
    assert np.array_equal(bits(mean["normal"].reshape(-1, 4)), bits(want)) and np.array_equal(mean["depth"].reshape(-1, 4)[:, 0], got["hit"][:, 3])


def test_device_planes_agree_with_the_host_arrays_after_resolve(vpt, walk):
    need_gpu(vpt)
    import torch
    host = load(vpt, "overlap")
    dev = vpt.DeviceScene(host, 0)
    p = params_of(vpt, 44, 4)                            # 44 x 44: tiles with padding slots
    want, st = aov_pass(host, dev, p, [2])
    lay, n = vpt.VptLayout(st.width, st.height, 8, 8, 0, 1), st.width * st.height
    slots = vpt.layout_slots(lay)
    hits, rng = torch.zeros(slots, dtype=torch.int32, device="cuda"), torch.zeros((slots, 2), dtype=torch.int64, device="cuda")
    image = torch.zeros((slots, 4), device="cuda")
    vpt.state_init_device(lay, image.data_ptr(), hits.data_ptr(), rng.data_ptr())
    tiles = {k: torch.zeros((slots, 2 if k == "ids" else 4), dtype=torch.int32 if k == "ids" else torch.float32, device="cuda") for k in ALL}
    dev.render_volgrid_aov_device(p, lay, 2, {k: t.data_ptr() for k, t in tiles.items()}, hits.data_ptr(), rng.data_ptr())
    rows = {k: torch.zeros((n, 2 if k == "ids" else 4), dtype=tiles[k].dtype, device="cuda") for k in ALL}
    for k in ("opacity", "albedo", "depth", "normal"):
        vpt.resolve_device(lay, tiles[k].data_ptr(), 1, rows[k].data_ptr())
    vpt.resolve_volgrid_ids_device(lay, tiles["ids"].data_ptr(), tiles["hit"].data_ptr(), rows["ids"].data_ptr(), rows["hit"].data_ptr())
    torch.cuda.synchronize()
    for k in ALL:
        assert np.array_equal(bits(rows[k].cpu().numpy()), bits(want[k])), k
    assert want["ids"].max() == 1 and (want["ids"][:, 0] == -1).any()


def test_a_medium_without_trdepth_is_refused_as_a_render_refuses_it(vpt):
    need_gpu(vpt)
    host = medium(vpt, "constant", trdepth=0.0)
    with pytest.raises(vpt.VptError, match=r"\(-1\).*vol_instance 0"):
        aov_pass(host, vpt.DeviceScene(host, 0), params_of(vpt, 32, 2), [1])


# ---- the session ------------------------------------------------------------------------------------------------------------------------------
def test_session_pick_follows_the_id_frame_edits_and_the_other_families_stay_refused(vpt):
    need_gpu(vpt)
    host = medium(vpt, "constant", trdepth=0.1)          # optical depth 10: every flight through the box collides
    dev = vpt.DeviceScene(host, 0)
    s = vpt.RenderSession(dev, params_of(vpt, 32, 4, 4), pratio=4, guide_samples=4)
    ids, hit = s.volgrid_ids()
    _, event, instance, t, _ = centre_flights(host, dev, params_of(vpt, 32, 1))
    assert np.array_equal(ids[..., 0].reshape(-1)[event == 1], instance[event == 1]) and np.array_equal(hit[..., 3].reshape(-1)[event == 1], t[event == 1])
    inside, moved_out, outside = (16, 24), (16, 8), (2, 2)   # (y, x): world x 0.79, 0.21 and a corner past the box
    for (y, x) in (inside, moved_out, outside):
        pick = s.pick_volgrid(x, y)
        assert s.stats()[2] == 48                              # the 48 bytes of the record, nothing else
        if ids[y, x, 0] < 0:
            assert pick is None and (y, x) == outside
            continue
        assert (pick["vol_instance"], pick["volume"], pick["material"]) == (0, 0, 0) and pick["distance"] == hit[y, x, 3]
        assert np.array_equal(pick["position"], hit[y, x, :3]) and np.all(pick["normal"] == 0)   # a constant grid has no gradient
        assert pick["density"] == host.volgrid_density(hit[y, x, :3][None])[0][0]
    for call in (lambda: s.pick(3, 3), lambda: s.pick_sdf(3, 3), lambda: s.ids(), lambda: s.sdf_ids()):
        with pytest.raises(vpt.VptError, match=r"\(-5\)"):
            call()
    host.set_volume_instance(0, frame=[1, 0, 0, 0, 1, 0, 0, 0, 1, -0.5, 0, 0])   # the box moves to x in [0.5, 1.5]
    s.edit_volumes(host.update_volumes())
    assert s.pick_volgrid(moved_out[1], moved_out[0]) is None and s.pick_volgrid(inside[1], inside[0]) is not None
    other = vpt.RenderSession(dev, vpt.PathtraceParams(resolution=32, shader="implicit", samples=2, bounces=2), pratio=4)
    for call in (lambda: other.pick_volgrid(3, 3), lambda: other.volgrid_ids()):
        with pytest.raises(vpt.VptError, match=r"\(-5\)"):
            call()


def test_sculpt_at_on_a_volgrid_session_is_the_hand_made_sculpt_of_its_entry(vpt):
    need_gpu(vpt)
    host, twin = (medium(vpt, "volgrid", trdepth=0.1) for _ in range(2))
    dev, dev_twin = vpt.DeviceScene(host, 0), vpt.DeviceScene(twin, 0)
    s = vpt.RenderSession(dev, params_of(vpt, 32, 4, 4), pratio=4)
    assert s.pick_volgrid(16, 16) is not None
    entry = s.sculpt_at(host, 16, 16, sphere_stamp(vpt, (0, 0, 0), 0.08).brush, vpt.SCULPT_REPLACE)
    assert entry.volume == 0 and all(0 < n < 32 for n in entry.region_whd) and s.samples == 0
    twin.sculpt_volume(0, entry.stamps, region=(entry.region_lo, entry.region_whd))
    dev_twin.sculpt_volumes(twin.update_sculpts())
    assert np.array_equal(bits(dev.get_voxels(0)), bits(dev_twin.get_voxels(0))) and np.array_equal(bits(host.volume(0)[0]), bits(twin.volume(0)[0]))
    assert not np.array_equal(bits(dev.get_voxels(0)), bits(load(vpt, "volgrid").volume(0)[0]))


# ---- statistical, with deterministic streams --------------------------------------------------------------------------------------------------
def test_opacity_and_mean_depth_of_a_slab_follow_their_closed_forms(vpt, walk):
    """Measured on an MI355X (either walk: `constant` has one brick): opacity max |z| 3.15, mean -0.041; depth max |z| 3.19, mean +0.039 (limit 0.357)"""
    need_gpu(vpt)
    host = load(vpt, "constant")
    p = params_of(vpt, 48, SAMPLES)
    got, _ = aov_pass(host, vpt.DeviceScene(host, 0), p, [SAMPLES], ("opacity", "depth"))
    keep = interior(CAM_BOX, 48, 0.25, 0.75).reshape(-1)
    assert keep.sum() == PIXELS
    assert np.array_equal(got["opacity"][keep, 3], got["depth"][keep, 3])
    z_o, z_d = slab_scores(got["opacity"][keep, 3].astype(np.float64), got["depth"][keep, 0].astype(np.float64), SAMPLES, **SLAB)
    print(f"opacity: max |z| {np.abs(z_o).max():.2f}, mean {z_o.mean():+.3f}; depth: max |z| {np.abs(z_d).max():.2f}, mean {z_d.mean():+.3f}; "
          f"limit on a mean {5 / np.sqrt(PIXELS):.3f}")
    assert slab_passes(z_o) and slab_passes(z_d)
