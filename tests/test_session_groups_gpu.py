"""The buffer groups of a session on the MI355X (csrc/vpt_session.hip: buffer_group, id_frame).  Every lazily made group
is keyed by the frame's pixels AND its tile-major slots.  Each case takes one session that has used a group at 105 x 40 to 100 x 42 -
4200 pixels both, 4480 slots against 4992 - and compares what the group then holds with a fresh session created at 100 x 42 on the
same scene, bit for bit.  The mesh id frame's own case is tests/test_aov_gpu.py's
test_id_frame_follows_a_frame_of_equal_pixels_and_more_slots."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, SCENE_03

pytestmark = pytest.mark.gpu

GRID = os.path.join(GOLDEN, "scenes", "06_gridsdf_synth", "gridsdf_synth.json")
A, B = (105, 40), (100, 42)
UNSUPPORTED = -5   # VPT_ERR_UNSUPPORTED


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


def scene_at_a(vpt, path):
    """(HostScene, DeviceScene) of its own - the case edits the camera - with the aspect of frame A"""
    if vpt.device_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible (the HIP path has no CPU fallback)")
    host = vpt.HostScene(path)
    dev = vpt.DeviceScene(host, 0)
    set_aspect(host, A, dev.update)
    return host, dev


def set_aspect(host, size, apply):
    cam = host.camera(0)
    cam.aspect = size[0] / size[1]
    host.set_camera(0, cam)
    apply(host.update_bvh())


def params(vpt, size, shader):
    return vpt.PathtraceParams(resolution=size[0], samples=4, shader=shader, bounces=2)


def session_at_a(vpt, dev, shader, **kw):
    s = vpt.RenderSession(dev, params(vpt, A, shader), pratio=4, **kw)
    assert s.size == A
    return s


def move_to_b(vpt, host, s, shader, **reset_kw):
    """the aspect through a camera edit (a reset to 105 x 44 that uses no lazily made group), the resolution through reset"""
    set_aspect(host, B, s.edit)
    assert s.size == (105, 44)
    s.reset(params=params(vpt, B, shader), **reset_kw)
    assert s.size == B
    assert [vpt.layout_slots(vpt.VptLayout(w, h, 8, 8, 0, 1)) for w, h in (A, B)] == [4480, 4992]


def fresh_at_b(vpt, dev, shader, **kw):
    s = vpt.RenderSession(dev, params(vpt, B, shader), pratio=4, **kw)
    assert s.size == B
    return s


def test_implicit_id_frame_follows_the_slots(vpt):
    host, dev = scene_at_a(vpt, GRID)
    s = session_at_a(vpt, dev, "implicit")
    s.sdf_ids()
    s.pick_sdf(50, 20)   # the id frame and its 48-byte record exist at the first size
    move_to_b(vpt, host, s, "implicit")
    ids, hit = s.sdf_ids()
    fresh = fresh_at_b(vpt, dev, "implicit")
    want_ids, want_hit = fresh.sdf_ids()
    fresh.close()
    assert same(ids, want_ids) and same(hit, want_hit)
    assert (ids.max(axis=-1) >= 0).any() and (ids.max(axis=-1) < 0).any()
    for x, y in ((0, 0), (99, 41), (50, 40)):   # the last tile row of the larger layout among them
        p = s.pick_sdf(x, y)
        assert (p is None) == (ids[y, x].max() < 0)
        if p is not None:
            assert (p["vol_instance"], p["sdf"]) == tuple(ids[y, x])
            assert same(np.append(p["position"], np.float32(p["distance"])), hit[y, x])
    s.close()


def test_state_staging_follows_the_slots(vpt):
    host, dev = scene_at_a(vpt, SCENE_03)
    s = session_at_a(vpt, dev, "pathtrace")
    s.state()
    move_to_b(vpt, host, s, "pathtrace")
    s.advance(4)
    got = s.state()
    s.close()
    fresh = fresh_at_b(vpt, dev, "pathtrace")
    fresh.advance(4)
    want = fresh.state()
    fresh.close()
    assert got.samples == want.samples == 4
    assert same(got.image, want.image) and same(got.hits, want.hits) and same(got.rngs, want.rngs)
    assert got.image.any()


def test_adaptive_planes_follow_the_slots(vpt):
    adaptive = (0.05, 2, 2)   # threshold, min_samples, step
    host, dev = scene_at_a(vpt, SCENE_03)
    s = session_at_a(vpt, dev, "pathtrace", adaptive=adaptive)
    s.advance(4)
    s.noise(), s.hits()
    move_to_b(vpt, host, s, "pathtrace")

    def planes(session):
        session.advance(4)
        return (*session.noise(), session.hits(), *session.adaptive_stats())
    got = planes(s)
    s.close()
    fresh = fresh_at_b(vpt, dev, "pathtrace", adaptive=adaptive)
    want = planes(fresh)
    fresh.close()
    for name, g, w in zip(("se2", "variance", "hits", "mean", "m2"), got, want):
        assert same(g, w), name
        assert g.any(), name


def test_filter_buffers_go_and_come_back_at_the_new_slots(vpt):
    host, dev = scene_at_a(vpt, SCENE_03)
    s = session_at_a(vpt, dev, "pathtrace", denoise=True, guide_samples=2)
    s.advance(4)
    s.reset(denoise=False)
    with pytest.raises(vpt.VptError, match="no guides"):
        s.guides()
    with pytest.raises(vpt.VptError, match="no filtered image"):
        s.image(denoised=True)
    move_to_b(vpt, host, s, "pathtrace", denoise=True)

    def filtered(session):
        session.advance(4)
        return (*session.guides(), session.image(denoised=True))
    got = filtered(s)
    s.close()
    fresh = fresh_at_b(vpt, dev, "pathtrace", denoise=True, guide_samples=2)
    want = filtered(fresh)
    fresh.close()
    for name, g, w in zip(("normal", "albedo", "denoised"), got, want):
        assert same(g, w), name
        assert g.any(), name


@pytest.mark.parametrize("kind", ["implicit", "mesh"])
def test_the_two_id_frames_stay_independent(vpt, kind):
    """a session makes the id frame of its own shader family and keeps refusing the other one's, before and after the move"""
    path, shader = (GRID, "implicit") if kind == "implicit" else (SCENE_03, "pathtrace")
    host, dev = scene_at_a(vpt, path)
    s = session_at_a(vpt, dev, shader)

    def own_and_other():
        w, h = s.size
        buf = np.zeros((h, w, 2), np.int32)
        if kind == "implicit":
            own = s.sdf_ids()
            assert vpt.hip.vpt_session_get_ids(s.handle, buf.ctypes.data, None) == UNSUPPORTED
            with pytest.raises(vpt.VptError):
                s.pick(1, 1)
            again = s.sdf_ids()
        else:
            own = s.ids()
            assert vpt.hip.vpt_session_get_sdf_ids(s.handle, buf.ctypes.data, None) == UNSUPPORTED
            with pytest.raises(vpt.VptError):
                s.pick_sdf(1, 1)
            again = s.ids()
        assert not buf.any()   # a refused call writes nothing
        assert all(same(a, b) for a, b in zip(own, again))
        return own
    own_and_other()
    move_to_b(vpt, host, s, shader)
    got = own_and_other()
    s.close()
    fresh = fresh_at_b(vpt, dev, shader)
    want = fresh.sdf_ids() if kind == "implicit" else fresh.ids()
    fresh.close()
    assert all(same(g, w) for g, w in zip(got, want))
