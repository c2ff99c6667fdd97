"""vpt_scene_sculpt_volumes on the GPU (include/vpt.h).  The criterion is equality of bits, no tolerance anywhere: A =
DeviceScene(06_gridsdf_synth) after A.sculpt_volumes(edit) against the host mirror (HostScene.sculpt_volume, pinned to the reference's
functions and to a numpy replay of the rule by tests/test_sculpt_host.py) and against B = a DeviceScene made from the sculpted host scene.
Compared: vpt_scene_get_voxels of every volume, renders with implicit and implicit_normal at 96 pixels and 2 samples (image as uint32,
rngs, hits), the six hashes of the light tables.  The cases are tests/sculpt_cases.py's; test_sculpt_host.py shows that each of them
changes at least 1 % of its region's voxels and the sign of at least one."""
import ctypes as C

import numpy as np
import pytest

import sculpt_cases as S

pytestmark = pytest.mark.gpu
F = np.float32
SHADERS = ("implicit", "implicit_normal")
NAN_WORD = 0x7fc12345


def render(vpt, dev, host, shader, spp=2):
    p = vpt.PathtraceParams(resolution=96, samples=spp, shader=shader, bounces=4)
    st = host.make_state(p)
    dev.pathtrace_samples(st, p, spp)
    return st


def same_state(a, b):
    return (a.samples == b.samples and np.array_equal(a.image.view(np.uint32), b.image.view(np.uint32)) and np.array_equal(a.rngs, b.rngs)
            and np.array_equal(a.hits, b.hits))


def voxels(dev):
    return [S.bits(dev.get_voxels(k)).tobytes() for k in (S.SACKBOY, S.BUNNY)]


def mirror(host):
    return [S.bits(host.volume(k)[0]).tobytes() for k in (S.SACKBOY, S.BUNNY)]


@pytest.fixture(scope="module")
def original(vpt):
    """the unedited scene, made once and never edited: (host scene, its six hashes, its render per shader, its voxels)"""
    host = vpt.HostScene(S.GRID)
    dev = vpt.DeviceScene(host, 0)
    return host, dev.light_tables_hash(), {s: render(vpt, dev, host, s) for s in SHADERS}, voxels(dev)


@pytest.fixture(scope="module")
def all_cases(vpt):
    return S.cases(vpt)


def fresh_pair(vpt):
    """(a resident scene of the unedited file, a host scene of the same file to sculpt)"""
    return vpt.DeviceScene(vpt.HostScene(S.GRID), 0), vpt.HostScene(S.GRID)


def assert_equals_mirror_and_fresh(vpt, A, host, original, what, renders=True):
    assert voxels(A) == mirror(host), f"{what}: voxels differ from the host mirror's"
    assert A.light_tables_hash() == original[1], f"{what}: the light tables changed"
    if renders:
        B = vpt.DeviceScene(host, 0)
        assert voxels(B) == mirror(host)
        for shader in SHADERS:
            assert same_state(render(vpt, A, host, shader), render(vpt, B, host, shader)), f"{what}: {shader} differs from a fresh handle's"


@pytest.mark.parametrize("name", S.NAMES)
def test_sculpt_equals_the_mirror_and_a_fresh_scene(vpt, original, all_cases, name):
    """every type x every op x both blends on a rotated frame; a 1-voxel region, REGION, rows of 37, the whole grid, strokes of 1 and 33
    stamps (the records are read through a uniform index, not staged in pieces: there is no piece size to straddle), identity axes, a
    REPLACE first (the kernel does not read), a grid of the caller's own"""
    A, host = fresh_pair(vpt)
    entry = S.apply(host, all_cases[name])
    edit = host.update_sculpts()
    A.sculpt_volumes(edit)
    launches, sent, ms = A.update_stats()
    print(f"{name}: {(launches, sent, ms)} (launches, bytes, device ms)", flush=True)
    assert (launches, sent) == (1, vpt.SCULPT_RECORD_BYTES * len(entry.stamps)) and sent == edit.payload_bytes()
    assert_equals_mirror_and_fresh(vpt, A, host, original, name)
    assert voxels(A)[S.BUNNY] != original[3][S.BUNNY] and voxels(A)[S.SACKBOY] == original[3][S.SACKBOY]


def test_nothing_to_do_launches_nothing(vpt, original):
    """an empty region, an entry without stamps, an edit without entries: no launch, no byte, no voxel"""
    A, host = fresh_pair(vpt)
    stamp = vpt.Stamp(S.brush(vpt, "sphere"), S.REPLACE)
    host.sculpt_volume(S.BUNNY, [stamp], region=((5, 5, 5), (0, 7, 7)))
    host.sculpt_volume(S.BUNNY, [stamp], region=((40, 40, 40), (0, 0, 0)))
    host.sculpt_volume(S.SACKBOY, [])
    edit = host.update_sculpts()
    assert len(edit.entries) == 3 and edit.payload_bytes() == 0
    corner = vpt.SculptEdit([vpt.SculptEntry(S.BUNNY, (0, 0, 0), (2, 2, 2), 0.0, 1.0, [stamp])])   # an edit with work, so that the counters show a launch
    A.sculpt_volumes(corner)
    assert A.update_stats()[:2] == (1, 80) and corner.payload_bytes() == 80
    A2, _ = fresh_pair(vpt)
    A2.sculpt_volumes(corner)
    A2.sculpt_volumes(edit)
    assert A2.update_stats()[:2] == (0, 0) and voxels(A2) == voxels(A)
    A2.sculpt_volumes(corner)
    A2.sculpt_volumes(vpt.SculptEdit())
    assert A2.update_stats()[:2] == (0, 0) and voxels(A2) == voxels(A)
    # one entry of three has work: one launch, the whole list's records
    B, host2 = fresh_pair(vpt)
    host2.sculpt_volume(S.BUNNY, [stamp], region=((5, 5, 5), (0, 7, 7)))
    host2.sculpt_volume(S.BUNNY, [stamp, stamp], region=S.REGION)
    host2.sculpt_volume(S.SACKBOY, [])
    B.sculpt_volumes(host2.update_sculpts())
    assert B.update_stats()[:2] == (1, 3 * 80)
    assert_equals_mirror_and_fresh(vpt, B, host2, original, "one entry of three", renders=False)


def test_a_stroke_equals_its_stamps_and_two_entries_equal_two_edits(vpt, original):
    stamps = S.stroke(vpt, 33)
    A, host = fresh_pair(vpt)
    whole = host.sculpt_volume(S.BUNNY, stamps, region=S.BOX)
    A.sculpt_volumes(host.update_sculpts())
    assert A.update_stats()[:2] == (1, 33 * 80)
    B, _ = fresh_pair(vpt)
    for s in stamps:
        B.sculpt_volumes(vpt.SculptEdit([vpt.SculptEntry(S.BUNNY, whole.region_lo, whole.region_whd, whole.origin, whole.step, [s])]))
        assert B.update_stats()[:2] == (1, 80)
    assert voxels(A)[S.BUNNY] == voxels(B)[S.BUNNY] == mirror(host)[S.BUNNY]
    # the same volume twice in one edit, overlapping regions, and the other volume between them: in order
    C1, host1 = fresh_pair(vpt)
    first = host1.sculpt_volume(S.BUNNY, stamps[:5], region=S.BOX)
    other = host1.sculpt_volume(S.SACKBOY, [vpt.Stamp(S.brush(vpt, "sphere", (70.0, 70.0, 70.0), S.rotation(), scale=1000.0), S.REPLACE, 2.0)], region=S.REGION)
    second = host1.sculpt_volume(S.BUNNY, [vpt.Stamp(S.brush(vpt, "plane", S.CENTRE, S.rotation(0.3, 0.5)), S.INTERSECT, 0.01)], region=S.ROWS)
    edit = host1.update_sculpts()
    assert [e.volume for e in edit.entries] == [S.BUNNY, S.SACKBOY, S.BUNNY]
    C1.sculpt_volumes(edit)
    assert C1.update_stats()[:2] == (3, 7 * 80)
    C2, _ = fresh_pair(vpt)
    for e in (first, other, second):
        C2.sculpt_volumes(vpt.SculptEdit([e]))
    assert voxels(C1) == voxels(C2)
    assert_equals_mirror_and_fresh(vpt, C1, host1, original, "two entries on one volume")
    assert voxels(C1)[S.SACKBOY] != original[3][S.SACKBOY]


def test_resident_nans(vpt, original):
    """NaN voxels written by set_volume first: UNION and INTERSECT replace them, SUBTRACT keeps their bits (blend 0)"""
    grid = original[0].volume(S.BUNNY)[0].copy()
    nan = np.array([NAN_WORD], np.uint32).view(F)[0]
    grid.reshape(-1)[::7] = nan
    sphere = S.brush(vpt, "sphere", S.CENTRE, S.rotation())
    for op, kept in ((S.UNION, False), (S.INTERSECT, False), (S.SUBTRACT, True)):
        A, host = fresh_pair(vpt)
        host.set_volume(S.BUNNY, grid)
        A.update_volumes(host.update_volumes())
        assert (S.bits(A.get_voxels(S.BUNNY)).reshape(-1)[::7] == NAN_WORD).all()
        host.sculpt_volume(S.BUNNY, [vpt.Stamp(sphere, op)])
        A.sculpt_volumes(host.update_sculpts())
        got = A.get_voxels(S.BUNNY).reshape(-1)[::7]
        assert (S.bits(got) == NAN_WORD).all() if kept else not np.isnan(got).any(), op
        assert_equals_mirror_and_fresh(vpt, A, host, original, f"NaN voxels, op {op}", renders=False)


def test_bytes_do_not_depend_on_the_region(vpt):
    """bytes = stamps x the record size, whatever the region: not one voxel crosses"""
    sent = []
    for region in (S.ONE, S.WHOLE):
        A, host = fresh_pair(vpt)
        host.sculpt_volume(S.BUNNY, S.stroke(vpt, 5), region=region)
        A.sculpt_volumes(host.update_sculpts())
        sent.append(A.update_stats()[:2])
    assert sent == [(1, 5 * vpt.SCULPT_RECORD_BYTES)] * 2 and vpt.SCULPT_RECORD_BYTES == 80


def _entry(vpt, stamps, volume=S.BUNNY, region=S.REGION, origin=(0.0, 0.0, 0.0), step=(0.1, 0.1, 0.1)):
    return vpt.SculptEntry(volume, region[0], region[1], origin, step, stamps)


def _stamp(vpt, **changes):
    s = vpt.Stamp(S.brush(vpt, "sphere"), S.REPLACE)
    for k, v in changes.items():
        if k in ("op", "blend"):
            setattr(s, k, v)
        elif k == "type":
            s.brush.type = v
        else:
            getattr(s.brush if k in ("whd", "p") else s.brush.frame, k)[0] = v
    return s


REFUSALS = {   # one per class of the validation: name -> (entries, what the message names)
    "volume": lambda vpt: ([_entry(vpt, [_stamp(vpt)]), _entry(vpt, [_stamp(vpt)], volume=2)], "entry 1: volume 2 out of range"),
    "region": lambda vpt: ([_entry(vpt, [_stamp(vpt)], region=((38, 0, 0), (3, 1, 1)))], "entry 0: the region leaves the grid"),
    "type": lambda vpt: ([_entry(vpt, [_stamp(vpt), _stamp(vpt, type=-1)])], "stamp 1: the brush's type"),
    "op": lambda vpt: ([_entry(vpt, [_stamp(vpt, op=4)])], "stamp 0: op"),
    "float": lambda vpt: ([_entry(vpt, [_stamp(vpt)]), _entry(vpt, [_stamp(vpt, z=np.nan)])], "stamp 1: a value is not finite"),
    "blend": lambda vpt: ([_entry(vpt, [_stamp(vpt, blend=-1.0)])], "stamp 0: blend is negative"),
    "step": lambda vpt: ([_entry(vpt, [_stamp(vpt)], step=(0.1, np.inf, 0.1))], "entry 0: origin or step is not finite"),
}


@pytest.fixture(scope="module")
def resident(vpt, original):
    """one resident scene for all refusals: each must leave it as it was"""
    return vpt.DeviceScene(vpt.HostScene(S.GRID), 0)


def assert_untouched(vpt, dev, original):
    host, hashes, renders, vox = original
    assert voxels(dev) == vox and dev.light_tables_hash() == hashes
    for shader in SHADERS:
        assert same_state(render(vpt, dev, host, shader), renders[shader]), shader


@pytest.mark.parametrize("name", list(REFUSALS))
def test_a_refused_edit_names_its_entry_or_stamp_and_leaves_the_scene(vpt, original, resident, name):
    import re
    entries, named = REFUSALS[name](vpt)
    with pytest.raises(vpt.VptError, match=re.escape(named)):
        resident.sculpt_volumes(vpt.SculptEdit(entries))
    assert_untouched(vpt, resident, original)


def test_stamp_range_and_work_guard_are_refused_from_the_descriptor_alone(vpt, original, resident):
    """a stamp range that leaves the edit's list; and the work guard with a descriptor only: 621 379 zeroed stamps (type 0, op 0, every
    float 0: valid) over the sackboy's 48^3 voxels are 2^36 evaluations and some - VPT_ERR_UNSUPPORTED before anything is launched"""
    entry = vpt.VptSculptEntry(volume=S.SACKBOY, first_stamp=1, num_stamps=1)
    entry.region_whd[:], entry.step[:] = (48, 48, 48), (1, 1, 1)
    one = (vpt.VptSculptStamp * 1)(_stamp(vpt).to_abi())
    edit = vpt.VptSculptEdit(1, C.addressof(entry), 1, C.addressof(one))
    assert vpt.hip.vpt_scene_sculpt_volumes(resident.handle, C.byref(edit)) == -1   # VPT_ERR_INVALID_ARG
    assert b"entry 0: the stamp range leaves the edit's list" in vpt.hip.vpt_last_error()
    many = np.zeros((621379, C.sizeof(vpt.VptSculptStamp)), np.uint8)
    entry.first_stamp, entry.num_stamps = 0, len(many)
    edit = vpt.VptSculptEdit(1, C.addressof(entry), len(many), many.ctypes.data)
    assert 48 ** 3 * len(many) > 2 ** 36 >= 48 ** 3 * (len(many) - 1)
    before = resident.update_stats()
    assert vpt.hip.vpt_scene_sculpt_volumes(resident.handle, C.byref(edit)) == -5   # VPT_ERR_UNSUPPORTED
    assert b"entry 0" in vpt.hip.vpt_last_error() and b"split the stroke" in vpt.hip.vpt_last_error()
    assert resident.update_stats() == before
    assert vpt.hip.vpt_scene_sculpt_volumes(resident.handle, None) == -1
    assert_untouched(vpt, resident, original)


# ---- the session ------------------------------------------------------------------------------------------------------------------------
def test_session_edit_sculpts_resets_and_sculpt_at_follows_the_pick(vpt, original):
    host = vpt.HostScene(S.GRID)   # a scene of its own: the session edits it
    dev = vpt.DeviceScene(host, 0)
    params = vpt.PathtraceParams(resolution=96, samples=8, shader="implicit", bounces=2)
    s = vpt.RenderSession(dev, params)
    s.advance(2)
    ids, hit = s.sdf_ids()
    bunny_pixels = np.argwhere(np.isin(ids[..., 0], S.BUNNY_INSTANCES))
    sdf_pixels = np.argwhere(ids[..., 1] >= 0)
    miss_pixels = np.argwhere(ids.max(axis=-1) < 0)
    assert len(bunny_pixels) and len(sdf_pixels) and len(miss_pixels)

    # edit_sculpts: the edit, then a reset - the next frames are a fresh session's on the sculpted scene
    host.sculpt_volume(S.BUNNY, S.stroke(vpt, 5), region=S.BOX)
    s.edit_sculpts(host.update_sculpts())
    assert s.samples == 0
    s.advance(2)
    fresh = vpt.RenderSession(vpt.DeviceScene(host, 0), params)
    fresh.advance(2)
    a, b = s.state(), fresh.state()
    assert same_state(a, b) and np.array_equal(S.bits(s.image()), S.bits(fresh.image()))
    ids2, hit2 = s.sdf_ids()                  # the id frame is remade after the edit ...
    ids3, hit3 = fresh.sdf_ids()
    assert np.array_equal(ids2, ids3) and np.array_equal(S.bits(hit2), S.bits(hit3))
    assert not np.array_equal(S.bits(hit2), S.bits(hit))   # ... and it shows the carved bunny
    fresh.close()

    # sculpt_at: on a pixel of the bunny it changes that volume alone, around the hit
    y, x = (int(c) for c in bunny_pixels[len(bunny_pixels) // 2])
    pick = s.pick_sdf(x, y)
    assert pick is not None and pick["volume"] == S.BUNNY
    before = [host.volume(k)[0].copy() for k in (S.SACKBOY, S.BUNNY)]
    ball = vpt.VptSdf(type=S.TYPES.index("sphere"))
    ball.frame.x[:], ball.frame.y[:], ball.frame.z[:], ball.p[0] = (1, 0, 0), (0, 1, 0), (0, 0, 1), 0.012
    entry = s.sculpt_at(host, x, y, ball, vpt.SCULPT_SUBTRACT, blend=0.002)
    assert entry.volume == S.BUNNY and len(entry.stamps) == 1 and all(0 < n < 40 for n in entry.region_whd) and s.samples == 0
    after = [host.volume(k)[0] for k in (S.SACKBOY, S.BUNNY)]
    assert np.array_equal(S.bits(after[S.SACKBOY]), S.bits(before[S.SACKBOY]))
    changed = np.argwhere(S.bits(after[S.BUNNY]) != S.bits(before[S.BUNNY]))[:, ::-1]   # (x, y, z)
    lo, size = np.array(entry.region_lo), np.array(entry.region_whd)
    assert len(changed) >= 10 and (changed >= lo).all() and (changed < lo + size).all()
    # the dent is where the pick was: the brush's local origin, taken back through its frame, is the hit in voxel space
    inst = host.volume_instance(pick["vol_instance"])
    centre = (pick["position"].astype(np.float64) @ np.array([inst.frame.x[:], inst.frame.y[:], inst.frame.z[:]]) + np.array(inst.frame.o[:])) / inst.scalef
    assert np.allclose(-np.array(entry.stamps[0].brush.frame.o[:]), centre, atol=1e-6)
    flipped = np.argwhere((after[S.BUNNY] > 0) & (before[S.BUNNY] < 0))[:, ::-1]   # carved: inside the ball, up to the blend
    assert len(flipped) and np.linalg.norm(flipped * np.array(entry.step) - centre, axis=1).max() < 0.012 + 0.002
    assert voxels(dev) == mirror(host)
    p = s.pick_sdf(x, y)                       # the id frame again: the ray now ends behind the dent, or on another object, or nowhere
    assert p is None or p["distance"] > pick["distance"] or p["vol_instance"] != pick["vol_instance"]

    # an analytic SDF or a miss under the pixel: VptError, nothing changes
    for pixels, what in ((sdf_pixels, "analytic SDF"), (miss_pixels, "hits nothing")):
        yy, xx = (int(c) for c in pixels[len(pixels) // 2])
        with pytest.raises(vpt.VptError, match=what):
            s.sculpt_at(host, xx, yy, ball, vpt.SCULPT_SUBTRACT)
    assert voxels(dev) == mirror(host) and host.update_sculpts().empty()
    # a refused edit leaves the session as it was
    s.advance(1)
    with pytest.raises(vpt.VptError, match="entry 0: the region leaves the grid"):
        s.edit_sculpts(vpt.SculptEdit([_entry(vpt, [_stamp(vpt)], region=((38, 0, 0), (3, 1, 1)))]))
    assert s.samples == 1
    s.close()


# ---- several devices, several kinds of edit -------------------------------------------------------------------------------------------
def test_multi_device_scene_on_one_device(vpt, original):
    host = vpt.HostScene(S.GRID)
    multi = vpt.MultiDeviceScene(vpt.HostScene(S.GRID), [0])
    host.sculpt_volume(S.BUNNY, S.stroke(vpt, 3), region=S.BOX)
    multi.sculpt_volumes(host.update_sculpts())
    B = vpt.DeviceScene(host, 0)
    for shader in SHADERS:
        p = vpt.PathtraceParams(resolution=96, samples=2, shader=shader, bounces=4)
        st = host.make_state(p)
        multi.pathtrace_samples(st, p, 2)
        assert same_state(st, render(vpt, B, host, shader)) and not same_state(st, original[2][shader]), shader
    with pytest.raises(vpt.VptError, match="entry 0: the region leaves the grid"):
        multi.sculpt_volumes(vpt.SculptEdit([_entry(vpt, [_stamp(vpt)], region=((38, 0, 0), (3, 1, 1)))]))


def test_sculpts_and_volume_edits_interleave(vpt, original):
    """sculpt, then update_volumes (new voxels in a region, a moved instance, a volume that grows: the pool is allocated anew), then
    sculpt again, on one handle: the fresh scene's voxels and renders"""
    A, host = fresh_pair(vpt)
    host.sculpt_volume(S.BUNNY, S.stroke(vpt, 4), region=S.BOX)
    A.sculpt_volumes(host.update_sculpts())
    rng = np.random.default_rng(3)
    host.set_volume(S.BUNNY, (rng.random((2, 3, 5), dtype=F) * F(0.01)).astype(F), region=S.REGION, mode=vpt.VOXELS_UNION)
    sack = host.volume(S.SACKBOY)[0]
    host.set_volume(S.SACKBOY, np.pad(sack, ((0, 1), (0, 2), (0, 0)), mode="edge"))
    host.set_volume_instance(2, scalef=1.25)
    A.update_volumes(host.update_volumes())
    host.sculpt_volume(S.BUNNY, [vpt.Stamp(S.brush(vpt, "torus", S.CENTRE, S.rotation()), S.UNION, 0.01)])
    host.sculpt_volume(S.SACKBOY, [vpt.Stamp(S.brush(vpt, "sphere", (70.0, 70.0, 70.0), scale=1000.0), S.SUBTRACT)], region=((3, 4, 5), (41, 45, 44)))
    A.sculpt_volumes(host.update_sculpts())
    assert A.update_stats()[:2] == (2, 160)
    assert tuple(A.get_volumes()[0][S.SACKBOY].whd) == (48, 50, 49)
    B = vpt.DeviceScene(host, 0)
    assert voxels(A) == mirror(host) == voxels(B)
    for shader in SHADERS:
        assert same_state(render(vpt, A, host, shader), render(vpt, B, host, shader)), shader
    assert A.light_tables_hash() == B.light_tables_hash()
