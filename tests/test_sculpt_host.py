"""Sculpting voxel grids with analytic SDF brushes, the host side (include/vpt.h: vpt_scene_sculpt_volumes).  No GPU.
The rule is one header (csrc/vpt_sculpt_rule.h) that the kernel and the host mirror compile; here the host mirror is pinned:
 * its six brush functions to the reference's own sdf_data::f, bit for bit, on the committed table of tests/test_kat.py and on a wider
   one (tests/golden/sculpt_kat.npz, made by tests/golden/make_sculpt_fixtures.py from the reference build);
 * its ops to truth tables written out here;
 * HostScene.sculpt_volume to a numpy replay of the rule, float32 operation by operation (tests/sculpt_cases.py);
 * every case the GPU tests run to an edit that does something;
 * the refusals, the ledger rules and the struct sizes."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import kat_lib as K
import sculpt_cases as S
from conftest import GOLDEN, ROOT

F = np.float32
WIDE = os.path.join(GOLDEN, "sculpt_kat.npz")


@pytest.fixture(scope="module")
def original(vpt):
    """06_gridsdf_synth as loaded, never edited: (host scene, the bunny's grid, its res)"""
    host = vpt.HostScene(S.GRID)
    grid, res = host.volume(S.BUNNY)
    return host, grid, res


@pytest.fixture(scope="module")
def all_cases(vpt):
    return S.cases(vpt)




# ---- the six functions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table,rows,key", [(K.TABLES, 4096, "sdf_function_sdfn"), (WIDE, 5834, "sdf_function")])
def test_brush_distance_is_the_references_function_bit_for_bit(vpt, table, rows, key):
    with np.load(table) as t:
        rec, ref = t[key + "_in"], t[key + "_out"][:, 0]
    assert len(rec) == rows
    host = vpt.HostScene(S.SDFS)
    nsdf = host.count_implicit("sdfs")
    assert set(np.unique(rec[:, 0]).astype(int)) == set(range(nsdf)) and {host.sdf(i).type for i in range(nsdf)} == set(range(6))
    got = np.zeros(len(rec), F)
    for i in range(nsdf):
        rows_i = rec[:, 0] == i
        got[rows_i] = S.brush_distance(vpt, host.sdf(i), rec[rows_i, 1:4])
    assert not np.isnan(ref).any()
    wrong = np.argwhere(S.bits(got) != S.bits(ref))[:, 0]
    assert len(wrong) == 0, (len(wrong), rec[wrong[:5]].tolist(), got[wrong[:5]].tolist(), ref[wrong[:5]].tolist())


def test_the_wider_table_is_wider(vpt):
    with np.load(WIDE) as t:
        rec = t["sdf_function_in"]
    assert os.path.getsize(WIDE) < 200 * 1024
    assert np.abs(rec[:4096, 1:4]).max() > 1.4 and (rec[4096:, 1:4] == 0).all(axis=1).sum() >= 10   # +-1.5, and the origin once per SDF


# ---- the ops ----------------------------------------------------------------------------------------------------------------------------
NAN = struct.unpack("<f", struct.pack("<I", 0x7fc12345))[0]   # a quiet NaN with a payload
VALUES = np.array([-1.0, -0.0, 0.0, 0.5, NAN], F)
PAIRS_A, PAIRS_B = (v.reshape(-1).copy() for v in np.meshgrid(VALUES, VALUES, indexing="ij"))


def combine(vpt, op, k, a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    out = np.zeros(len(a), F)
    assert vpt.host.vpth_sculpt_combine(op, C.c_float(k), a.ctypes.data, b.ctypes.data, len(a), out.ctypes.data) == 0
    return out


def word(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def test_ops_without_blend_are_the_references_selects(vpt):
    """REPLACE b; UNION (a < b) ? a : b; SUBTRACT (-b > a) ? -b : a; INTERSECT (a > b) ? a : b, on floats whose order Python's own
    comparisons decide as IEEE does: bits compared, a NaN that passes through keeps its payload"""
    assert S.bits(PAIRS_A)[-1] == 0x7fc12345 and len(PAIRS_A) == 25
    select = {S.REPLACE: lambda a, b: b, S.UNION: lambda a, b: a if a < b else b, S.SUBTRACT: lambda a, b: -b if -b > a else a,
              S.INTERSECT: lambda a, b: a if a > b else b}
    for op, rule in select.items():
        got = combine(vpt, op, 0.0, PAIRS_A, PAIRS_B)
        for a, b, g in zip(PAIRS_A, PAIRS_B, got):
            want = rule(float(a), float(b))   # (float32 -> double -> float32 keeps the bits, a NaN's payload included)
            assert word(g) == word(want), (op, a, b, g, want)
    # what the contract says about NaN in so many words: a NaN resident value is replaced by UNION and INTERSECT, kept by SUBTRACT
    nan, half = np.array([NAN], F), np.array([0.5], F)
    assert S.bits(combine(vpt, S.UNION, 0.0, nan, half))[0] == S.bits(half)[0] == S.bits(combine(vpt, S.INTERSECT, 0.0, nan, half))[0]
    assert S.bits(combine(vpt, S.SUBTRACT, 0.0, nan, half))[0] == 0x7fc12345
    # -0 against +0: neither is less, so the second operand of the select is taken
    assert word(combine(vpt, S.UNION, 0.0, [-0.0], [0.0])[0]) == word(0.0) and word(combine(vpt, S.UNION, 0.0, [0.0], [-0.0])[0]) == word(-0.0)


def test_ops_with_blend_are_the_polynomial_smooth_minimum(vpt):
    """k = 0.25: m - ((h * h) * k) * 0.25 with h = max(k - |x - y|, 0) / k, operation by operation in numpy; bits on the pairs without a
    NaN, `is NaN` on the others (an arithmetic NaN's payload is the processor's)"""
    k = 0.25
    for op in (S.REPLACE, S.UNION, S.SUBTRACT, S.INTERSECT):
        got, want = combine(vpt, op, k, PAIRS_A, PAIRS_B), S.combine(op, k, PAIRS_A, PAIRS_B)
        clean = ~(np.isnan(PAIRS_A) | np.isnan(PAIRS_B))
        assert clean.sum() == 16 and np.array_equal(S.bits(got)[clean], S.bits(want)[clean]), op
        assert np.array_equal(np.isnan(got), np.isnan(want)), op
    # values written out by hand: smin(0, 0.125, 0.25) = 0 - (0.5 * 0.5 * 0.25) * 0.25
    assert combine(vpt, S.UNION, k, [0.0], [0.125])[0] == F(-0.015625)
    assert combine(vpt, S.SUBTRACT, k, [0.0], [0.125])[0] == F(0.015625) and combine(vpt, S.INTERSECT, k, [0.0], [0.125])[0] == F(0.140625)
    # further apart than k: the plain minimum / maximum
    assert combine(vpt, S.UNION, k, [-1.0], [0.5])[0] == F(-1) and combine(vpt, S.INTERSECT, k, [-1.0], [0.5])[0] == F(0.5)
    assert combine(vpt, S.REPLACE, k, [-1.0], [0.5])[0] == F(0.5)


# ---- the mirror against the replay ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_mirror_equals_the_numpy_replay_and_the_edit_does_something(vpt, original, all_cases, name):
    """every type x every op x both blends on a rotated, translated frame, regions that are not the grid, strokes, a grid of the
    caller's own.  Outside the region every voxel keeps its bits; inside, at least 1 % change and at least one changes sign - these are the
    cases tests/test_sculpt_gpu.py runs."""
    _, grid, res = original
    assert list(all_cases) == S.NAMES
    case = all_cases[name]
    host = vpt.HostScene(S.GRID)
    entry = S.apply(host, case)
    got = host.volume(S.BUNNY)[0]
    want = S.replay(vpt, grid, res, case)
    assert np.array_equal(S.bits(got), S.bits(want)), name
    assert np.array_equal(S.bits(host.volume(S.SACKBOY)[0]), S.bits(original[0].volume(S.SACKBOY)[0]))
    lo, size = entry.region_lo, entry.region_whd
    inside = np.zeros(grid.shape, bool)
    inside[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]] = True
    changed = S.bits(got) != S.bits(grid)
    assert not changed[~inside].any(), f"{name}: a voxel outside the region changed"
    assert changed[inside].mean() >= 0.01, f"{name}: {changed[inside].mean():.4f} of the region's voxels change"
    assert ((got < 0) != (grid < 0))[inside].any(), f"{name}: no voxel changes sign"


def test_a_stroke_equals_its_stamps_one_at_a_time(vpt):
    stamps = S.stroke(vpt, 33)
    whole, single = vpt.HostScene(S.GRID), vpt.HostScene(S.GRID)
    whole.sculpt_volume(S.BUNNY, stamps, region=S.BOX)
    for s in stamps:
        single.sculpt_volume(S.BUNNY, [s], region=S.BOX)
    assert np.array_equal(S.bits(whole.volume(S.BUNNY)[0]), S.bits(single.volume(S.BUNNY)[0]))
    assert len(whole.update_sculpts().entries) == 1 and len(single.update_sculpts().entries) == 33


def test_resident_nans_are_replaced_by_union_and_kept_by_subtract(vpt, original):
    _, grid, res = original
    holes = grid.copy()
    holes.reshape(-1)[::7] = NAN
    sphere = S.brush(vpt, "sphere", S.CENTRE, S.rotation())
    for op, kept in ((S.UNION, False), (S.INTERSECT, False), (S.SUBTRACT, True)):
        host = vpt.HostScene(S.GRID)
        host.set_volume(S.BUNNY, holes)
        host.update_volumes()
        host.sculpt_volume(S.BUNNY, [vpt.Stamp(sphere, op)])
        got = host.volume(S.BUNNY)[0]
        assert np.array_equal(S.bits(got), S.bits(S.replay(vpt, holes, res, (S.BUNNY, [vpt.Stamp(sphere, op)], None, None, None))))
        at = got.reshape(-1)[::7]
        assert (S.bits(at) == 0x7fc12345).all() if kept else not np.isnan(at).any(), op


# ---- refusals, ledgers, sizes -----------------------------------------------------------------------------------------------------------
def _stamp(vpt, **changes):
    s = vpt.Stamp(S.brush(vpt, "sphere"), S.SUBTRACT)
    for k, v in changes.items():
        if k in ("op", "blend"):
            setattr(s, k, v)
        elif k == "type":
            s.brush.type = v
        else:
            getattr(s.brush if k in ("whd", "p") else s.brush.frame, k)[0] = v
    return s


REFUSALS = {   # name -> (arguments of sculpt_volume after the HostScene, what the message names)
    "volume": lambda vpt: ((7, [_stamp(vpt)]), {}, "volume 7 out of range"),
    "region_leaves": lambda vpt: ((S.BUNNY, [_stamp(vpt)]), dict(region=((38, 0, 0), (3, 1, 1))), "entry 0: the region leaves the grid"),
    "region_negative": lambda vpt: ((S.BUNNY, [_stamp(vpt)]), dict(region=((-1, 0, 0), (3, 1, 1))), "entry 0: the region leaves the grid"),
    "type": lambda vpt: ((S.BUNNY, [_stamp(vpt), _stamp(vpt, type=6)]), {}, "stamp 1: the brush's type"),
    "op": lambda vpt: ((S.BUNNY, [_stamp(vpt, op=4)]), {}, "stamp 0: op"),
    "frame": lambda vpt: ((S.BUNNY, [_stamp(vpt, o=np.inf)]), {}, "stamp 0: a value is not finite"),
    "whd": lambda vpt: ((S.BUNNY, [_stamp(vpt, whd=np.nan)]), {}, "stamp 0: a value is not finite"),
    "p": lambda vpt: ((S.BUNNY, [_stamp(vpt, p=-np.inf)]), {}, "stamp 0: a value is not finite"),
    "blend_nan": lambda vpt: ((S.BUNNY, [_stamp(vpt, blend=np.nan)]), {}, "stamp 0: a value is not finite"),
    "blend_negative": lambda vpt: ((S.BUNNY, [_stamp(vpt), _stamp(vpt), _stamp(vpt, blend=-0.5)]), {}, "stamp 2: blend is negative"),
    "origin": lambda vpt: ((S.BUNNY, [_stamp(vpt)]), dict(origin=(0, np.inf, 0)), "entry 0: origin or step is not finite"),
    "step": lambda vpt: ((S.BUNNY, [_stamp(vpt)]), dict(step=(0.1, 0.1, np.nan)), "entry 0: origin or step is not finite"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_a_refused_sculpt_names_its_entry_or_stamp_and_changes_nothing(vpt, original, name):
    args, kwargs, named = REFUSALS[name](vpt)
    host = vpt.HostScene(S.GRID)
    with pytest.raises(vpt.VptError, match=re.escape(named)):
        host.sculpt_volume(*args, **kwargs)
    assert np.array_equal(S.bits(host.volume(S.BUNNY)[0]), S.bits(original[1]))
    assert host.update_sculpts().empty()


def test_the_mirror_refuses_a_stamp_range_outside_the_list_and_too_much_work(vpt, original):
    """through the host library's entry point itself: HostScene.sculpt_volume always names its own stamps.  The work guard is tested with
    a descriptor alone: 2^36 / 48^3 = 621 378.4 zeroed stamps of the sackboy's whole grid are one too few to be refused, one more is refused
    before a voxel is touched"""
    host = vpt.HostScene(S.GRID)
    call = vpt.host.vpth_scene_sculpt_volume
    err = C.create_string_buffer(256)
    entry = vpt.VptSculptEntry(volume=S.SACKBOY, first_stamp=1, num_stamps=1)
    entry.region_whd[:], entry.step[:] = (48, 48, 48), (1, 1, 1)
    one = (vpt.VptSculptStamp * 1)(_stamp(vpt).to_abi())
    assert call(host.handle, C.byref(entry), C.addressof(one), 1, err, len(err)) != 0 and b"entry 0: the stamp range leaves the edit's list" in err.value
    many = np.zeros((621379, C.sizeof(vpt.VptSculptStamp)), np.uint8)   # type 0, op 0, every float 0: valid stamps
    entry.first_stamp, entry.num_stamps = 0, len(many)
    assert 48 ** 3 * len(many) > 2 ** 36 >= 48 ** 3 * (len(many) - 1)
    assert call(host.handle, C.byref(entry), many.ctypes.data, len(many), err, len(err)) != 0 and b"split the stroke" in err.value
    for k in (S.SACKBOY, S.BUNNY):
        assert np.array_equal(S.bits(host.volume(k)[0]), S.bits(original[0].volume(k)[0]))


def test_the_two_ledgers_of_a_volume_do_not_mix(vpt, original):
    _, grid, res = original
    stamp = vpt.Stamp(S.brush(vpt, "sphere"), S.SUBTRACT)
    host = vpt.HostScene(S.GRID)
    host.set_volume(S.BUNNY, grid + F(0.001))
    with pytest.raises(vpt.VptError, match=r"update_volumes\(\)"):
        host.sculpt_volume(S.BUNNY, [stamp])
    assert np.array_equal(S.bits(host.volume(S.BUNNY)[0]), S.bits(grid + F(0.001))) and host.update_sculpts().empty()
    host.sculpt_volume(S.SACKBOY, [stamp])            # another volume: free to go
    assert not host.update_volumes().empty()
    host.sculpt_volume(S.BUNNY, [stamp])              # handed out: free again
    after = host.volume(S.BUNNY)[0].copy()
    verts = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0]], F)
    for refused in (lambda: host.set_volume(S.BUNNY, grid), lambda: host.set_volume(S.SACKBOY, host.volume(S.SACKBOY)[0]),
                    lambda: host.bake_volume(S.BUNNY, verts, [[0, 1, 2]])):
        with pytest.raises(vpt.VptError, match=r"update_sculpts\(\)"):
            refused()
    assert np.array_equal(S.bits(host.volume(S.BUNNY)[0]), S.bits(after)) and host.update_volumes().empty()
    edit = host.update_sculpts()
    assert [e.volume for e in edit.entries] == [S.SACKBOY, S.BUNNY] and host.update_sculpts().empty()
    host.set_volume(S.BUNNY, grid)                    # handed out: free again
    assert list(host.update_volumes().volumes) == [S.BUNNY]
    # the other ledgers do not care: an instance frame, a texture or a camera may be pending while a volume is sculpted
    host.set_volume_instance(2, scalef=1.5)
    host.sculpt_volume(S.BUNNY, [stamp])
    assert not host.update_sculpts().empty() and list(host.update_volumes().vol_instances) == [2]


def test_defaults_are_those_of_bake_volume(vpt, original):
    _, grid, res = original
    host = vpt.HostScene(S.GRID)
    entry = host.sculpt_volume(S.BUNNY, [(S.brush(vpt, "sphere"), S.UNION)])   # a (brush, op) pair is a Stamp
    step = float(F(res) * F(40) / F(39))
    assert entry.region_lo == (0, 0, 0) and entry.region_whd == (40, 40, 40) and entry.origin == (0.0, 0.0, 0.0) and entry.step == (step,) * 3
    assert entry.stamps[0].blend == 0.0 and isinstance(entry.stamps[0], vpt.Stamp)


def test_struct_sizes_and_the_record_size_are_those_of_the_header(vpt):
    header = open(os.path.join(ROOT, "include", "vpt.h")).read()
    assert int(re.search(r"#define VPT_SCULPT_RECORD_BYTES (\d+)", header).group(1)) == vpt.SCULPT_RECORD_BYTES == 80
    # vpt_sculpt_stamp {vpt_sdf (84), int32, float}; vpt_sculpt_entry: 15 four-byte words; vpt_sculpt_edit: two {int32, pointer} pairs
    assert C.sizeof(vpt.VptSdf) == 84 and C.sizeof(vpt.VptSculptStamp) == 92 and C.sizeof(vpt.VptSculptEntry) == 60 and C.sizeof(vpt.VptSculptEdit) == 32
    for name, value in (("REPLACE", 0), ("UNION", 1), ("SUBTRACT", 2), ("INTERSECT", 3)):
        assert re.search(rf"VPT_SCULPT_{name} = {value}\b", header) and getattr(vpt, "SCULPT_" + name) == value
    a = vpt.Stamp(S.brush(vpt, "torus", S.CENTRE, S.rotation()), S.SUBTRACT, 0.25)
    b = vpt.Stamp(S.brush(vpt, "box"), S.UNION)
    edit = vpt.SculptEdit([vpt.SculptEntry(1, (1, 2, 3), (4, 5, 6), (0.5, 0.25, 0.125), (1, 2, 4), [a, b]), vpt.SculptEntry(0, (0, 0, 0), (0, 0, 0), 0.0, 1.0, [b])])
    abi, keep = edit.to_abi()
    entries, stamps = keep
    assert (abi.num_entries, abi.num_stamps) == (2, 3) and abi.entries == C.addressof(entries) and abi.stamps == C.addressof(stamps)
    assert (entries[0].volume, entries[0].first_stamp, entries[0].num_stamps, entries[1].first_stamp, entries[1].num_stamps) == (1, 0, 2, 2, 1)
    assert list(entries[0].region_lo) == [1, 2, 3] and list(entries[0].region_whd) == [4, 5, 6] and list(entries[0].step) == [1, 2, 4]
    assert list(entries[1].step) == [1, 1, 1] and list(entries[0].origin) == [0.5, 0.25, 0.125]
    assert bytes(stamps[0])[:84] == bytes(a.brush) and (stamps[0].op, stamps[0].blend, stamps[2].op) == (S.SUBTRACT, 0.25, S.UNION)
    assert edit.payload_bytes() == 3 * 80 and vpt.SculptEdit().empty() and vpt.SculptEdit().payload_bytes() == 0
    empty, _ = vpt.SculptEdit().to_abi()
    assert (empty.num_entries, empty.entries, empty.num_stamps, empty.stamps) == (0, None, 0, None)


def test_new_names_are_exported(vpt):
    for name in ("Stamp", "SculptEntry", "SculptEdit", "VptSculptStamp", "VptSculptEntry", "VptSculptEdit", "SCULPT_REPLACE", "SCULPT_UNION",
                 "SCULPT_SUBTRACT", "SCULPT_INTERSECT", "SCULPT_RECORD_BYTES"):
        assert hasattr(vpt, name), name
    for cls, method in ((vpt.HostScene, "sculpt_volume"), (vpt.HostScene, "update_sculpts"), (vpt.DeviceScene, "sculpt_volumes"),
                        (vpt.MultiDeviceScene, "sculpt_volumes"), (vpt.RenderSession, "edit_sculpts"), (vpt.RenderSession, "sculpt_at")):
        assert callable(getattr(cls, method)), method
