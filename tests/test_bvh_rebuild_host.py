"""The host side of vpt_scene_rebuild_bvh: HostScene.rebuild_bvh(), the mirror of the reference's make_bvh run again
on an edited scene, pinned to the reference's own statistics (tests/golden/rebuild_stats.json, made by
tests/golden/make_rebuild_fixtures.py) and to a load of the edited scene written out; the ABI struct; the argument checks that
need no device."""
import ctypes as C
import json
import os
import sys

import pytest

import rebuild_edits as R
from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
KEEP = ("positions", "pos_fnv", "bvh_nodes", "bvh_nodes_fnv", "bvh_prims_fnv")


def fixtures():
    return json.load(open(os.path.join(GOLDEN, "rebuild_stats.json")))


def part(stats):
    return {"scene_bvh": stats["scene_bvh"], "shapes": [{k: s[k] for k in KEEP} for s in stats["shapes"]]}


def test_the_reference_fixtures_are_there():
    assert set(fixtures()) == set(R.CASES)
    assert sum("stats" in f for f in fixtures().values()) >= 5   # the 03_volume and the chain cases at least


@pytest.mark.parametrize("name", list(R.CASES))
def test_rebuild_against_the_refit_the_reference_and_a_fresh_load(vpt, tmp_path, name):
    from make_update_fixtures import write_edited_scene
    case = R.CASES[name]
    source = case.path(tmp_path / "source")
    h = vpt.HostScene(source)
    refitted = []
    R.apply(h, case, refitted=refitted)
    # the case is a case: the rebuilt integer fields (start, num, axis, internal, counts, primitive orders) differ from the refitted tree's
    assert refitted[0] != R.integer_fields(h), f"{name}: the rebuild gives the refitted tree's topology - replace the edit"
    # the mirror pinned to the reference's own make_bvh of the edited scene
    fixture = fixtures()[name]
    if "stats" in fixture:
        assert part(json.loads(h.stats())) == fixture["stats"]
    else:
        print(f"{name}: not pinned to the reference: {fixture['refused']}")
    # and to this library's loader: the written edited scene, loaded afresh
    fresh = vpt.HostScene(write_edited_scene(vpt, source, h, str(tmp_path / "written")))
    for a, b in zip(h.bvh_nodes() + h.bvh_prims(), fresh.bvh_nodes() + fresh.bvh_prims()):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("scene_file", [R.S03, R.CURVES])
def test_a_rebuild_of_an_unedited_scene_reproduces_its_bvh(vpt, scene_file):
    h = vpt.HostScene(os.path.join(R.SCENES, scene_file))
    before, fields = h.stats(), R.integer_fields(h)
    assert h.rebuild_bvh().shapes == () and h.stats() == before            # the scene level alone
    what = h.rebuild_bvh("all")
    assert what.shapes == tuple(range(h.count("shapes"))) and what.scene
    assert h.stats() == before and R.integer_fields(h) == fields
    assert h.rebuild_bvh([1], scene=False).scene is False and h.stats() == before


def test_rebuild_wants_the_pending_edit_handed_out_and_good_ids(vpt):
    import scene_edits as E
    h = vpt.HostScene(os.path.join(R.SCENES, R.S03))
    E.translate(h, h.count("instances") - 1, dy=0.05)   # a refit of this edit keeps a topology a fresh build does not give
    with pytest.raises(vpt.VptError):
        h.rebuild_bvh()
    h.update_bvh()
    before = h.stats()
    for bad in ([h.count("shapes")], [-1], [0, 0]):
        with pytest.raises(vpt.VptError):
            h.rebuild_bvh(bad)
    assert h.stats() == before
    h.rebuild_bvh()
    assert h.stats() != before


def test_bvh_rebuild_packs_the_abi_struct(vpt):
    assert C.sizeof(vpt.VptBvhRebuild) == 24
    abi, keep = vpt.BvhRebuild((3, 1), True).to_abi()
    assert (abi.num_shapes, abi.scene) == (2, 1) and [abi.shape_ids[0], abi.shape_ids[1]] == [3, 1]
    abi, keep = vpt.BvhRebuild((), False).to_abi()
    assert (abi.num_shapes, abi.scene) == (0, 0) and not abi.shape_ids
    assert vpt.BvhRebuild((), False).empty() and not vpt.BvhRebuild((), True).empty() and not vpt.BvhRebuild((0,), False).empty()


def test_abi_argument_checks(vpt):
    what = vpt.VptBvhRebuild(0, None, 1)
    assert vpt.hip.vpt_scene_rebuild_bvh(None, C.byref(what)) == -1 and b"null" in vpt.hip.vpt_last_error()
    assert vpt.hip.vpt_scene_rebuild_bvh(None, None) == -1
    assert vpt.hip.vpt_multi_rebuild_bvh(None, C.byref(what)) == -1 and b"null" in vpt.hip.vpt_last_error()
    assert vpt.hip.vpt_session_rebuild_bvh(None, C.byref(what)) == -1
    a, b = C.c_int32(0), C.c_int64(0)
    assert vpt.hip.vpt_scene_get_bvh_counts(None, C.byref(a), C.byref(b), None) == -1
    assert vpt.hip.vpt_scene_get_bvh_prims(None, None, 0, None, 0) == -1
