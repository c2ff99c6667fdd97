"""The host side of vpt_scene_update_instances: HostScene.add_instance / remove_instances / set_instance /
update_instances, the mirror of scene.instances.erase + push_back, make_bvh's scene level and make_lights on the edited scene, pinned
to the reference's own statistics (tests/golden/instance_edit_stats.json, made by tests/golden/make_instance_edit_fixtures.py) and
to a load of the edited scene written out; the setters' errors and the pending-edit exclusions; the ABI struct; a numpy replay of
the renumbering; the refusals that need no device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import instance_edits as I
from conftest import GOLDEN

KEEP = ("positions", "pos_fnv", "bvh_nodes", "bvh_nodes_fnv", "bvh_prims_fnv")


def fixtures():
    return json.load(open(os.path.join(GOLDEN, "instance_edit_stats.json")))


def part(stats):
    return {"scene_bvh": stats["scene_bvh"], "shapes": [{k: s[k] for k in KEEP} for s in stats["shapes"]], "lights": stats["lights"]}


def test_the_reference_fixtures_are_there():
    f = fixtures()
    assert set(f) == set(I.CASES)
    assert all("stats" in v for v in f.values()), "no case may be refused"


@pytest.mark.parametrize("name", list(I.CASES))
def test_the_mirror_against_the_reference_and_a_fresh_load(vpt, tmp_path, name):
    case = I.CASES[name]
    source = case.path(tmp_path / "source")
    h = vpt.HostScene(source)
    before, edits = I.scene_fields(h), []
    I.apply(h, case, after=edits.append)
    assert all(not e.empty() for e in edits)
    if name == "round_trip":
        original = vpt.HostScene(source)
        assert h.stats() == original.stats() and I.instances_of(h).tobytes() == I.instances_of(original).tobytes()
    else:   # the case is a case: the scene BVH's integer fields, node count or primitive order change
        assert I.scene_fields(h) != before, f"{name}: the edit leaves the scene BVH's topology as it was - replace the edit"
    # the mirror pinned to the reference's own make_bvh and make_lights of the edited scene
    assert part(json.loads(h.stats())) == fixtures()[name]["stats"]
    # and to this library's loader: the written edited scene, loaded afresh
    fresh = vpt.HostScene(I.write_edited_scene(source, h, str(tmp_path / "written")))
    assert h.stats() == fresh.stats()
    assert I.instances_of(h).tobytes() == I.instances_of(fresh).tobytes()
    for a, b in zip(h.bvh_nodes() + h.bvh_prims() + h.lights(), fresh.bvh_nodes() + fresh.bvh_prims() + fresh.lights()):
        assert a.tobytes() == b.tobytes()


def replay(instances, edit):
    """the rule of include/vpt.h in numpy: set on current ids, keep flags and their exclusive scan, survivors gathered, adds appended"""
    out = instances.copy()
    for i, (frame, shape, material) in edit.set.items():
        out[i] = (frame, shape, material)
    keep = np.ones(len(out), np.int32)
    keep[list(edit.remove)] = 0
    new_id = np.cumsum(keep) - keep                       # the exclusive scan
    new_of_old = np.where(keep == 1, new_id, -1)
    gathered = np.zeros(int(keep.sum()), instances.dtype)
    gathered[new_id[keep == 1]] = out[keep == 1]
    return np.concatenate([gathered, vpt_records(instances.dtype, edit.add)]), new_of_old


def vpt_records(dtype, items):
    out = np.zeros(len(items), dtype)
    for i, item in enumerate(items):
        out[i] = item
    return out


@pytest.mark.parametrize("name", ["crowd_remove_mid", "crowd_all_three", "curves_off_on"])
def test_a_numpy_replay_of_the_renumbering(vpt, tmp_path, name):
    case = I.CASES[name]
    h = vpt.HostScene(case.path(tmp_path))
    for step in case.steps:
        was = I.instances_of(h)
        step(h)
        edit = h.update_instances()
        want, new_of_old = replay(was, edit)
        got = I.instances_of(h)
        assert got.tobytes() == want.tobytes()
        # survivors keep their relative order and the ids close up
        kept = new_of_old[new_of_old >= 0]
        assert np.array_equal(kept, np.arange(len(kept))) and len(got) == len(kept) + len(edit.add)


def test_order_of_application(vpt, tmp_path):
    """set names current ids, removal names current ids, an added instance comes after the survivors: add_instance returns its id"""
    h = vpt.HostScene(I.CASES["crowd_remove_mid"].path(tmp_path))
    was = I.instances_of(h)
    h.set_instance(10, material=I.RED, frame=I.frame(1, (0.25, 0.25, 0.25)))
    h.remove_instances([4])
    new = h.add_instance(I.frame(2), I.BLOB, I.GREY)
    assert new == 69
    h.update_instances()
    now = I.instances_of(h)
    assert len(now) == 70 and now[9]["material"] == I.RED and now[9]["shape"] == was[10]["shape"]
    assert np.array_equal(now[9]["frame"], I.frame(1, (0.25, 0.25, 0.25))) and now[69]["shape"] == I.BLOB
    assert now[:4].tobytes() == was[:4].tobytes() and now[4:9].tobytes() == was[5:10].tobytes() and now[10:69].tobytes() == was[11:].tobytes()


def test_setter_errors_and_the_pending_edit_exclusions(vpt, tmp_path):
    import scene_edits as E
    h = vpt.HostScene(I.CASES["crowd_remove_mid"].path(tmp_path))
    n, before = h.count("instances"), h.stats()
    nan = I.frame()
    nan[3] = np.inf
    for bad in (lambda: h.add_instance(I.frame(), h.count("shapes"), 0), lambda: h.add_instance(I.frame(), 0, -1), lambda: h.add_instance(nan, 0, 0),
                lambda: h.add_instance(np.zeros(11, np.float32), 0, 0), lambda: h.remove_instances([n]), lambda: h.remove_instances([2, 2]),
                lambda: h.set_instance(-1, material=0), lambda: h.set_instance(3, shape=99), lambda: h.set_instance(3, frame=nan)):
        with pytest.raises(vpt.VptError):
            bad()
    assert h.update_instances().empty() and h.stats() == before
    h.remove_instances([3])
    for bad in (lambda: h.set_instance(3, material=1), lambda: h.remove_instances([3])):   # set and removed; removed twice
        with pytest.raises(vpt.VptError):
            bad()
    h.set_instance(5, material=1)
    with pytest.raises(vpt.VptError):
        h.remove_instances([5])
    # a frame or vertex edit may not begin while instance changes are pending, nor a rebuild
    for bad in (lambda: E.translate(h, 1, dx=0.1), lambda: h.set_shape_positions(0, h.shape_positions(0)), lambda: h.rebuild_bvh()):
        with pytest.raises(vpt.VptError):
            bad()
    edit = h.update_instances()
    assert edit.remove == (3,) and list(edit.set) == [5] and h.count("instances") == n - 1
    # and the reverse: instance changes may not begin while a frame edit is pending
    E.translate(h, 1, dx=0.1)
    for bad in (lambda: h.add_instance(I.frame(), 0, 0), lambda: h.remove_instances([0]), lambda: h.set_instance(0, material=1), h.update_instances):
        with pytest.raises(vpt.VptError):
            bad()
    h.update_bvh()
    h.add_instance(I.frame(), 0, 0)
    assert h.update_instances().add and h.count("instances") == n


def test_instance_edit_packs_the_abi_struct(vpt):
    assert C.sizeof(vpt.VptInstance) == 56 and C.sizeof(vpt.VptInstanceEdit) == 56
    f = I.frame(1, (0.5, 0.25, 2), (1, 2, 3))
    abi, keep = vpt.InstanceEdit((4, 2), {7: (f, 1, 3)}, [(I.frame(), 0, 1), (f, 2, 0)]).to_abi()
    assert (abi.num_remove, abi.num_set, abi.num_add) == (2, 1, 2)
    assert list(np.ctypeslib.as_array(C.cast(abi.remove_ids, C.POINTER(C.c_int32)), (2,))) == [4, 2]
    assert C.cast(abi.set_ids, C.POINTER(C.c_int32))[0] == 7
    rec = C.cast(abi.set, C.POINTER(vpt.VptInstance))[0]
    assert (rec.shape, rec.material) == (1, 3) and list(rec.frame.x) + list(rec.frame.y) + list(rec.frame.z) + list(rec.frame.o) == list(f)
    add = C.cast(abi.add, C.POINTER(vpt.VptInstance))
    assert (add[1].shape, add[1].material, add[0].material) == (2, 0, 1) and list(add[1].frame.o) == [1, 2, 3]
    abi, keep = vpt.InstanceEdit().to_abi()
    assert (abi.num_remove, abi.num_set, abi.num_add) == (0, 0, 0) and not abi.remove_ids and not abi.set and not abi.add
    assert vpt.InstanceEdit().empty() and not vpt.InstanceEdit((0,)).empty() and not vpt.InstanceEdit(add=[(f, 0, 0)]).empty()


def test_abi_argument_checks(vpt):
    """every entry point refuses a null handle or edit before it touches a device"""
    edit = vpt.VptInstanceEdit()
    assert vpt.hip.vpt_scene_update_instances(None, C.byref(edit)) == -1 and b"null" in vpt.hip.vpt_last_error()
    assert vpt.hip.vpt_scene_update_instances(None, None) == -1
    assert vpt.hip.vpt_multi_update_instances(None, C.byref(edit)) == -1 and b"null" in vpt.hip.vpt_last_error()
    assert vpt.hip.vpt_session_edit_instances(None, C.byref(edit)) == -1
    n = C.c_int(0)
    assert vpt.hip.vpt_scene_get_instances(None, None, 0, C.byref(n)) == -1
    assert vpt.hip.vpt_scene_instance_tables_hash(None, None) == -1


def test_the_host_library_refuses_what_the_device_refuses(vpt, tmp_path):
    """vpth_scene_edit_instances called past the setters: ids, shapes, materials, null lists - the scene stays"""
    h = vpt.HostScene(I.CASES["crowd_remove_mid"].path(tmp_path))
    before, n = h.stats(), h.count("instances")
    ok = I.frame()
    for edit in (vpt.InstanceEdit((n,)), vpt.InstanceEdit((1, 1)), vpt.InstanceEdit((2,), {2: (ok, 0, 0)}), vpt.InstanceEdit(set={n: (ok, 0, 0)}),
                 vpt.InstanceEdit(add=[(ok, 7, 0)]), vpt.InstanceEdit(add=[(ok, 0, 4)]), vpt.InstanceEdit(set={0: (ok, -1, 0)})):
        abi, keep = edit.to_abi()
        err = C.create_string_buffer(512)
        assert vpt.host.vpth_scene_edit_instances(h.handle, abi.remove_ids, abi.num_remove, abi.set_ids, abi.set, abi.num_set, abi.add, abi.num_add, err, len(err)) == -1
        assert err.value and h.stats() == before
    err = C.create_string_buffer(512)
    assert vpt.host.vpth_scene_edit_instances(h.handle, None, 2, None, None, 0, None, 0, err, len(err)) == -1 and b"null" in err.value
