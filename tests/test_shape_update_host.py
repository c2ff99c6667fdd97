"""The host side of vpt_scene_update_shapes: HostScene.add_shape / set_shape / remove_shapes / update_shapes, the
mirror of scene.shapes replace / erase / push_back with the instances renumbered, make_bvh of the new shapes and make_lights on the
edited scene, pinned to the reference's own statistics (tests/golden/shape_edit_stats.json, made by
tests/golden/make_shape_edit_fixtures.py) and to a load of the edited scene written out; a numpy replay of the renumbering and the
pool offsets; the order of application; the setters' errors and the pending-edit exclusions; the ABI structs; the refusals that
need no device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import instance_edits as I
import shape_edits as S
from conftest import GOLDEN

KEEP = ("positions", "pos_fnv", "bvh_nodes", "bvh_nodes_fnv", "bvh_prims_fnv")
TRIANGLE = dict(positions=np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), triangles=[[0, 1, 2]])


def fixtures():
    return json.load(open(os.path.join(GOLDEN, "shape_edit_stats.json")))


def part(stats):
    return {"scene_bvh": stats["scene_bvh"], "shapes": [{k: s[k] for k in KEEP} for s in stats["shapes"]], "lights": stats["lights"]}


def test_the_reference_fixtures_are_there():
    f = fixtures()
    assert set(f) == set(S.CASES)
    assert all("stats" in v for v in f.values()), "no case may be refused"


@pytest.mark.parametrize("name", list(S.ALL_CASES))
def test_the_mirror_against_the_reference_and_a_fresh_load(vpt, tmp_path, name):
    case = S.ALL_CASES[name]
    source = case.path(tmp_path / "source")
    h, names = vpt.HostScene(source), S.shape_names(source)
    before, edits = S.shape_fields(h), []
    S.apply(h, case, after_shapes=edits.append, names=names)
    assert edits and all(not e.empty() for e in edits)
    if name in S.ROUND_TRIPS:
        original = vpt.HostScene(source)
        assert h.stats() == original.stats() and h.bvh_nodes()[1].tobytes() == original.bvh_nodes()[1].tobytes()
    else:   # the case is a case: integer fields, node count or primitive order of the pooled shape BVHs change
        assert S.shape_fields(h) != before, f"{name}: the edit leaves the shape BVHs as they were - replace the edit"
    if name not in S.CASES:   # an empty shape: no loader takes a shape file without elements, so there is no file to load it from
        empty = h.count("shapes") - 1
        assert len(h.bvh_nodes()[1]) == len(vpt.HostScene(source).bvh_nodes()[1]) + 1 and not h.bvh_nodes()[1][-1]["internal"] and h.bvh_nodes()[1][-1]["num"] == 0
        assert desc_shapes(h)[empty]["num_bvh_nodes"] == 1 and len(h.bvh_prims()[1]) == len(vpt.HostScene(source).bvh_prims()[1])
        return
    # the mirror pinned to the reference's own make_bvh and make_lights of the edited scene
    assert part(json.loads(h.stats())) == fixtures()[name]["stats"]
    # and to this library's loader: the written edited scene, loaded afresh
    fresh = vpt.HostScene(S.write_edited_scene(source, h, names, str(tmp_path / "written")))
    assert h.stats() == fresh.stats()
    assert I.instances_of(h).tobytes() == I.instances_of(fresh).tobytes()
    for a, b in zip(h.bvh_nodes() + h.bvh_prims() + h.lights(), fresh.bvh_nodes() + fresh.bvh_prims() + fresh.lights()):
        assert a.tobytes() == b.tobytes()
    for s in range(h.count("shapes")):
        a, b = h.shape_arrays(s), fresh.shape_arrays(s)
        assert all(a[k].tobytes() == b[k].tobytes() for k in a), (name, s)


SHAPE = np.dtype([(k, np.int32) for k in ("num_vertices", "position_offset", "normal_offset", "texcoord_offset", "color_offset", "num_triangles",
                                          "triangle_offset", "num_quads", "quad_offset", "num_bvh_nodes", "bvh_node_offset", "bvh_prim_offset")])   # vpt_shape


def desc_shapes(h):
    """the shape table of the flattened descriptor: its third {int32 count, pointer} pair"""
    count = C.c_int32.from_address(h.desc + 2 * 16).value
    table = C.c_void_p.from_address(h.desc + 2 * 16 + 8).value
    return np.ctypeslib.as_array(C.cast(table, C.POINTER(C.c_int32)), (count, 12)).copy().view(SHAPE).reshape(count)


def sizes_of(h):
    """per shape: vertices, entries of the normal / texcoord / colour pools, elements, BVH nodes"""
    out = []
    for s in range(h.count("shapes")):
        a = h.shape_arrays(s)
        out.append([len(a["positions"]), len(a["normals"]), len(a["texcoords"]), len(a["colors"]), max(len(a[k]) for k in ("triangles", "quads", "points", "lines"))])
    return np.array(out, np.int64).reshape(-1, 5)


def replay(sizes, inst_shape, edit, new_sizes):
    """the rule of include/vpt.h in numpy: set on current ids, keep flags and their exclusive scan, survivors gathered, adds appended;
    every instance's shape through the map; per pool the exclusive prefix sums of the new list"""
    out = sizes.copy()
    for i in edit.set:
        out[i] = new_sizes(edit.set[i])
    keep = np.ones(len(out), np.int64)
    keep[list(edit.remove)] = 0
    new_id = np.cumsum(keep) - keep
    new_of_old = np.where(keep == 1, new_id, -1)
    out = np.concatenate([out[keep == 1], np.array([new_sizes(m) for m in edit.add], np.int64).reshape(-1, 5)])
    offsets = np.cumsum(out, axis=0) - out
    return out, offsets, new_of_old[inst_shape]


def mesh_sizes(m):
    n = lambda k: 0 if m[k] is None else len(m[k])
    return [n("positions"), n("normals"), n("texcoords"), n("colors"), max(n(k) for k in ("triangles", "quads", "points", "lines"))]


@pytest.mark.parametrize("name", ["remove_first", "all_three", "grid_shrink_flip", "add_two"])
def test_a_numpy_replay_of_the_renumbering_and_the_pool_offsets(vpt, tmp_path, name):
    case = S.CASES[name]
    h = vpt.HostScene(case.path(tmp_path))
    for kind, step in case.steps:
        sizes, inst_shape = sizes_of(h), np.array([h.instance_ids(i)[0] for i in range(h.count("instances"))], np.int64)
        step(h)
        if kind == "instances":
            h.update_instances()
            continue
        edit = h.update_shapes()
        want, offsets, want_shapes = replay(sizes, inst_shape, edit, mesh_sizes)
        assert np.array_equal(sizes_of(h), want)
        assert np.array_equal([h.instance_ids(i)[0] for i in range(h.count("instances"))], want_shapes) and (want_shapes >= 0).all()
        # the flattened descriptor lays the pools out in shape order: the offsets are the prefix sums (-1: the shape has no such attribute)
        d = desc_shapes(h)
        assert np.array_equal(d["num_vertices"], want[:, 0]) and np.array_equal(d["position_offset"], offsets[:, 0])
        for k, key in ((1, "normal_offset"), (2, "texcoord_offset"), (3, "color_offset")):
            assert np.array_equal(d[key], np.where(want[:, k] > 0, offsets[:, k], -1)), key
        assert np.array_equal(np.maximum(d["num_triangles"], d["num_quads"]), np.where(d["num_triangles"] + d["num_quads"] > 0, want[:, 4], 0))
        assert np.array_equal(d["bvh_prim_offset"], offsets[:, 4]) and np.array_equal(d["bvh_node_offset"], np.cumsum(d["num_bvh_nodes"]) - d["num_bvh_nodes"])


def test_order_of_application(vpt, tmp_path):
    """set names current ids, removal names current ids, an added shape comes after the survivors: add_shape returns its id"""
    h = vpt.HostScene(S.CASES["remove_first"].path(tmp_path))
    h.remove_instances(S.instances_of_shape(h, S.QUAD_LEAF))
    h.update_instances()
    was = [h.shape_arrays(s)["positions"].tobytes() for s in range(7)]
    blob_instances = S.instances_of_shape(h, S.BLOB)
    h.set_shape(S.GRID_TRIS, **S.blob(9))
    h.remove_shapes([S.QUAD_LEAF])
    new = h.add_shape(**TRIANGLE)
    assert new == 6
    edit = h.update_shapes()
    assert edit.remove == (S.QUAD_LEAF,) and list(edit.set) == [S.GRID_TRIS] and len(edit.add) == 1 and h.count("shapes") == 7
    now = [h.shape_arrays(s)["positions"].tobytes() for s in range(7)]
    assert now[0] == was[0] and now[1:3] == was[2:4] and now[4:6] == was[5:7]          # survivors keep their order, ids close up
    assert now[3] == S.blob(9)["positions"].tobytes() and now[6] == TRIANGLE["positions"].tobytes()
    assert S.instances_of_shape(h, S.BLOB - 1) == blob_instances                         # the instances follow the renumbering


def test_setter_errors_and_the_pending_edit_exclusions(vpt, tmp_path):
    import scene_edits as E
    h = vpt.HostScene(S.CASES["remove_first"].path(tmp_path))
    n, before = h.count("shapes"), h.stats()
    P = TRIANGLE["positions"]
    nan = P.copy()
    nan[1, 1] = np.nan
    for bad in (lambda: h.add_shape(P, triangles=[[0, 1, 3]]), lambda: h.add_shape(P, triangles=[[0, 1, 2]], quads=[[0, 1, 2, 2]]),
                lambda: h.add_shape(P, points=[0, 1]), lambda: h.add_shape(P, lines=[[0, 1]], triangles=[[0, 1, 2]], radius=[1, 1, 1]),
                lambda: h.add_shape(nan, triangles=[[0, 1, 2]]), lambda: h.add_shape(P, triangles=[[0, 1, 2]], normals=P[:2]),
                lambda: h.set_shape(n, **TRIANGLE), lambda: h.set_shape(-1, **TRIANGLE), lambda: h.remove_shapes([n]),
                lambda: h.remove_shapes([S.BLOB])):                                      # instances still name it
        with pytest.raises(vpt.VptError):
            bad()
    assert h.update_shapes().empty() and h.stats() == before
    h.set_shape(3, **TRIANGLE)
    with pytest.raises(vpt.VptError):
        h.remove_shapes([3])                                                             # set and removed
    # no frame, vertex or instance change and no rebuild may begin while shape changes are pending
    for bad in (lambda: E.translate(h, 1, dx=0.1), lambda: h.set_shape_positions(0, h.shape_positions(0)), lambda: h.rebuild_bvh(),
                lambda: h.add_instance(I.frame(), 0, 0), lambda: h.remove_instances([0]), lambda: h.set_instance(0, material=1), h.update_instances):
        with pytest.raises(vpt.VptError):
            bad()
    assert list(h.update_shapes().set) == [3]
    # and the reverse: shape changes may not begin while a frame edit or instance changes are pending
    E.translate(h, 1, dx=0.1)
    for bad in (lambda: h.add_shape(**TRIANGLE), lambda: h.set_shape(0, **TRIANGLE), lambda: h.remove_shapes([0]), h.update_shapes):
        with pytest.raises(vpt.VptError):
            bad()
    h.update_bvh()
    h.add_instance(I.frame(), 0, 0)
    for bad in (lambda: h.add_shape(**TRIANGLE), h.update_shapes):
        with pytest.raises(vpt.VptError):
            bad()
    h.update_instances()
    assert h.add_shape(**TRIANGLE) == n and len(h.update_shapes().add) == 1 and h.count("shapes") == n + 1


def test_shape_edit_packs_the_abi_structs(vpt):
    assert C.sizeof(vpt.VptShapeData) == 112 and C.sizeof(vpt.VptShapeEdit) == 56
    assert [vpt.VptShapeData.positions.offset, vpt.VptShapeData.radius.offset, vpt.VptShapeData.num_triangles.offset, vpt.VptShapeData.lines.offset] == [8, 40, 48, 104]
    m = dict(S.with_attributes(S.grid(2)), colors=np.ones((9, 4), np.float32))
    abi, keep = vpt.ShapeEdit((4, 2), {5: m}, [TRIANGLE, S.points(3)]).to_abi()
    assert (abi.num_remove, abi.num_set, abi.num_add) == (2, 1, 2)
    assert list(np.ctypeslib.as_array(C.cast(abi.remove_ids, C.POINTER(C.c_int32)), (2,))) == [4, 2]
    assert C.cast(abi.set_ids, C.POINTER(C.c_int32))[0] == 5
    rec = C.cast(abi.set, C.POINTER(vpt.VptShapeData))[0]
    assert (rec.num_vertices, rec.num_quads, rec.num_triangles, rec.num_points, rec.num_lines) == (9, 4, 0, 0, 0) and not rec.triangles and not rec.radius
    assert np.ctypeslib.as_array(C.cast(rec.positions, C.POINTER(C.c_float)), (27,)).tobytes() == m["positions"].tobytes()
    assert np.ctypeslib.as_array(C.cast(rec.quads, C.POINTER(C.c_int32)), (16,)).tobytes() == m["quads"].tobytes()
    assert rec.normals and rec.texcoords and rec.colors
    add = C.cast(abi.add, C.POINTER(vpt.VptShapeData))
    assert (add[0].num_triangles, add[1].num_points, add[1].num_vertices) == (1, 3, 3) and add[1].radius and not add[0].normals
    abi, keep = vpt.ShapeEdit().to_abi()
    assert (abi.num_remove, abi.num_set, abi.num_add) == (0, 0, 0) and not abi.remove_ids and not abi.set and not abi.add
    assert vpt.ShapeEdit().empty() and not vpt.ShapeEdit((0,)).empty() and not vpt.ShapeEdit(add=[TRIANGLE]).empty()


def test_abi_argument_checks(vpt):
    """every entry point refuses a null handle or edit before it touches a device"""
    edit = vpt.VptShapeEdit()
    assert vpt.hip.vpt_scene_update_shapes(None, C.byref(edit)) == -1 and b"null" in vpt.hip.vpt_last_error()
    assert vpt.hip.vpt_scene_update_shapes(None, None) == -1
    assert vpt.hip.vpt_multi_update_shapes(None, C.byref(edit)) == -1 and b"null" in vpt.hip.vpt_last_error()
    assert vpt.hip.vpt_session_edit_shapes(None, C.byref(edit)) == -1
    assert vpt.hip.vpt_scene_shape_tables_hash(None, None) == -1
    assert vpt.hip.vpt_scene_get_shape_counts(None, None, None, None) == -1


def test_the_host_library_refuses_what_the_device_refuses(vpt, tmp_path):
    """vpth_scene_edit_shapes called past the setters: ids, a shape still instanced, bad meshes, null lists - the scene stays"""
    h = vpt.HostScene(S.CASES["remove_first"].path(tmp_path))
    before, n = h.stats(), h.count("shapes")
    P = TRIANGLE["positions"]
    both = dict(TRIANGLE, quads=[[0, 1, 2, 2]])
    for edit in (vpt.ShapeEdit((n,)), vpt.ShapeEdit((-1,)), vpt.ShapeEdit(set={n: TRIANGLE}), vpt.ShapeEdit((S.BLOB,)),
                 vpt.ShapeEdit(add=[dict(positions=P, triangles=[[0, 1, 3]])]), vpt.ShapeEdit(add=[both]), vpt.ShapeEdit(add=[dict(positions=P, points=[0])]),
                 vpt.ShapeEdit(add=[dict(positions=P, lines=[[0, 1]], triangles=[[0, 1, 2]], radius=[1, 1, 1])]),
                 vpt.ShapeEdit(add=[dict(positions=[[0, 0, np.inf], [1, 0, 0], [0, 1, 0]], triangles=[[0, 1, 2]])])):
        abi, keep = edit.to_abi()
        err = C.create_string_buffer(512)
        assert vpt.host.vpth_scene_edit_shapes(h.handle, abi.remove_ids, abi.num_remove, abi.set_ids, abi.set, abi.num_set, abi.add, abi.num_add, err, len(err)) == -1
        assert err.value and h.stats() == before
    ids = np.array([1, 1], np.int32)
    err = C.create_string_buffer(512)
    assert vpt.host.vpth_scene_edit_shapes(h.handle, ids.ctypes.data, 2, None, None, 0, None, 0, err, len(err)) == -1 and b"repeated" in err.value
    assert vpt.host.vpth_scene_edit_shapes(h.handle, None, 2, None, None, 0, None, 0, err, len(err)) == -1 and b"null" in err.value
    assert h.stats() == before
