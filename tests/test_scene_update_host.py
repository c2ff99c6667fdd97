"""The host side of scene editing: HostScene's setters and update_bvh(), the mirror of the reference's
update_bvh(bvh, scene, updated_instances, updated_shapes) - a refit that keeps topology and primitive order - and the argument
checks of vpt_scene_update that need no device."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import scene_edits as E
from conftest import GOLDEN, ROOT

F = np.float32
S03 = "03_volume/volume.json"
CURVES = "09_curves_synth/curves.json"
HEAD = "05_head1ss_sub/head1ss_sub.json"
SURF = "01_surface_min/surface_min.json"
REF_KEYS = ("positions", "normals", "texcoords", "colors", "triangles", "quads", "pos_fnv", "nrm_fnv", "uv_fnv", "tri_fnv", "quad_fnv",
            "bvh_nodes", "bvh_nodes_fnv", "bvh_prims_fnv")


def path(scene_file):
    return os.path.join(GOLDEN, "scenes", scene_file)


def reference_stats(scene_file):
    if scene_file == S03:
        return json.load(open(os.path.join(GOLDEN, "03_volume_stats.json")))
    if scene_file == CURVES:
        return json.load(open(os.path.join(GOLDEN, "curves_stats.json")))["curves"]
    return json.load(open(os.path.join(GOLDEN, "substitute_stats.json")))[scene_file]


def bvh_part(stats):
    return {"scene_bvh": stats["scene_bvh"], "shapes": [{k: s[k] for k in ("bvh_nodes", "bvh_nodes_fnv", "bvh_prims_fnv", "pos_fnv")} for s in stats["shapes"]]}


@pytest.mark.parametrize("scene_file", [S03, CURVES, HEAD, SURF])
def test_refit_of_an_unedited_scene_is_the_references_build(vpt, scene_file):
    """update_bvh over ALL shapes and instances of an unedited scene leaves every box as make_bvh made it: the statistics stay the
    reference's own (committed hashes of its nodes and primitive orders)"""
    h = vpt.HostScene(path(scene_file))
    before = h.stats()
    assert h.update_bvh().empty() and h.stats() == before   # nothing edited: the scene BVH alone is refitted
    for s in range(h.count("shapes")):
        h.set_shape_positions(s, h.shape_positions(s))
    for i in range(h.count("instances")):
        h.set_instance_frame(i, h.instance_frame(i))
    edit = h.update_bvh()
    assert len(edit.shapes) == h.count("shapes") and len(edit.instances) == h.count("instances")
    assert h.stats() == before
    assert bvh_part(json.loads(h.stats())) == bvh_part(reference_stats(scene_file))


def test_setters_read_back_and_reach_the_descriptor(vpt):
    h = vpt.HostScene(path(S03))
    E.edit_camera(h)
    E.edit_material(h, E.first_plain_material(h))
    E.rotate_environment(h, 0, 0.3)
    E.translate(h, 2, dy=0.25)
    p = E.nudge(h.shape_positions(1))
    h.set_shape_positions(1, p, -h.shape_normals(1))
    cam = h.camera(0)
    assert abs(cam.aperture - 0.01) < 1e-9 and abs(cam.focus - 1.5) < 1e-9
    assert np.array_equal(h.shape_positions(1), p)
    edit = h.update_bvh()
    assert set(edit.cameras) == {0} and set(edit.instances) == {2} and set(edit.environments) == {0} and len(edit.materials) == 1 and set(edit.shapes) == {1}
    assert edit.shapes[1][1] is not None and np.array_equal(edit.shapes[1][0], p)
    assert h.update_bvh().empty()
    with pytest.raises(vpt.VptError):
        h.set_shape_positions(1, p[:-1])   # counts cannot change
    with pytest.raises(vpt.VptError):
        h.set_instance_frame(h.count("instances"), np.zeros(12, np.float32))


# ---- a numpy replay of the refit rule (include/vpt.h) for the scene BVH -----------------------------------------------------------
def sel_min(a, b):
    return a if a < b else b   # the reference's select form: not np.minimum (signed zeros, order)


def sel_max(a, b):
    return a if a > b else b


FLT_MAX = F(3.402823466e+38)


def merge(box, lo, hi):
    return ([sel_min(box[0][k], lo[k]) for k in range(3)], [sel_max(box[1][k], hi[k]) for k in range(3)])


def replay_scene_refit(vpt, h):
    """the scene BVH's nodes after a refit, from the descriptor's instance frames, shape root boxes, primitive order and topology"""
    d = vpt.VptSceneDescBvh.from_address(h.desc + vpt.VptSceneDescBvh.OFFSET)
    nodes, shape_nodes = h.bvh_nodes()
    prims = np.ctypeslib.as_array(C.cast(d.scene_bvh_prims, C.POINTER(C.c_int32)), (d.num_scene_bvh_prims,)).copy()
    # the root node of every shape: the descriptor's shapes are laid out one after the other in the pool
    roots, offset = [], 0
    stats = json.loads(h.stats())
    for s in stats["shapes"]:
        roots.append(shape_nodes[offset] if s["bvh_nodes"] else None)
        offset += s["bvh_nodes"]
    boxes = []
    for i in range(h.count("instances")):
        f = h.instance_frame(i)
        root = roots[h.instance_ids(i)[0]]
        box = ([FLT_MAX] * 3, [-FLT_MAX] * 3)
        if root is not None:
            for cx in range(2):
                for cy in range(2):
                    for cz in range(2):
                        p = [F(root["bbox_max"][0] if cx else root["bbox_min"][0]), F(root["bbox_max"][1] if cy else root["bbox_min"][1]),
                             F(root["bbox_max"][2] if cz else root["bbox_min"][2])]
                        w = [F(F(F(F(f[k] * p[0]) + F(f[3 + k] * p[1])) + F(f[6 + k] * p[2])) + f[9 + k]) for k in range(3)]
                        box = merge(box, w, w)
        boxes.append(box)
    out = nodes.copy()
    for n in range(len(out) - 1, -1, -1):
        box = ([FLT_MAX] * 3, [-FLT_MAX] * 3)
        if out[n]["internal"]:
            for c in (out[n]["start"], out[n]["start"] + 1):
                box = merge(box, [F(x) for x in out[c]["bbox_min"]], [F(x) for x in out[c]["bbox_max"]])
        else:
            for k in range(out[n]["num"]):
                b = boxes[prims[out[n]["start"] + k]]
                box = merge(box, b[0], b[1])
        out[n]["bbox_min"], out[n]["bbox_max"] = box
    return out


def edited_scene_file(tmp_path, scene_file, frames):
    """the scene file with the instances' frames replaced ({instance: 12 floats})"""
    def change(d):
        for i, f in frames.items():
            d["instances"][i]["frame"] = [float(x) for x in f]
    return E.write_scene_variant(tmp_path, path(scene_file), change)


NON_PINNED = {  # a rebuild of the edited scene has another topology: nothing of the reference's to compare the boxes with
    "light_rotation": lambda h: E.rotate_instance(h, E.light_instances(h)[0], 0.4),
    "last_y005": lambda h: E.translate(h, h.count("instances") - 1, dy=0.05),
}


@pytest.mark.parametrize("name", list(NON_PINNED))
def test_refit_rule_and_closest_hits_on_edits_that_change_the_topology(vpt, oracle, tmp_path, name):
    h = vpt.HostScene(path(S03))
    topology = [h.bvh_nodes()[0][k].copy() for k in ("start", "num", "axis", "internal")]
    NON_PINNED[name](h)
    edit = h.update_bvh()
    nodes = h.bvh_nodes()[0]
    assert all(np.array_equal(nodes[k], t) for k, t in zip(("start", "num", "axis", "internal"), topology))
    assert replay_scene_refit(vpt, h).tobytes() == nodes.tobytes()
    # closest hits: the refitted tree finds what a tree rebuilt for the edited scene finds
    rebuilt = vpt.HostScene(edited_scene_file(tmp_path, S03, edit.instances))
    assert all(np.array_equal(rebuilt.instance_frame(i), f) for i, f in edit.instances.items())
    rng = np.random.default_rng(5)
    n = 4096
    o = rng.uniform((-0.9, -0.05, -0.6), (0.9, 0.9, 0.6), size=(n, 3))
    t = rng.uniform((-0.6, 0.0, -0.4), (0.6, 0.5, 0.4), size=(n, 3))
    d = t - o
    rays = np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], axis=1).astype(np.float32)
    ia, ua = oracle.oracle_intersect(h, rays)
    ib, ub = oracle.oracle_intersect(rebuilt, rays)
    assert (ia[:, 0] >= 0).mean() > 0.5
    differ = (ia != ib).any(axis=1) | (ua.view(np.uint32) != ub.view(np.uint32)).any(axis=1)
    tied = differ & (ua[:, 2] == ub[:, 2]) & (ia[:, 0] >= 0) & (ib[:, 0] >= 0)
    print(f"{name}: {int(differ.sum())} rays differ, {int(tied.sum())} of them tied in distance")
    assert not (differ & ~tied).any()
    assert tied.mean() < 0.01


# ---- pinned to the reference itself: tests/golden/update_stats.json (tests/golden/make_update_fixtures.py) ------------------------
def pinned_cases():
    f = os.path.join(GOLDEN, "update_stats.json")
    return json.load(open(f)) if os.path.exists(f) else {}


def test_the_reference_fixtures_are_there():
    assert set(E.PINNED) == set(pinned_cases())


@pytest.mark.parametrize("name", sorted(pinned_cases()))
def test_refit_equals_the_references_build_of_the_edited_scene(vpt, name):
    """Where a fresh make_bvh of the edited scene has the original's topology, the refitted boxes are the rebuilt ones bit for bit:
    the REFERENCE's statistics of the edited scene (its own loader, its own make_bvh) against the mirror's after setters + update_bvh()"""
    case = pinned_cases()[name]
    scene_file, edit = E.PINNED[name]
    h = vpt.HostScene(path(scene_file))
    edit(h)
    h.update_bvh()
    mine = json.loads(h.stats())
    assert [s["pos_fnv"] for s in mine["shapes"]] == [s["pos_fnv"] for s in case["stats"]["shapes"]], "the edit's formula drifted from the fixture's"
    assert bvh_part(mine) == bvh_part(case["stats"])


# ---- argument checks that need no device ----------------------------------------------------------------------------------------
def test_abi_argument_checks(vpt):
    edit = vpt.VptSceneEdit()
    assert vpt.hip.vpt_scene_update(None, C.byref(edit)) == -1 and b"null" in vpt.hip.vpt_last_error()
    assert vpt.hip.vpt_scene_update(None, None) == -1
    assert vpt.hip.vpt_multi_update(None, C.byref(edit)) == -1 and b"null" in vpt.hip.vpt_last_error()
    assert vpt.hip.vpt_scene_get_bvh(None, None, 0, None, 0) == -1
    n, b, ms = C.c_int(0), C.c_int64(0), C.c_float(0)
    assert vpt.hip.vpt_scene_update_stats(None, C.byref(n), C.byref(b), C.byref(ms)) == -1


def test_scene_edit_packs_the_abi_struct(vpt):
    """SceneEdit.to_abi: counts, ids and payloads where vpt_scene_edit wants them (the struct's layout is include/vpt.h's)"""
    assert C.sizeof(vpt.VptSceneEdit) == 4 * 24 + 32 and C.sizeof(vpt.VptCamera) == 72 and C.sizeof(vpt.VptMaterial) == 84
    h = vpt.HostScene(path(S03))
    p = h.shape_positions(1)
    e = vpt.SceneEdit(cameras={0: h.camera(0)}, instances={3: h.instance_frame(3), 1: h.instance_frame(1)}, shapes={1: (p, None)})
    abi, keep = e.to_abi()
    assert (abi.num_cameras, abi.num_instances, abi.num_environments, abi.num_materials, abi.num_shapes) == (1, 2, 0, 0, 1)
    ids = np.ctypeslib.as_array(C.cast(abi.instance_ids, C.POINTER(C.c_int32)), (2,))
    frames = np.ctypeslib.as_array(C.cast(abi.instance_frames, C.POINTER(C.c_float)), (2, 12))
    assert list(ids) == [3, 1] and np.array_equal(frames[0], h.instance_frame(3)) and np.array_equal(frames[1], h.instance_frame(1))
    pos = C.cast(abi.shape_positions, C.POINTER(C.c_void_p))[0]
    assert np.array_equal(np.ctypeslib.as_array(C.cast(pos, C.POINTER(C.c_float)), p.shape), p)
    assert C.cast(abi.shape_normals, C.POINTER(C.c_void_p))[0] is None
    merged = e.merge(vpt.SceneEdit(instances={1: np.zeros(12, np.float32)}, shapes={1: (p * 2, None)}))
    assert set(merged.instances) == {1, 3} and not merged.instances[1].any() and np.array_equal(merged.shapes[1][0], p * 2)


# ---- ypathtrace --cameras: the errors that come before a device is needed -------------------------------------------------------
BIN = os.path.join(ROOT, "volumetric-path-tracer_amd", "ypathtrace")


def test_cli_cameras_errors(tmp_path):
    bad = tmp_path / "bad.json"
    for text in ("[{\"lens\": 0.05}", "{}", "[]", "[3]"):
        bad.write_text(text)
        r = subprocess.run([BIN, "--scene", path(S03), "--cameras", str(bad)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 1 and r.stderr.startswith(f"error: {bad}: parse error"), (text, r.stderr[:200])
    r = subprocess.run([BIN, "--scene", path(S03), "--cameras"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and r.stderr.startswith("error: missing value for cameras")
    r = subprocess.run([BIN, "--scene", path(S03), "--cameras", str(tmp_path / "none.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "none.json" in r.stderr
