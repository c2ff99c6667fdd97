"""The host side of editing subdivision surfaces (include/vpt.h: vpt_scene_attach_subdiv, vpt_scene_update_subdivs): the
tesselation plan the host library exports, HostScene.set_subdiv and the pending SubdivEdit.  Equality of bits throughout, no GPU.
 1. A numpy replay of an exported plan (tests/subdiv_edits.py: replay) gives the mesh of HostScene.shape_arrays - which the reference's
    hashes pin (tests/test_tesselate.py) - for every subdiv of 08_subdiv_synth and 01_surface_min.
 2. set_subdiv with a moved cage and another displacement leaves the hashes of a fresh load of files that carry the same edit.
 3. Where the reference is built, the reference's own load + tesselate_surfaces of those files gives them too.
 4. Argument checks that need no device."""
import ctypes as C
import json

import numpy as np
import pytest

import subdiv_edits as S

F = np.float32
SUBDIVS = [(S.SYNTH, i) for i in range(4)] + [(S.SURF, i) for i in range(4)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def meshes(stats):
    """the counts and hashes of every shape's arrays; the BVH entries are left out - an edit refits the trees it has, a load builds them"""
    return [{k: v for k, v in shape.items() if not k.startswith("bvh_")} for shape in json.loads(stats)["shapes"]]


@pytest.mark.parametrize("scene_file,index", SUBDIVS)
def test_a_replay_of_the_plan_gives_the_tesselated_shape(vpt, scene_file, index):
    host = vpt.HostScene(S.path(scene_file))
    s, plan = host.subdiv(index), host.subdiv_plan(index)
    assert (plan.shape, plan.subdivisions, plan.smooth, len(plan.levels)) == (s["shape"], s["subdivisions"], s["smooth"], s["subdivisions"])
    want, got = host.shape_arrays(s["shape"]), S.replay(vpt, host, index)
    assert len(plan.verts) == len(want["positions"]) > 0
    for key in ("positions", "normals", "texcoords"):
        assert got[key].shape == want[key].shape and np.array_equal(bits(got[key]), bits(want[key])), (scene_file, index, key)
    assert np.array_equal(got["triangles"], want["triangles"]), (scene_file, index)
    # asking for the plan changed nothing of the scene
    assert host.stats() == vpt.HostScene(S.path(scene_file)).stats()


def edited(vpt, scene_file, tmp_path, moves, amounts):
    """(the mirror after set_subdiv, the file of a copy of the scene whose cages and JSON carry the same edit)"""
    host = vpt.HostScene(S.path(scene_file))
    cages = {i: S.moved(host.subdiv(i)["positions"], seed) for i, seed in moves.items()}
    for i in sorted(set(cages) | set(amounts)):
        host.set_subdiv(i, positions=cages.get(i), displacement=amounts.get(i))
    edit = host.update_subdivs()
    assert sorted(edit.subdivs) == sorted(set(cages) | set(amounts)) and not edit.empty() and host.update_subdivs().empty()
    for i, (positions, amount) in edit.subdivs.items():
        assert (positions is None) == (i not in cages) and (amount is None) == (i not in amounts)
    return host, S.write_scene(scene_file, tmp_path, cages, {i: {"displacement": a} for i, a in amounts.items()}), cages


CASES = {"synth": (S.SYNTH, {S.BOWTIE: 1, S.TETRA: 2, S.STRIP: 3, S.BALL: 4}, {S.STRIP: 0.05, S.BALL: 0.0625}),
         "synth_flat_strip": (S.SYNTH, {S.STRIP: 5}, {S.STRIP: 0.0}),
         "surface": (S.SURF, {0: 6, 1: 7, 2: 8, S.CUBE: 9}, {1: 0.03125})}


@pytest.mark.parametrize("name", list(CASES))
def test_set_subdiv_equals_a_fresh_load_of_the_edited_files(vpt, tmp_path, name):
    scene_file, moves, amounts = CASES[name]
    host, file, cages = edited(vpt, scene_file, tmp_path, moves, amounts)
    fresh = vpt.HostScene(file)
    for i, positions in cages.items():   # the files give the floats back: the comparison below compares tesselations, not parsers
        assert np.array_equal(bits(fresh.subdiv(i)["positions"]), bits(positions)), (name, i)
    for i, amount in amounts.items():
        assert F(fresh.subdiv(i)["displacement"]) == F(amount) == F(host.subdiv(i)["displacement"])
    assert meshes(host.stats()) == meshes(fresh.stats()) and json.loads(host.stats())["lights"] == json.loads(fresh.stats())["lights"]
    assert meshes(host.stats()) != meshes(vpt.HostScene(S.path(scene_file)).stats())


@pytest.mark.parametrize("name", list(CASES))
def test_set_subdiv_equals_the_reference_on_the_edited_files(vpt, tmp_path, name):
    import oracle_lib as O
    if not O.have_reference():
        pytest.skip("oracle/_ref is not built here (the committed fixtures pin the same path)")
    scene_file, moves, amounts = CASES[name]
    host, file, _ = edited(vpt, scene_file, tmp_path, moves, amounts)
    *_, ref = O.reference_render(file, "eyelight", 16, 1, 4, stats=True, workdir=str(tmp_path))
    assert meshes(host.stats()) == meshes(json.dumps(ref))


def test_levels_and_smooth_leave_as_a_shape_edit(vpt, tmp_path):
    host = vpt.HostScene(S.path(S.SYNTH))
    shape = host.subdiv(S.TETRA)["shape"]
    host.set_subdiv(S.TETRA, subdivisions=1)
    assert host.update_subdivs().empty()
    edit = host.update_shapes()
    assert list(edit.set) == [shape] and not edit.remove and not edit.add and len(edit.set[shape]["positions"]) == 14
    fresh = vpt.HostScene(S.write_scene(S.SYNTH, tmp_path, settings={S.TETRA: {"subdivisions": 1}}))
    assert json.loads(host.stats())["shapes"] == json.loads(fresh.stats())["shapes"]
    assert len(host.subdiv_plan(S.TETRA).levels) == 1   # the plan is made again
    # smooth: the tetra gains normals; and the ball's displacement switched off keeps the cage's own normals: other pools, a `set`
    host.set_subdiv(S.TETRA, smooth=True)
    ball = host.subdiv(S.BALL)
    assert len(ball["quadsnorm"]) > 0 and not ball["smooth"] and len(host.shape_normals(ball["shape"])) == 0
    host.set_subdiv(S.BALL, displacement=0.0)
    assert host.update_subdivs().empty()
    edit = host.update_shapes()
    assert sorted(edit.set) == [shape, ball["shape"]] and edit.set[shape]["normals"] is not None and edit.set[ball["shape"]]["normals"] is not None
    fresh = vpt.HostScene(S.write_scene(S.SYNTH, tmp_path / "b", settings={S.TETRA: {"subdivisions": 1, "smooth": True}, S.BALL: {"displacement": 0.0}}))
    assert json.loads(host.stats())["shapes"] == json.loads(fresh.stats())["shapes"]


def test_the_pending_edits_keep_their_order(vpt):
    host = vpt.HostScene(S.path(S.SYNTH))
    host.set_subdiv(S.STRIP, displacement=0.05)
    for refused in (lambda: host.set_subdiv(S.TETRA, subdivisions=1), lambda: host.remove_shapes([0]), lambda: host.rebuild_bvh("all"),
                    lambda: host.set_instance(0, material=1)):
        with pytest.raises(vpt.VptError, match="update_subdivs"):
            refused()
    host.set_subdiv(S.STRIP, positions=host.subdiv(S.STRIP)["positions"])   # a second change of the same subdiv joins the first
    edit = host.update_subdivs()
    assert list(edit.subdivs) == [S.STRIP] and edit.subdivs[S.STRIP][0] is not None and edit.subdivs[S.STRIP][1] == 0.05
    assert edit.shape_of == {S.STRIP: 3} and edit.payload_bytes() == 12 * 9
    host.set_subdiv(S.TETRA, subdivisions=1)   # nothing pending: allowed now
    with pytest.raises(vpt.VptError, match="update_shapes"):
        host.set_subdiv(S.STRIP, displacement=0.01)


def test_bad_arguments_are_refused_without_a_device(vpt):
    host = vpt.HostScene(S.path(S.SYNTH))
    before = host.stats()
    cage = host.subdiv(S.BOWTIE)["positions"]
    bad = cage.copy()
    bad[3, 1] = np.nan
    for call in (lambda: host.set_subdiv(9), lambda: host.set_subdiv(-1), lambda: host.set_subdiv(S.BOWTIE, positions=cage[:-1]),
                 lambda: host.set_subdiv(S.BOWTIE, positions=bad), lambda: host.set_subdiv(S.STRIP, displacement=np.inf),
                 lambda: host.set_subdiv(S.TETRA, subdivisions=11), lambda: host.subdiv_plan(7)):
        with pytest.raises(vpt.VptError):
            call()
    assert host.stats() == before and host.update_subdivs().empty() and host.update_shapes().empty()
    # the C entry points check their arguments before they look for a device
    plan, keep = host.subdiv_plan(S.BOWTIE).to_abi()
    edit, keep2 = vpt.SubdivEdit({0: (cage, None), 1: (None, 0.5), 2: (None, None)}).to_abi({0: 4, 1: 5, 2: 6})
    out = C.c_int(7)
    invalid = -1
    assert vpt.hip.vpt_scene_attach_subdiv(None, C.byref(plan), C.byref(out)) == invalid and b"null" in vpt.hip.vpt_last_error()
    assert vpt.hip.vpt_multi_attach_subdiv(None, C.byref(plan), C.byref(out)) == invalid and out.value == 7
    assert vpt.hip.vpt_scene_update_subdivs(None, C.byref(edit)) == invalid and vpt.hip.vpt_multi_update_subdivs(None, C.byref(edit)) == invalid
    assert vpt.hip.vpt_session_edit_subdivs(None, C.byref(edit)) == invalid
    assert vpt.hip.vpt_scene_detach_subdiv(None, 0) == invalid and vpt.hip.vpt_scene_subdiv_count(None) == invalid
    assert vpt.hip.vpt_scene_subdiv_shape(None, 0) == -1 and vpt.hip.vpt_multi_subdiv_shape(None, 0) == -1
    # the struct of an edit: ids through the map, a null cage and a NaN amount where an entry keeps
    assert edit.num == 3
    ids = np.ctypeslib.as_array(C.cast(edit.subdiv_ids, C.POINTER(C.c_int32)), (3,))
    cages = C.cast(edit.cage_positions, C.POINTER(C.c_void_p))
    amounts = np.ctypeslib.as_array(C.cast(edit.displacement, C.POINTER(C.c_float)), (3,))
    assert list(ids) == [4, 5, 6] and [bool(cages[i]) for i in range(3)] == [True, False, False]
    assert np.isnan(amounts[0]) and amounts[1] == 0.5 and np.isnan(amounts[2])
    assert vpt.SubdivEdit().empty() and vpt.SubdivEdit().to_abi()[0].num == 0
    del keep, keep2
