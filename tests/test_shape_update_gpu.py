"""vpt_scene_update_shapes on the GPU (include/vpt.h).  The criterion is equality of bits, no tolerance anywhere:
A = DeviceScene(original) taken through every step of a case of tests/shape_edits.py against B = a DeviceScene made from the host
mirror after the same steps.  Compared: node arrays, primitive orders, counts and offsets against the mirror's bytes; the instances
and the light list and CDFs against the mirror's; vpt_scene_shape_tables_hash, vpt_scene_instance_tables_hash and
vpt_scene_light_tables_hash against B's; renders (image as uint32, rngs, hits); vpt_intersect on 40 000 NaN-prone rays as a scene
query and as single-instance queries on an instance of a replaced shape and of a renumbered one; the bytes against the rule.
Every test calls an entry point that exists only with the feature."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import instance_edits as I
import shape_edits as S
import synth_scenes
from conftest import ROOT
from test_instance_update_gpu import assert_same_everything as assert_same_instances_and_renders
from test_instance_update_gpu import mixed_scene, quad_count, render
from test_scene_update_gpu import same_state
from test_shape_update_host import TRIANGLE, desc_shapes

pytestmark = pytest.mark.gpu

# per case: an instance of a replaced shape, or one whose shape id the edit changed (None: the middle of the list)
QUERIED = {"tri_leaf_5": 2, "blob_65_257": 4, "grid_shrink_flip": 3, "remove_first": 3, "add_two": 71, "all_three": 5, "lamp_small_sizes": 0, "lamp_large_2": 1,
           "curves_radii": 2, "points_on": 70, "curves_off": 3, "vol_colours": 3, "vol_lamp": 6}


def all_hashes(dev):
    return dev.shape_tables_hash(), dev.instance_tables_hash(), dev.light_tables_hash()


def assert_same_everything(vpt, A, B, host, case, what, **kw):
    assert A.get_shape_counts() == B.get_shape_counts() and A.get_shape_counts()[0] == host.count("shapes"), what
    assert A.record_bytes() == B.record_bytes(), f"{what}: the compact records are there on one handle only"
    for k, (a, b) in enumerate(zip(A.shape_tables_hash(), B.shape_tables_hash())):
        assert a == b, f"{what}: group {k} of the shape tables differs from the fresh scene's"
    assert_same_instances_and_renders(vpt, A, B, host, case, what, **kw)


def pad16(n):
    return (n + 15) // 16 * 16


def payload_bytes(meshes):
    """the staged block: every array of every mesh at a 16-byte aligned offset - positions, normals, texcoords, colors, the radius of a
    shape of points or lines, the index list (an empty one still takes its aligned place)"""
    size = 0
    for m in meshes:
        curves = m["points"] is not None or m["lines"] is not None
        index = next((m[k] for k in ("triangles", "quads", "points", "lines") if m[k] is not None), None)
        size = pad16(size) + (0 if m["positions"] is None else m["positions"].nbytes)
        for a in (m["normals"], m["texcoords"], m["colors"], m["radius"] if curves else None):
            if a is not None:
                size = pad16(size) + a.nbytes
        size = pad16(size) + (0 if index is None else index.nbytes)
    return size


def stated_bytes(edit, host, shapes_before):
    """the bytes the rule of include/vpt.h states for `edit`, the lights' few words apart: (fixed part, lights of the new scene);
    host: the mirror AFTER the edit"""
    n_new, n_inst = host.count("shapes"), host.count("instances")
    scene_nodes, shape_nodes = host.bvh_nodes()
    d = desc_shapes(host)
    survivors = shapes_before - len(edit.remove)
    new_of_old = {old: new for new, old in enumerate(i for i in range(shapes_before) if i not in edit.remove)}
    made = [new_of_old[i] for i in edit.set] + list(range(survivors, n_new))
    elems = lambda j: max(d[j]["num_triangles"], d[j]["num_quads"], *(len(host.shape_arrays(j)[k]) for k in ("points", "lines")))
    nodes = lambda j: shape_nodes[d[j]["bvh_node_offset"]: d[j]["bvh_node_offset"] + d[j]["num_bvh_nodes"]]
    built = len(edit.set) > 0
    down = payload_bytes(list(edit.set.values()) + list(edit.add)) + sum(128 * quad_count(nodes(j)) for j in made) + 80 * n_new * (2 if built else 1)
    down += 8 * shapes_before + (96 + 4) * n_inst + (128 * quad_count(scene_nodes) if built else 0)
    up = sum(32 * len(nodes(j)) + 4 * int(elems(j)) for j in made) + ((32 * len(scene_nodes) + 4 * n_inst) if built else 0)
    return down + up, len(host.lights()[0])


def edited_pair(vpt, tmp_path, name, stats=None):
    """(A, B, the host mirror) after every step of the case; stats: receives (update_stats, stated bytes) per shape step"""
    case = S.ALL_CASES[name]
    file = case.path(tmp_path)
    A = vpt.DeviceScene(vpt.HostScene(file), 0)
    host = vpt.HostScene(file)
    count = [host.count("shapes")]

    def after_shapes(edit):
        A.update_shapes(edit)
        if stats is not None:
            stats.append((A.update_stats(), stated_bytes(edit, host, count[0])))
        count[0] = host.count("shapes")

    S.apply(host, case, after_shapes=after_shapes, after_instances=A.update_instances)
    return A, vpt.DeviceScene(host, 0), host


@pytest.mark.parametrize("name", list(S.ALL_CASES))
def test_edited_shapes_equal_a_fresh_scene(vpt, tmp_path, name):
    case, stats = S.ALL_CASES[name], []
    A, B, host = edited_pair(vpt, tmp_path, name, stats)
    for (launches, nbytes, ms), (fixed, lights) in stats:
        print(f"{name}: {launches} launches, {nbytes} bytes, {ms:.3f} device ms; the rule states {fixed} bytes + a few words for each of {lights} lights", flush=True)
        # a condition from the rule, not a measurement: at most 32 + 56 + 4 + 24 + 8 = 124 B per light, SDF lights 4 more
        assert fixed <= nbytes <= fixed + 128 * lights, (name, nbytes, fixed, lights)
    shaders = ("pathtrace", "volpathtrace", "eyelight", "normal") + (("implicit",) if case.scene == S.S03 else ())
    assert_same_everything(vpt, A, B, host, case, name, shaders=shaders, renumbered=QUERIED.get(name))
    if name in S.ROUND_TRIPS:   # the tables of the ORIGINAL fresh handle
        O = vpt.DeviceScene(vpt.HostScene(case.path(tmp_path / "again")), 0)
        assert all_hashes(A) == all_hashes(O)
        assert [x.tobytes() for x in A.get_bvh() + A.get_bvh_prims()] == [x.tobytes() for x in O.get_bvh() + O.get_bvh_prims()]


def test_the_kernel_instances_follow_the_scene(vpt, tmp_path):
    """compact records go and come back, VPT_FEAT_CURVES switches on and off (the intersect kernels are chosen by it), varying media flip"""
    seen = []
    case = S.CASES["compact_off_on"]
    file = case.path(tmp_path / "tris")
    A, host = vpt.DeviceScene(vpt.HostScene(file), 0), vpt.HostScene(file)
    S.apply(host, case, after_shapes=lambda e: (A.update_shapes(e), seen.append(A.record_bytes())), after_instances=A.update_instances)
    assert seen == [(64, 96), (48, 64)] and A.shape_tables_hash()[5] != 0
    file = S.CASES["vol_colours"].path(tmp_path)
    A, host = vpt.DeviceScene(vpt.HostScene(file), 0), vpt.HostScene(file)
    seen = [A.media_vary()]
    S.apply(host, S.CASES["vol_colours"], after_shapes=lambda e: (A.update_shapes(e), seen.append(A.media_vary())))
    assert seen == [False, True, False]


def test_an_empty_edit_does_nothing(vpt, tmp_path):
    case = S.CASES["tri_leaf_5"]
    host = vpt.HostScene(case.path(tmp_path))
    A = vpt.DeviceScene(host, 0)
    A.update_shapes(vpt.ShapeEdit(add=[TRIANGLE]))
    before, hashes = A.update_stats(), all_hashes(A)
    A.update_shapes(vpt.ShapeEdit())
    assert A.update_stats() == before and all_hashes(A) == hashes   # no launch, no bytes: the counters were not even reset


def test_shapes_then_instances_then_shapes(vpt, tmp_path):
    """the "import an object" sequence and back, on one handle"""
    case = S.CASES["add_two"]
    A, B, host = edited_pair(vpt, tmp_path, "add_two")
    host.remove_instances([70, 71, 72])
    A.update_instances(host.update_instances())
    host.remove_shapes([7])
    host.set_shape(S.QUAD_LEAF, **S.grid(4))
    A.update_shapes(host.update_shapes())
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, case, "shapes, instances, shapes", n_rays=4000, renumbered=3)


def test_shapes_then_refit_then_rebuild_then_shapes(vpt, tmp_path):
    """a refit after a shape edit makes its level tables anew; a rebuild fills the per-shape depths the next shape edit decides from"""
    import scene_edits as E
    case = S.CASES["blob_65_257"]
    A, B, host = edited_pair(vpt, tmp_path, "blob_65_257")
    E.translate(host, 20, dx=0.07, dy=0.02)
    host.set_shape_positions(S.GRID_TRIS, E.nudge(host.shape_positions(S.GRID_TRIS)))
    A.update(host.update_bvh())
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, case, "refit after shapes", n_rays=4000, shaders=("pathtrace", "normal"))
    A.rebuild_bvh(host.rebuild_bvh((S.BLOB, S.GRID_TRIS), True))
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, case, "rebuild after shapes", n_rays=4000, shaders=("pathtrace", "normal"))
    host.add_shape(**S.blob(30, seed=2))      # no shape replaced: the refitted and rebuilt trees and the scene BVH stay as the device holds them
    A.update_shapes(host.update_shapes())
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, case, "shapes after a rebuild", n_rays=4000, shaders=("pathtrace", "normal"))


def test_shapes_then_the_other_edits(vpt, tmp_path):
    """a shape edit, then update_lights, update_textures and update_volumes on a scene with meshes, grids and SDFs, each against a fresh one"""
    case = S.Case(S.S03, [])
    file = mixed_scene(tmp_path)
    A, host = vpt.DeviceScene(vpt.HostScene(file), 0), vpt.HostScene(file)
    shaders = ("volpathtrace", "implicit")
    fresh = lambda what: assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, case, what, shaders=shaders, n_rays=4000, renumbered=6)
    host.set_shape(S.AREALIGHT1, **S.lamp(3))
    host.add_shape(**S.blob(12, seed=5, scale=0.25))
    A.update_shapes(host.update_shapes())
    fresh("shapes")
    m = host.material(1)      # the glass becomes a lamp: a light on the sphere
    m.emission[:] = (2.0, 1.5, 1.0)
    host.set_material(1, m)
    A.update_lights(host.update_lights())
    fresh("lights after shapes")
    tex, linear = host.texture(0)
    host.set_texture(0, tex[::-1].copy())
    A.update_textures(host.update_textures())
    fresh("textures after shapes")
    host.set_volume_instance(0, scalef=0.0015)
    host.set_sdf(1, material=6)   # an emissive material: an SDF light appears behind the mesh lights
    A.update_volumes(host.update_volumes())
    fresh("volumes after shapes")
    host.set_shape(S.SPHERE, **S.blob(40, seed=9, scale=0.25))   # and shapes again: the SDF light and the environment's stay byte for byte
    A.update_shapes(host.update_shapes())
    fresh("shapes after volumes")


@pytest.mark.parametrize("switch", ["VPT_NO_GROUP_FORMS=1", "VPT_STACK_LDS=4", "VPT_LIGHTS_PLAIN=1", "VPT_NO_COMPACT_TRIANGLES=1"])
def test_ab_switches_give_the_same_bits(switch):
    """the switches are read when a scene is created or edited: in a child process, as the existing tests of such switches do"""
    key, value = switch.split("=")
    env = dict(os.environ, **{key: value})
    names = ["compact_off_on", "curves_off"] if key == "VPT_NO_COMPACT_TRIANGLES" else ["all_three", "lamp_small_sizes"]
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu"] + [f"{__file__}::test_edited_shapes_equal_a_fresh_scene[{n}]" for n in names],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("devices", [[0], [0, 0]])
def test_multi_update_shapes(vpt, tmp_path, devices):
    """one device, and two virtual ranks on it"""
    case = S.CASES["all_three"]
    file = case.path(tmp_path)
    M = vpt.MultiDeviceScene(vpt.HostScene(file), devices)
    host = vpt.HostScene(file)
    S.apply(host, case, after_shapes=M.update_shapes, after_instances=M.update_instances)
    B = vpt.DeviceScene(host, 0)
    p = vpt.PathtraceParams(resolution=96, samples=2, shader="volpathtrace", bounces=4)
    want, got = host.make_state(p), host.make_state(p)
    B.pathtrace_samples(want, p, 2)
    M.pathtrace_samples(got, p, 2)
    assert same_state(got, want)
    with pytest.raises(vpt.VptError):
        M.update_shapes(vpt.ShapeEdit((999,)))
    M.close()


def test_the_adaptive_path_after_an_edit(vpt, tmp_path):
    A, B, host = edited_pair(vpt, tmp_path, "lamp_large_2")
    p = vpt.PathtraceParams(resolution=64, samples=24, shader="pathtrace", bounces=4)
    a, b = host.make_state(p), host.make_state(p)
    ra = A.pathtrace_adaptive(a, p, 0.05, min_samples=4, step=4)
    rb = B.pathtrace_adaptive(b, p, 0.05, min_samples=4, step=4)
    assert ra == rb and same_state(a, b)


def test_session_edit_shapes(vpt, tmp_path):
    """the preview and the display after edit_shapes + N samples equal a fresh session's; a refused edit leaves the session as it was"""
    case = S.CASES["grid_shrink_flip"]
    file = case.path(tmp_path)
    host = vpt.HostScene(file)
    p = vpt.PathtraceParams(resolution=96, samples=8, shader="pathtrace", bounces=4)
    session = vpt.RenderSession(vpt.DeviceScene(vpt.HostScene(file), 0), p, pratio=8)
    session.advance(3)
    S.apply(host, case, after_shapes=session.edit_shapes)
    assert session.samples == 0
    fresh = vpt.RenderSession(vpt.DeviceScene(host, 0), p, pratio=8)
    assert np.array_equal(session.display(), fresh.display())   # the preview
    session.advance(3), fresh.advance(3)
    assert same_state(session.state(), fresh.state())
    session.advance(5), fresh.advance(5)
    assert same_state(session.state(), fresh.state()) and np.array_equal(session.display(), fresh.display())
    with pytest.raises(vpt.VptError):
        session.edit_shapes(vpt.ShapeEdit((3, 3)))
    assert session.samples == 8 and same_state(session.state(), fresh.state())
    session.close(), fresh.close()


def test_refusals_leave_the_scene_untouched(vpt, tmp_path):
    """every refusal class of include/vpt.h, with all hashes and a render unchanged"""
    case = S.CASES["vol_lamp"]
    host = vpt.HostScene(case.path(tmp_path))
    A = vpt.DeviceScene(host, 0)
    n = host.count("shapes")
    P = TRIANGLE["positions"]
    before = [render(vpt, A, host, case, s) for s in ("volpathtrace", "normal")]
    state = lambda: ([x.tobytes() for x in A.get_bvh() + A.get_bvh_prims()], all_hashes(A), A.get_instances().tobytes(), A.get_shape_counts())
    was = state()
    bad_float = lambda key, width: dict(TRIANGLE, **{key: np.full((3, width) if width else (3,), np.nan, np.float32)})
    bad = [vpt.ShapeEdit((n,)), vpt.ShapeEdit((-1,)), vpt.ShapeEdit(set={n: TRIANGLE}),                          # bad ids
           vpt.ShapeEdit((S.SPHERE,)),                                                                          # instances still name it
           vpt.ShapeEdit(add=[dict(positions=P, triangles=[[0, 1, 3]])]), vpt.ShapeEdit(add=[dict(positions=P, quads=[[0, 1, 2, -1]])]),
           vpt.ShapeEdit(set={0: dict(positions=P, lines=[[0, 3]], radius=[1, 1, 1])}), vpt.ShapeEdit(add=[dict(positions=P, points=[5], radius=[1, 1, 1])]),
           vpt.ShapeEdit(add=[dict(TRIANGLE, quads=[[0, 1, 2, 2]])]),                                           # both triangles and quads
           vpt.ShapeEdit(add=[dict(positions=P, points=[0, 1])]),                                               # points without radius
           vpt.ShapeEdit(add=[bad_float("positions", 3)]), vpt.ShapeEdit(add=[bad_float("normals", 3)]), vpt.ShapeEdit(add=[bad_float("texcoords", 2)]),
           vpt.ShapeEdit(add=[bad_float("colors", 4)]), vpt.ShapeEdit(add=[dict(positions=P, points=[0], radius=[np.inf, 1, 1])])]
    for edit in bad:
        abi, keep = edit.to_abi()
        assert vpt.hip.vpt_scene_update_shapes(A.handle, C.byref(abi)) == -1, vpt.hip.vpt_last_error()
        assert vpt.hip.vpt_last_error() != b""
    mixed = vpt.ShapeEdit(add=[dict(positions=P, lines=[[0, 1]], triangles=[[0, 1, 2]], radius=[1, 1, 1])])      # VPT_ERR_UNSUPPORTED, as at creation
    abi, keep = mixed.to_abi()
    assert vpt.hip.vpt_scene_update_shapes(A.handle, C.byref(abi)) == -5 and b"mixes" in vpt.hip.vpt_last_error()
    ids = (C.c_int32 * 2)(0, 0)
    rec = (vpt.VptShapeData * 2)()
    both = vpt.ShapeEdit((3,), set={3: TRIANGLE}).to_abi()
    for abi in (vpt.VptShapeEdit(2, None, 0, None, None, 0, None), vpt.VptShapeEdit(0, None, 2, C.cast(ids, C.c_void_p), None, 0, None),
                vpt.VptShapeEdit(0, None, 2, None, C.cast(rec, C.c_void_p), 0, None), vpt.VptShapeEdit(0, None, 0, None, None, 1, None),
                vpt.VptShapeEdit(-1, C.cast(ids, C.c_void_p), 0, None, None, 0, None), vpt.VptShapeEdit(2, C.cast(ids, C.c_void_p), 0, None, None, 0, None), both[0]):
        assert vpt.hip.vpt_scene_update_shapes(A.handle, C.byref(abi)) == -1, vpt.hip.vpt_last_error()
    assert vpt.hip.vpt_scene_update_shapes(A.handle, None) == -1 and b"null" in vpt.hip.vpt_last_error()
    assert state() == was
    assert all(same_state(render(vpt, A, host, case, s), b) for s, b in zip(("volpathtrace", "normal"), before))


def test_a_shape_past_the_stack_limit_is_refused_and_a_removed_deep_shape_lowers_the_stacks(vpt, tmp_path, capfd):
    """deep_scene's layout of instances with a chain shape added that is deep enough for creation to refuse the mirror's descriptor:
    the shape edit that would make an INSTANCED shape that deep is refused with VPT_ERR_UNSUPPORTED after building, the scene is
    untouched and a smaller replacement works afterwards.  Then the deepest shape of a scene is removed: VPT_DEBUG's stack line, printed
    when the limits are decided, is a fresh handle's."""
    file, facts = synth_scenes.deep_scene(str(tmp_path), levels=20, chain_depth=12, name="deep20")
    chain = 0                                                    # deep_scene lists the chain first
    case = S.Case(file, [])
    A, host, big = vpt.DeviceScene(vpt.HostScene(file), 0), vpt.HostScene(file), vpt.HostScene(file)
    depth = synth_scenes.STACK_LIMIT - facts["scene_depth"] - 4 + 1   # (scene + 2) + (depth + 2) > 256
    big.set_shape(chain, **dict(zip(("positions", "triangles"), synth_scenes.chain_geometry(depth))))
    edit = big.update_shapes()
    assert synth_scenes.stack_need(synth_scenes.bvh_depth(big.bvh_nodes()[0]), depth) > synth_scenes.STACK_LIMIT
    out = C.c_void_p()
    assert vpt.hip.vpt_scene_create_curves(big.desc, big.curves, 0, C.byref(out)) == -5 and b"traversal stack" in vpt.hip.vpt_last_error()
    before = ([x.tobytes() for x in A.get_bvh() + A.get_bvh_prims()], all_hashes(A), A.get_shape_counts())
    image = render(vpt, A, host, case, "normal")
    abi, keep = edit.to_abi()
    assert vpt.hip.vpt_scene_update_shapes(A.handle, C.byref(abi)) == -5, vpt.hip.vpt_last_error().decode()
    assert b"traversal stack" in vpt.hip.vpt_last_error()
    assert ([x.tobytes() for x in A.get_bvh() + A.get_bvh_prims()], all_hashes(A), A.get_shape_counts()) == before
    assert same_state(render(vpt, A, host, case, "normal"), image)
    host.set_shape(chain, **dict(zip(("positions", "triangles"), synth_scenes.chain_geometry(30))))   # a smaller one works afterwards
    A.update_shapes(host.update_shapes())
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, case, "a smaller replacement", shaders=("pathtrace", "normal"), n_rays=4000)
    # the deepest shape leaves: its instance first, then the shape; the limits are decided from the shapes that stay
    host.remove_instances(S.instances_of_shape(host, chain))
    A.update_instances(host.update_instances())
    host.remove_shapes([chain])
    edit = host.update_shapes()
    os.environ["VPT_DEBUG"] = "1"
    try:
        capfd.readouterr()
        A.update_shapes(edit)
        edited = [line for line in capfd.readouterr().err.splitlines() if "quad stack need" in line]
        B = vpt.DeviceScene(host, 0)
        created = [line for line in capfd.readouterr().err.splitlines() if "quad stack need" in line]
    finally:
        del os.environ["VPT_DEBUG"]
    assert len(edited) == 1 and edited == created[-1:], (edited, created)
    assert_same_everything(vpt, A, B, host, case, "the deepest shape removed", shaders=("pathtrace", "normal"), n_rays=4000)
