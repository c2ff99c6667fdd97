"""vpt_scene_update_instances on the GPU (include/vpt.h).  The criterion is equality of bits, no tolerance anywhere:
A = DeviceScene(original) taken through every step of a case of tests/instance_edits.py against B = a DeviceScene made from the
host mirror after the same steps.  Compared: node arrays, primitive orders and counts against the mirror's bytes; the instances and
the light list against the mirror's; vpt_scene_instance_tables_hash and vpt_scene_light_tables_hash against B's; renders (image as
uint32, rngs, hits), vpt_intersect on 40 000 NaN-prone rays as a scene query and as a single-instance query on the last and on a
renumbered instance."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import instance_edits as I
import synth_scenes
from conftest import ROOT
from test_bvh_rebuild_gpu import MESH_SHADERS, assert_same_trees
from test_scene_update_gpu import rays_for, same_state

pytestmark = pytest.mark.gpu

# an instance whose id the case's edit changed (its new id); None: the edit moves no id, the middle of the list is taken
RENUMBERED = {"crowd_remove_mid": 5, "crowd_remove_lamp": 0, "crowd_all_three": 11, "vol_add_remove": 7, "curves_off_on": 2}


def size_of(case):
    """(resolution, samples, bounces): 03_volume as tests/cases.py renders it, the other scenes at the size of their own tests"""
    return (64, 4, 8) if case.scene == I.S03 else (96, 2, 4)


def render(vpt, dev, host, case, shader):
    res, spp, bounces = size_of(case)
    p = vpt.PathtraceParams(resolution=res, samples=spp, shader=shader, bounces=bounces)
    st = host.make_state(p)
    dev.pathtrace_samples(st, p, spp)
    return st


def assert_same_everything(vpt, A, B, host, case, what, shaders=MESH_SHADERS, n_rays=40000, renumbered=None):
    assert_same_trees(A, host, what)
    assert A.light_tables_hash() == B.light_tables_hash(), f"{what}: light tables differ from the fresh scene's"
    assert A.instance_tables_hash() == B.instance_tables_hash(), f"{what}: instance tables differ from the fresh scene's"
    assert A.get_instances().tobytes() == I.instances_of(host).tobytes(), f"{what}: the instances differ from the host mirror's"
    la, ca = A.get_lights()
    lh, ch = host.lights()
    assert la.tobytes() == lh.tobytes() and ca.tobytes() == ch.tobytes(), f"{what}: the light list or CDFs differ from the host mirror's"
    assert A.media_vary() == B.media_vary(), what
    for shader in shaders:
        assert same_state(render(vpt, A, host, case, shader), render(vpt, B, host, case, shader)), f"{what}: {shader} differs from the fresh scene's render"
    n = host.count("instances")
    if n == 0:
        return
    rays = rays_for(host, n_rays)
    for instance in (-1, n - 1, n // 2 if renumbered is None else renumbered):
        ia, ua = A.intersect(rays, instance)
        ib, ub = B.intersect(rays, instance)
        assert np.array_equal(ia, ib), (what, instance)
        assert np.array_equal(ua.view(np.uint32), ub.view(np.uint32)), (what, instance)
    assert (A.intersect(rays, -1)[0][:, 0] >= 0).mean() > 0.02, f"{what}: the rays hit nothing"


def quad_count(nodes) -> int:
    """quad nodes of a BVH: vpt_scene_prep.cpp quad_order"""
    if len(nodes) == 0 or not nodes[0]["internal"]:
        return 0
    count, todo = 0, [0]
    while todo:
        i = todo.pop()
        count += 1
        for side in range(2):
            c = int(nodes[i]["start"]) + side
            if nodes[c]["internal"]:
                todo += [g for g in (int(nodes[c]["start"]), int(nodes[c]["start"]) + 1) if nodes[g]["internal"]]
    return count


def stated_bytes(edit, host):
    """the bytes the rule of include/vpt.h states for `edit`, the lights' few words apart: (fixed part, lights of the new scene)"""
    pad = lambda n: (n + 15) // 16 * 16
    n_new, (scene_nodes, _) = host.count("instances"), host.bvh_nodes()
    down = pad(pad(4 * len(edit.remove)) + 4 * len(edit.set)) + 128 * (len(edit.set) + len(edit.add))
    down += 128 * quad_count(scene_nodes) + (96 + 4) * n_new
    up = 32 * len(scene_nodes) + 4 * n_new
    return down + up, len(host.lights()[0])


def edited_pair(vpt, tmp_path, name, stats=None):
    """(A, B, the host mirror) after every step of the case; stats: receives (edit, update_stats, stated bytes) per step"""
    case = I.CASES[name]
    file = case.path(tmp_path)
    A = vpt.DeviceScene(vpt.HostScene(file), 0)
    host = vpt.HostScene(file)

    def after(edit):
        A.update_instances(edit)
        if stats is not None:
            stats.append((edit, A.update_stats(), stated_bytes(edit, host)))

    I.apply(host, case, after=after)
    return A, vpt.DeviceScene(host, 0), host


@pytest.mark.parametrize("name", list(I.CASES))
def test_edited_instances_equal_a_fresh_scene(vpt, tmp_path, name):
    case, stats = I.CASES[name], []
    A, B, host = edited_pair(vpt, tmp_path, name, stats)
    for edit, (launches, nbytes, ms), (fixed, lights) in stats:
        print(f"{name}: {launches} launches, {nbytes} bytes, {ms:.3f} device ms; the rule states {fixed} bytes + a few words for each of {lights} lights", flush=True)
        # a condition from the rule, not a measurement: at most 32 + 56 + 4 + 24 + 8 = 124 B per light, SDF lights 4 more
        assert fixed <= nbytes <= fixed + 128 * lights, (name, nbytes, fixed, lights)
    # `implicit` on a mesh scene: K2's mesh-light walk over the new scene BVH
    assert_same_everything(vpt, A, B, host, case, name, MESH_SHADERS + (("implicit",) if name == "vol_add_remove" else ()), renumbered=RENUMBERED.get(name))
    if name == "round_trip":   # the tables of the ORIGINAL fresh handle
        O = vpt.DeviceScene(vpt.HostScene(case.path(tmp_path / "again")), 0)
        assert A.instance_tables_hash() == O.instance_tables_hash() and A.light_tables_hash() == O.light_tables_hash()
        assert [x.tobytes() for x in A.get_bvh() + A.get_bvh_prims()] == [x.tobytes() for x in O.get_bvh() + O.get_bvh_prims()]


def test_an_empty_edit_does_nothing(vpt, tmp_path):
    case = I.CASES["crowd_remove_mid"]
    host = vpt.HostScene(case.path(tmp_path))
    A = vpt.DeviceScene(host, 0)
    A.update_instances(vpt.InstanceEdit((5,)))
    before = A.update_stats()
    hashes = A.instance_tables_hash()
    A.update_instances(vpt.InstanceEdit())
    assert A.update_stats() == before and A.instance_tables_hash() == hashes   # no launch, no bytes: the counters were not even reset


def test_every_instance_removed_and_some_added_again(vpt, tmp_path):
    """zero instances is a scene vpt_scene_create accepts: so does the edit; then the scene is populated again"""
    case = I.CASES["crowd_grow"]
    file = case.path(tmp_path)
    A, host = vpt.DeviceScene(vpt.HostScene(file), 0), vpt.HostScene(file)
    host.remove_instances(range(host.count("instances")))
    A.update_instances(host.update_instances())
    assert host.count("instances") == 0 and len(A.get_instances()) == 0
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, case, "emptied", shaders=("pathtrace",))
    host.add_instance(I.frame(0, (0.5, 0.5, 0.5)), I.LAMP_LARGE, I.MAT_LAMP_LARGE)
    host.add_instance(I.scatter(3), I.BLOB, I.RED)
    A.update_instances(host.update_instances())
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, case, "populated again", n_rays=4000)


def test_frame_edit_then_instances_then_frame_edit(vpt, tmp_path):
    """a refit (its level tables made), an instance edit (they are of the old list), a refit again (made anew), on one handle"""
    import scene_edits as E
    case = I.CASES["crowd_all_three"]
    file = case.path(tmp_path)
    A, host = vpt.DeviceScene(vpt.HostScene(file), 0), vpt.HostScene(file)
    E.translate(host, 20, dx=0.07, dy=0.02)
    A.update(host.update_bvh())
    I.apply(host, case, after=A.update_instances)
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, case, "instances after a refit", n_rays=4000)
    E.translate(host, host.count("instances") - 1, dx=-0.05)
    E.rotate_instance(host, 11, 0.3)
    A.update(host.update_bvh())
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, case, "refit after instances", n_rays=4000)


def test_instances_then_a_shape_rebuild(vpt, tmp_path):
    case = I.CASES["crowd_add_lit_grid"]
    A, B, host = edited_pair(vpt, tmp_path, "crowd_add_lit_grid")
    A.rebuild_bvh(host.rebuild_bvh((I.BLOB, I.GRID_QUADS), True))
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, case, "rebuild after instances", n_rays=4000)
    host.remove_instances([2, 3])          # and the limits of the next instance edit come from the rebuilt shapes
    A.update_instances(host.update_instances())
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, case, "instances after a rebuild", n_rays=4000)


def mixed_scene(tmp_path):
    """03_volume with the volumes, grid instances and SDFs of 06_gridsdf_synth beside its meshes: every kind of edit applies to it"""
    a = json.load(open(os.path.join(I.SCENES, I.S03)))
    g = json.load(open(os.path.join(I.SCENES, "06_gridsdf_synth", "gridsdf_synth.json")))
    out = str(tmp_path / "mixed")
    os.makedirs(out)
    for key in ("shapes", "textures"):
        for item in a[key]:
            item["uri"] = os.path.relpath(os.path.join(I.SCENES, "03_volume", item["uri"]), out)
    for key in ("volumes", "vol_instances", "sdfunctions"):
        a[key] = g[key]
        for item in a[key]:
            if "uri" in item:
                item["uri"] = os.path.relpath(os.path.join(I.SCENES, "06_gridsdf_synth", item["uri"]), out)
    path = os.path.join(out, "mixed.json")
    json.dump(a, open(path, "w"))
    return path


def test_instances_then_the_other_edits(vpt, tmp_path):
    """an instance edit, then update_lights, update_textures and update_volumes on the same handle, each against a fresh one"""
    case = I.Case(I.S03, [I.vol_add_remove])
    file = mixed_scene(tmp_path)
    A, host = vpt.DeviceScene(vpt.HostScene(file), 0), vpt.HostScene(file)
    shaders = ("volpathtrace", "implicit")
    fresh = lambda what: assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, case, what, shaders=shaders, n_rays=4000, renumbered=7)
    I.apply(host, case, after=A.update_instances)
    fresh("instances")
    m = host.material(1)      # the glass becomes a lamp: the light list grows by an instance that was renumbered into place
    m.emission[:] = (2.0, 1.5, 1.0)
    host.set_material(1, m)
    A.update_lights(host.update_lights())
    fresh("lights after instances")
    tex, linear = host.texture(0)
    host.set_texture(0, tex[::-1].copy())
    A.update_textures(host.update_textures())
    fresh("textures after instances")
    host.set_volume_instance(0, scalef=0.0015)
    host.set_sdf(1, material=6)   # an emissive material: an SDF light appears behind the mesh lights
    A.update_volumes(host.update_volumes())
    fresh("volumes after instances")
    host.remove_instances([1])    # and instances again: the SDF light and the environment's stay byte for byte
    A.update_instances(host.update_instances())
    fresh("instances after volumes")


@pytest.mark.parametrize("switch", ["VPT_NO_GROUP_FORMS=1", "VPT_STACK_LDS=4", "VPT_LIGHTS_PLAIN=1"])
def test_ab_switches_give_the_same_bits(switch):
    """the switches are read when a scene is created or edited: in a child process, as the existing tests of such switches do"""
    key, value = switch.split("=")
    env = dict(os.environ, **{key: value})
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", f"{__file__}::test_edited_instances_equal_a_fresh_scene[crowd_all_three]",
                        f"{__file__}::test_edited_instances_equal_a_fresh_scene[crowd_grow]"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("devices", [[0], [0, 0]])
def test_multi_update_instances(vpt, tmp_path, devices):
    """one device, and two virtual ranks on it"""
    case = I.CASES["crowd_all_three"]
    file = case.path(tmp_path)
    M = vpt.MultiDeviceScene(vpt.HostScene(file), devices)
    host = vpt.HostScene(file)
    I.apply(host, case, after=M.update_instances)
    B = vpt.DeviceScene(host, 0)
    p = vpt.PathtraceParams(resolution=96, samples=2, shader="volpathtrace", bounces=4)
    want, got = host.make_state(p), host.make_state(p)
    B.pathtrace_samples(want, p, 2)
    M.pathtrace_samples(got, p, 2)
    assert same_state(got, want)
    with pytest.raises(vpt.VptError):
        M.update_instances(vpt.InstanceEdit((999,)))
    M.close()


def test_the_adaptive_path_after_an_edit(vpt, tmp_path):
    A, B, host = edited_pair(vpt, tmp_path, "crowd_remove_lamp")
    p = vpt.PathtraceParams(resolution=64, samples=24, shader="pathtrace", bounces=4)
    a, b = host.make_state(p), host.make_state(p)
    ra = A.pathtrace_adaptive(a, p, 0.05, min_samples=4, step=4)
    rb = B.pathtrace_adaptive(b, p, 0.05, min_samples=4, step=4)
    assert ra == rb and same_state(a, b)


def test_session_edit_instances(vpt, tmp_path):
    """the preview and the display after edit_instances + N samples equal a fresh session's; a refused edit leaves the session as it was"""
    case = I.CASES["crowd_all_three"]
    file = case.path(tmp_path)
    host = vpt.HostScene(file)
    p = vpt.PathtraceParams(resolution=96, samples=8, shader="pathtrace", bounces=4)
    session = vpt.RenderSession(vpt.DeviceScene(vpt.HostScene(file), 0), p, pratio=8)
    session.advance(3)
    I.apply(host, case, after=session.edit_instances)
    assert session.samples == 0
    fresh = vpt.RenderSession(vpt.DeviceScene(host, 0), p, pratio=8)
    assert np.array_equal(session.display(), fresh.display())   # the preview
    session.advance(3), fresh.advance(3)
    assert same_state(session.state(), fresh.state())
    session.advance(5), fresh.advance(5)
    assert same_state(session.state(), fresh.state()) and np.array_equal(session.display(), fresh.display())
    with pytest.raises(vpt.VptError):
        session.edit_instances(vpt.InstanceEdit((3, 3)))
    assert session.samples == 8 and same_state(session.state(), fresh.state())
    session.close(), fresh.close()


def nan_frame():
    f = I.frame()
    f[4] = np.nan
    return f


def test_refusals_leave_the_scene_untouched(vpt, tmp_path):
    case = I.CASES["vol_add_remove"]
    host = vpt.HostScene(case.path(tmp_path))
    A = vpt.DeviceScene(host, 0)
    n, ok = host.count("instances"), I.frame()
    before = [render(vpt, A, host, case, s) for s in ("volpathtrace", "normal")]
    state = lambda: ([x.tobytes() for x in A.get_bvh() + A.get_bvh_prims()], A.instance_tables_hash(), A.light_tables_hash(), A.get_instances().tobytes())
    was = state()
    bad = [vpt.InstanceEdit((n,)), vpt.InstanceEdit((-1,)), vpt.InstanceEdit((2, 2)),                   # bad ids
           vpt.InstanceEdit(set={n: (ok, 1, 1)}), vpt.InstanceEdit((3,), set={3: (ok, 1, 1)}),          # ... and one both set and removed
           vpt.InstanceEdit(add=[(ok, host.count("shapes"), 0)]), vpt.InstanceEdit(add=[(ok, -1, 0)]),  # bad shape
           vpt.InstanceEdit(set={0: (ok, 0, host.count("materials"))}), vpt.InstanceEdit(add=[(ok, 1, -2)]),   # bad material
           vpt.InstanceEdit(add=[(nan_frame(), 1, 1)]), vpt.InstanceEdit(set={1: (nan_frame(), 1, 1)})]  # a NaN frame
    for edit in bad:
        with pytest.raises(vpt.VptError):
            A.update_instances(edit)
        assert vpt.hip.vpt_last_error() != b""
    ids = (C.c_int32 * 2)(0, 1)
    rec = (vpt.VptInstance * 2)()
    for abi in (vpt.VptInstanceEdit(2, None, 0, None, None, 0, None), vpt.VptInstanceEdit(0, None, 2, C.cast(ids, C.c_void_p), None, 0, None),
                vpt.VptInstanceEdit(0, None, 2, None, C.cast(rec, C.c_void_p), 0, None), vpt.VptInstanceEdit(0, None, 0, None, None, 1, None),
                vpt.VptInstanceEdit(-1, C.cast(ids, C.c_void_p), 0, None, None, 0, None)):      # null lists with non-zero counts, a negative count
        assert vpt.hip.vpt_scene_update_instances(A.handle, C.byref(abi)) == -1, vpt.hip.vpt_last_error()
    assert vpt.hip.vpt_scene_update_instances(A.handle, None) == -1 and b"null" in vpt.hip.vpt_last_error()
    assert state() == was
    assert all(same_state(render(vpt, A, host, case, s), b) for s, b in zip(("volpathtrace", "normal"), before))


def test_a_dangling_texture_id_on_a_newly_bound_material_is_refused(vpt, tmp_path):
    """06_gridsdf ships materials with dangling texture ids that only SDFs use: creation tolerates them there and refuses them on a mesh
    instance; so does the edit, for the same reason - and a scene file with the instance is refused by vpt_scene_create"""
    file = mixed_scene(tmp_path)
    d = json.load(open(file))
    d["materials"].append({"name": "dangling", "type": "matte", "color": [0.5, 0.5, 0.5], "color_tex": 1})
    d["textures"] = d["textures"][:1]                     # texture 1 is gone ...
    d["environments"][0].pop("emission_tex")              # ... from the environment too
    d["sdfunctions"][0]["material"] = len(d["materials"]) - 1   # bound to an SDF only: tolerated
    json.dump(d, open(file, "w"))
    host, dangling = vpt.HostScene(file), len(d["materials"]) - 1
    A = vpt.DeviceScene(host, 0)
    was = (A.instance_tables_hash(), A.light_tables_hash())
    for edit in (vpt.InstanceEdit(add=[(I.frame(), 1, dangling)]), vpt.InstanceEdit(set={2: (I.frame(), 1, dangling)})):
        abi, keep = edit.to_abi()
        assert vpt.hip.vpt_scene_update_instances(A.handle, C.byref(abi)) == -1 and b"texture id out of range" in vpt.hip.vpt_last_error()
    assert (A.instance_tables_hash(), A.light_tables_hash()) == was
    host.add_instance(I.frame(), 1, dangling)
    host.update_instances()
    out = C.c_void_p()
    assert vpt.hip.vpt_scene_create_curves(host.desc, host.curves, 0, C.byref(out)) == -1 and b"texture id out of range" in vpt.hip.vpt_last_error()


def test_a_scene_tree_past_the_stack_limit_is_refused_and_the_scene_stays(vpt, tmp_path):
    """One shape, a chain 200 levels deep (chain_geometry), and 60 added instances of it laid out as deep_scene lays out its scene-level
    chain - box [0, 4 v] on axis i % 3, v shrinking by 0.77 - so that split_middle peels one instance per level: the binary walk would
    need (scene depth + 2) + (200 + 2) > 256 entries.  The edit is refused with VPT_ERR_UNSUPPORTED after everything was built, the
    scene is untouched, vpt_scene_create refuses the mirror's descriptor for the same reason, and a smaller addition still works."""
    depth, added = 200, 60
    w = synth_scenes._Writer(str(tmp_path))
    chain = w.shape("chain", *synth_scenes.chain_geometry(depth))
    w.instance(chain, np.concatenate([np.eye(3).reshape(-1), [0, 0, 0]]), 0)
    file, facts = w.write("deep_chain", synth_scenes._look_at([-2.2, -1.8, -2.6], [0.3, 0.3, 0.3]))
    case = I.Case(file, [])
    A, host, big = vpt.DeviceScene(vpt.HostScene(file), 0), vpt.HostScene(file), vpt.HostScene(file)
    v = 0.5
    for i in range(added):
        f = synth_scenes._axis_frame(i % 3, v)
        f[9 + i % 3] = np.float32(2) * np.float32(v)      # the chain's root box is [-2, 2]^3: [0, 4 v] on the item's axis
        big.add_instance(f, chain, i % 2)
        v *= synth_scenes.CHAIN_RATIO
    edit = big.update_instances()
    scene_depth = synth_scenes.bvh_depth(big.bvh_nodes()[0])
    assert synth_scenes.stack_need(scene_depth, depth) > synth_scenes.STACK_LIMIT, scene_depth
    out = C.c_void_p()
    assert vpt.hip.vpt_scene_create_curves(big.desc, big.curves, 0, C.byref(out)) == -5 and b"traversal stack" in vpt.hip.vpt_last_error()
    before = ([x.tobytes() for x in A.get_bvh() + A.get_bvh_prims()], A.instance_tables_hash(), A.light_tables_hash())
    image = render(vpt, A, host, case, "normal")
    abi, keep = edit.to_abi()
    assert vpt.hip.vpt_scene_update_instances(A.handle, C.byref(abi)) == -5, vpt.hip.vpt_last_error().decode()
    assert b"traversal stack" in vpt.hip.vpt_last_error()
    assert ([x.tobytes() for x in A.get_bvh() + A.get_bvh_prims()], A.instance_tables_hash(), A.light_tables_hash()) == before
    assert same_state(render(vpt, A, host, case, "normal"), image)
    for k in range(3):
        host.add_instance(I.scatter(k), chain, k % 2)
    A.update_instances(host.update_instances())
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, case, "a smaller addition", shaders=("pathtrace", "normal"), n_rays=4000)
