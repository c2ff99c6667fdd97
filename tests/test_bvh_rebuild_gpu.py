"""vpt_scene_rebuild_bvh on the GPU (include/vpt.h).  The criterion is equality of bits, no tolerance anywhere:
A = DeviceScene(original) taken through every step of a case of tests/rebuild_edits.py (the edit through update_lights, then
rebuild_bvh) against B = a DeviceScene made from the host mirror after the same steps.  Compared: node arrays, primitive orders and
counts against the mirror's bytes; renders (image as uint32, rngs, hits) at the sizes of tests/cases.py, vpt_intersect on 40 000
NaN-prone rays (scene query and single-instance query) and vpt_scene_light_tables_hash against B's."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rebuild_edits as R
from conftest import ROOT
from test_scene_update_gpu import rays_for, same_state

pytestmark = pytest.mark.gpu

MESH_SHADERS = ("pathtrace", "volpathtrace", "eyelight", "normal")


def size_of(case):
    """(resolution, samples, bounces): 03_volume as tests/cases.py renders it, the curves and synthetic scenes at the size of their own tests"""
    return (64, 4, 8) if case.scene == R.S03 else (96, 2, 4)


def render(vpt, dev, host, case, shader):
    res, spp, bounces = size_of(case)
    p = vpt.PathtraceParams(resolution=res, samples=spp, shader=shader, bounces=bounces)
    st = host.make_state(p)
    dev.pathtrace_samples(st, p, spp)
    return st


def assert_same_trees(dev, host, what):
    a, b = dev.get_bvh()
    c, d = host.bvh_nodes()
    assert dev.get_bvh_counts()[:2] == (len(c), len(d)), what
    assert a.tobytes() == c.tobytes(), f"{what}: scene BVH nodes differ from the host mirror's"
    assert b.tobytes() == d.tobytes(), f"{what}: shape BVH nodes differ from the host mirror's"
    pa, pb = dev.get_bvh_prims()
    pc, pd = host.bvh_prims()
    assert pa.tobytes() == pc.tobytes(), f"{what}: the scene's primitive order differs from the host mirror's"
    assert pb.tobytes() == pd.tobytes(), f"{what}: the shapes' primitive orders differ from the host mirror's"
    offsets, at = dev.get_bvh_counts()[2], 0
    for s, shape in enumerate(__import__("json").loads(host.stats())["shapes"]):
        assert offsets[s] == at, (what, s)
        at += shape["bvh_nodes"]


def assert_same_everything(vpt, A, B, host, case, what, shaders=MESH_SHADERS, n_rays=40000):
    assert_same_trees(A, host, what)
    assert A.light_tables_hash() == B.light_tables_hash(), f"{what}: light tables differ from the fresh scene's"
    for shader in shaders:
        assert same_state(render(vpt, A, host, case, shader), render(vpt, B, host, case, shader)), f"{what}: {shader} differs from the fresh scene's render"
    rays = rays_for(host, n_rays)
    for instance in (-1, host.count("instances") - 1):
        ia, ua = A.intersect(rays, instance)
        ib, ub = B.intersect(rays, instance)
        assert np.array_equal(ia, ib), (what, instance)
        assert np.array_equal(ua.view(np.uint32), ub.view(np.uint32)), (what, instance)
    assert (A.intersect(rays, -1)[0][:, 0] >= 0).mean() > 0.02, f"{what}: the rays hit nothing"


def rebuilt_pair(vpt, tmp_path, name):
    """(A, B, the host mirror) after every step of the case"""
    case = R.CASES[name]
    file = case.path(tmp_path)
    A = vpt.DeviceScene(vpt.HostScene(file), 0)
    host = vpt.HostScene(file)
    R.apply(host, case, after_edit=A.update_lights, after_rebuild=A.rebuild_bvh)
    return A, vpt.DeviceScene(host, 0), host


@pytest.mark.parametrize("name", list(R.CASES))
def test_rebuild_equals_a_fresh_scene(vpt, tmp_path, name):
    case = R.CASES[name]
    A, B, host = rebuilt_pair(vpt, tmp_path, name)
    print(f"{name}: {A.update_stats()} (launches, bytes, device ms)", flush=True)
    # `implicit` on a mesh scene: K2's mesh-light walk over the rebuilt binary trees (03_volume has two mesh lights)
    assert_same_everything(vpt, A, B, host, case, name, MESH_SHADERS + (("implicit",) if name == "vol_times2" else ()))


def test_rebuild_twice_and_then_a_refit(vpt, tmp_path):
    """a second rebuild changes nothing; an instance edit through vpt_scene_update afterwards refits the NEW trees (its level and
    quad-slot tables are made anew), against the mirror"""
    import scene_edits as E
    case = R.CASES["curves_twist"]
    A, B, host = rebuilt_pair(vpt, tmp_path, "curves_twist")
    A.rebuild_bvh(vpt.BvhRebuild((R.HAIR, R.DUST), True))
    assert_same_everything(vpt, A, B, host, case, "rebuilt twice", n_rays=4000)
    E.translate(host, 2, dx=0.07, dy=0.02)
    E.rotate_instance(host, 7, 0.3)
    A.update(host.update_bvh())
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, case, "refit after a rebuild", n_rays=4000)
    A.rebuild_bvh(host.rebuild_bvh((), True))   # the scene level alone
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, case, "scene level alone", n_rays=4000)


def test_fold_and_unfold_on_one_handle(vpt, tmp_path, monkeypatch, capfd):
    """the chain folded (shallow: no HBM stack), then unfolded (depth 40: the HBM overflow stack appears), on ONE handle; VPT_DEBUG's
    stack line of each rebuild shows the HBM part going 0 -> > 0, and the renders take the spilled variant from then on"""
    monkeypatch.setenv("VPT_DEBUG", "1")
    case = R.CASES["chain_unfold"]
    file = case.path(tmp_path)
    A = vpt.DeviceScene(vpt.HostScene(file), 0)
    host = vpt.HostScene(file)
    spills = []

    def rebuild(what):
        capfd.readouterr()
        A.rebuild_bvh(what)
        spills.append(int(re.findall(r"in LDS \+ (\d+) in HBM", capfd.readouterr().err)[-1]))
        assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, case, f"step {len(spills)}", n_rays=4000)

    counts = [A.get_bvh_counts()[1]]
    for edit, shapes in case.steps:
        edit(host)
        A.update_lights(host.update_lights())
        rebuild(host.rebuild_bvh(shapes, True))
        counts.append(A.get_bvh_counts()[1])
    assert spills[0] == 0 and spills[1] > 0, spills
    assert counts[1] < counts[0] == counts[2], counts


@pytest.mark.parametrize("switch", ["VPT_NO_GROUP_FORMS=1", "VPT_STACK_LDS=4", "VPT_NO_COMPACT_TRIANGLES=1"])
def test_ab_switches_give_the_same_bits(switch):
    """the switches are read when a scene is created or rebuilt: in a child process, as the existing tests of such switches do"""
    key, value = switch.split("=")
    env = dict(os.environ, **{key: value})
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", f"{__file__}::test_rebuild_equals_a_fresh_scene[vol_times2]",
                        f"{__file__}::test_rebuild_equals_a_fresh_scene[chain_unfold]"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_multi_rebuild_on_virtual_ranks(vpt, tmp_path):
    case = R.CASES["vol_times2"]
    file = case.path(tmp_path)
    M = vpt.MultiDeviceScene(vpt.HostScene(file), [0, 0])
    host = vpt.HostScene(file)
    R.apply(host, case, after_edit=M.update_lights, after_rebuild=M.rebuild_bvh)
    B = vpt.DeviceScene(host, 0)
    p = vpt.PathtraceParams(resolution=64, samples=4, shader="volpathtrace", bounces=8)
    want, got = host.make_state(p), host.make_state(p)
    B.pathtrace_samples(want, p, 4)
    M.pathtrace_samples(got, p, 4)
    assert same_state(got, want)
    with pytest.raises(vpt.VptError):
        M.rebuild_bvh(vpt.BvhRebuild((99,), True))
    M.close()


def test_session_rebuild(vpt, tmp_path):
    """the display after rebuild_bvh + N samples equals a fresh session's"""
    case = R.CASES["curves_twist"]
    file = case.path(tmp_path)
    host = vpt.HostScene(file)
    p = vpt.PathtraceParams(resolution=96, samples=4, shader="pathtrace", bounces=4)
    session = vpt.RenderSession(vpt.DeviceScene(vpt.HostScene(file), 0), p, pratio=8)
    session.advance(2)
    R.apply(host, case, after_edit=session.edit_lights, after_rebuild=session.rebuild_bvh)
    assert session.samples == 0
    session.advance(3)
    fresh = vpt.RenderSession(vpt.DeviceScene(host, 0), p, pratio=8)
    fresh.advance(3)
    assert same_state(session.state(), fresh.state())
    assert np.array_equal(session.display(), fresh.display())
    with pytest.raises(vpt.VptError):
        session.rebuild_bvh(vpt.BvhRebuild((2, 2), True))
    assert session.samples == 3 and same_state(session.state(), fresh.state())
    session.close(), fresh.close()


def test_refusals_leave_the_scene_untouched(vpt, tmp_path):
    case = R.CASES["vol_times2"]
    host = vpt.HostScene(case.path(tmp_path))
    A = vpt.DeviceScene(host, 0)
    before = [render(vpt, A, host, case, s) for s in MESH_SHADERS]
    trees = [x.tobytes() for x in A.get_bvh() + A.get_bvh_prims()]
    for what in (vpt.BvhRebuild((host.count("shapes"),), True), vpt.BvhRebuild((-1,), False), vpt.BvhRebuild((1, 0, 1), True)):
        with pytest.raises(vpt.VptError):
            A.rebuild_bvh(what)
    abi = vpt.VptBvhRebuild(2, None, 1)
    assert vpt.hip.vpt_scene_rebuild_bvh(A.handle, C.byref(abi)) == -1 and b"null" in vpt.hip.vpt_last_error()
    assert vpt.hip.vpt_scene_rebuild_bvh(A.handle, None) == -1
    assert [x.tobytes() for x in A.get_bvh() + A.get_bvh_prims()] == trees
    assert all(same_state(render(vpt, A, host, case, s), b) for s, b in zip(MESH_SHADERS, before))
    A.rebuild_bvh(vpt.BvhRebuild((), False))   # valid, and nothing to do
    assert [x.tobytes() for x in A.get_bvh() + A.get_bvh_prims()] == trees
    # a rebuild of the unedited scene reproduces creation's trees
    A.rebuild_bvh(vpt.BvhRebuild(range(host.count("shapes")), True))
    assert [x.tobytes() for x in A.get_bvh() + A.get_bvh_prims()] == trees
    assert all(same_state(render(vpt, A, host, case, s), b) for s, b in zip(MESH_SHADERS, before))


def test_a_tree_past_the_stack_limit_is_refused_and_the_scene_stays(vpt, tmp_path):
    """258 unshared triangles as a blob (shallow), then moved into a chain 254 levels deep: the binary walk would need
    (0 + 2) + (254 + 2) = 258 > 256 stack entries, the limit vpt_scene_create refuses scenes at (tests/test_traversal_depth.py).  The
    rebuild is refused with VPT_ERR_UNSUPPORTED after everything was built - and nothing of the scene has changed: the refitted
    trees, the primitive orders and the renders are what they were, and a rebuild that fits still works afterwards."""
    import synth_scenes
    depth = 254
    chain, faces = synth_scenes.chain_geometry(depth)
    w = synth_scenes._Writer(str(tmp_path))
    shape = w.shape("chain", np.asarray(synth_scenes._blob(np.random.default_rng(3), len(faces))[0], np.float32), faces)
    floor = w.shape("floor", [[-4, -1.5, -4], [4, -1.5, -4], [4, -1.5, 4], [-4, -1.5, 4]], [[0, 1, 2], [0, 2, 3]])
    identity = np.concatenate([np.eye(3).reshape(-1), [0, 0, 0]])
    w.instance(floor, identity, 0), w.instance(shape, identity, 1)
    file, _ = w.write("blob", synth_scenes._look_at([-2.2, -1.8, -2.6], [0.3, 0.3, 0.3]))
    case = R.Case(file, [])
    host = vpt.HostScene(file)
    A = vpt.DeviceScene(vpt.HostScene(file), 0)
    host.set_shape_positions(shape, chain)
    A.update(host.update_bvh())
    B = vpt.DeviceScene(host, 0)   # the refitted scene: what A must stay
    before = [x.tobytes() for x in A.get_bvh() + A.get_bvh_prims()]
    abi, keep = vpt.BvhRebuild((shape,), True).to_abi()
    assert vpt.hip.vpt_scene_rebuild_bvh(A.handle, C.byref(abi)) == -5, vpt.hip.vpt_last_error().decode()
    assert b"traversal stack" in vpt.hip.vpt_last_error()
    assert [x.tobytes() for x in A.get_bvh() + A.get_bvh_prims()] == before
    for shader in ("pathtrace", "normal"):
        assert same_state(render(vpt, A, host, case, shader), render(vpt, B, host, case, shader)), shader
    A.rebuild_bvh(vpt.BvhRebuild((floor,), True))
    assert [x.tobytes() for x in A.get_bvh() + A.get_bvh_prims()] == before
