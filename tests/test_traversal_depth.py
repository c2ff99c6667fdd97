"""BVH traversal (vpt_mesh_kernel.hip.h: traverse()) on the scenes of tests/synth_scenes.py and on the golden ones, under the switches that
change how the walk is organised but must not change a bit: VPT_STACK_LDS=4 (four stack entries per lane in LDS, every deeper one in the
per-launch HBM array: lane_stack2<true>'s checked push / store / load, the `room_for` shortcuts, the helper lanes' stores into their owner's
column) and VPT_NO_GROUP_FORMS=1 (every ray in its own lane), each alone and both together.  Both are read when a scene handle is created.

  * intersect: ids and uvt bit for bit equal to the oracle's intersect_bvh, dense waves and waves of 12 / 3 / 1 rays (group forms from a
    ray's first node), whole-scene and single-instance queries: more than 16 instances (phase C's own root-box tests), a shape BVH 40
    levels deep, the deepest scene BVH the reference walks (124 levels); and, held to the own form's bits because the reference's
    128-entry stack cannot walk them, a scene BVH whose line rays enter their instances at stack depth 257 (the pop floor the group form
    hands to its helper lanes no longer fits 8 bits) and the deepest scene the create-time limit accepts;
  * renders: spilled against unspilled stacks, bit for bit, batched and unbatched; one crowd render against the reference;
  * the limit: one entry past it is refused with VPT_ERR_UNSUPPORTED, and the next scene is created as usual."""
import os
import re

import numpy as np
import pytest

import synth_scenes as ss
from conftest import GOLDEN
from kat_lib import edge_rays
from test_gpu_parity import _check_against_reference, _scene_of_triangles

pytestmark = pytest.mark.gpu

SETTINGS = {
    "default": {},
    "lds4": {"VPT_STACK_LDS": "4"},
    "own": {"VPT_NO_GROUP_FORMS": "1"},
    "lds4+own": {"VPT_STACK_LDS": "4", "VPT_NO_GROUP_FORMS": "1"},
}
FAR = np.float32([1e3, 1e3, 1e3, 0.57735027, 0.57735027, 0.57735027])   # misses every scene here: its lane finishes at once
N_RAYS = 20000


def _device(vpt, monkeypatch, scene, env):
    for k in ("VPT_STACK_LDS", "VPT_NO_GROUP_FORMS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return vpt.DeviceScene(scene, 0)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _batches(rays):
    """dense waves, then waves that keep 12 / 3 / 1 of their 64 rays (the others miss the scene)"""
    lane = np.arange(len(rays)) % 64
    out = [("dense", rays, 64)]
    for keep in (12, 3, 1):
        sparse = rays.copy()
        sparse[(lane * 7 + 3) % 64 >= keep] = FAR
        out.append((f"{keep} per wave", sparse, keep))
    return out


def _intersect_everywhere(vpt, oracle, monkeypatch, scene, rays, instances, name, min_hit_share, deep=None):
    """every batch x query x setting against the oracle (oracle = None: against the own form with the default stack, for scenes the
    reference's 128-entry traversal stack cannot walk); returns {(batch, instance): reference ids}.  deep: (instance ids, minimum hits on
    them per whole-scene batch)"""
    devs = {k: _device(vpt, monkeypatch, scene, env) for k, env in SETTINGS.items()}
    out = {}
    for bname, batch, keep in _batches(rays):
        for inst in instances:
            rids, ruvt = oracle.oracle_intersect(scene, batch, inst) if oracle is not None else devs["own"].intersect(batch, inst)
            for sname, dev in devs.items():
                ids, uvt = dev.intersect(batch, inst)
                bad = np.nonzero((ids != rids).any(axis=1) | (uvt.view(np.uint32) != ruvt.view(np.uint32)).any(axis=1))[0]
                assert len(bad) == 0, (name, bname, inst, sname, len(bad), bad[:8].tolist(), ids[bad[:3]].tolist(), rids[bad[:3]].tolist())
            hits = int((rids[:, 0] >= 0).sum())
            real = len(batch) * keep // 64
            deep_hits = int(np.isin(rids[:, 0], deep[0]).sum()) if deep is not None and inst < 0 else None
            print(f"{name}: {bname}, instance {inst}: {hits} hits of {real} rays" + (f", {deep_hits} on the deepest instances" if deep_hits is not None else "")
                  + f"; equal bits under {', '.join(devs)}")
            if inst < 0 or keep == 64:
                assert hits >= min_hit_share[inst < 0] * real, (name, bname, inst, hits, real)
            if deep_hits is not None:
                assert deep_hits >= deep[1] * real, (name, bname, deep_hits, real)
            out[(bname, inst)] = rids
    return out


def _deepest_instance(f):
    return max(f["depth_of"], key=lambda i: (f["depth_of"][i], i))


@pytest.mark.parametrize("count", [17, 33, 200])
def test_intersect_crowds(vpt, oracle, monkeypatch, tmp_path, count):
    """more instances than VPT_HOIST_MAX (16) and than the 32 bits of `reach`: phase C tests each instance's root box"""
    path, f = ss.crowd_scene(tmp_path, count)
    scene = vpt.HostScene(path)
    rays = edge_rays(np.random.default_rng(count), (-1.3, -1.3, -1.3), (1.3, 1.3, 1.3), N_RAYS)
    _intersect_everywhere(vpt, oracle, monkeypatch, scene, rays, (-1, _deepest_instance(f)), f"crowd_{count}", {True: 0.2, False: 0.002})


def test_intersect_chain_shape(vpt, oracle, monkeypatch, tmp_path):
    """a shape BVH 40 levels deep: the worst case needs 41 stack entries, the HBM-overflow variant runs without an override"""
    path, f = ss.chain_scene(tmp_path, 40)
    scene = vpt.HostScene(path)
    rng = np.random.default_rng(40)
    rays = np.concatenate([ss.line_rays(rng, N_RAYS // 2), edge_rays(rng, (-1, -1, -1), (1, 1, 1), N_RAYS - N_RAYS // 2)])
    _intersect_everywhere(vpt, oracle, monkeypatch, scene, rays, (-1, 1), "chain_40", {True: 0.3, False: 0.3})


def _host_figures(capfd, vpt, monkeypatch, scene):
    """the loader's own BVH figures (VPT_DEBUG line of scene creation)"""
    capfd.readouterr()
    monkeypatch.setenv("VPT_DEBUG", "1")
    vpt.DeviceScene(scene, 0).close()
    monkeypatch.delenv("VPT_DEBUG")
    err = capfd.readouterr().err
    m = re.search(r"binary depth scene (\d+) shape (\d+); quad stack need scene (\d+) \+ shape (\d+)", err)
    assert m, err
    return tuple(int(g) for g in m.groups())


@pytest.mark.parametrize("levels,chain_depth,blocker", [(62, None, "shield"), (86, None, "shield"), (86, None, "decoy"), (86, 80, "shield")])
def test_intersect_deep_scene(vpt, oracle, monkeypatch, capfd, tmp_path, levels, chain_depth, blocker):
    """a scene BVH 2 * levels deep with three leaf siblings per quad level.  levels = 62: 124 binary levels, the deepest scene BVH the
    reference's intersect_bvh walks (its stack holds 128 nodes per level), against the oracle.  levels = 86: rays along the line of instances
    enter the innermost ones at stack depth 257, past the 8 bits the group form of the node phase once carried a ray's pop floor in; the
    reference cannot walk this scene, so every setting is held to the own form's bits.  With chain_depth = 80 the binary need is exactly the
    create-time limit (256) and the innermost leaf holds an instance of an 80-level chain shape as well.  The shield of the innermost leaf
    is every line ray's nearest hit (the rays reached that leaf); the decoy is entered and missed (a line ray's group pops from the shape
    level back into the scene entries under its floor, and the nearest hit is in one of them)"""
    path, f = ss.deep_scene(tmp_path, levels=levels, chain_depth=chain_depth, blocker=blocker)
    scene = vpt.HostScene(path)
    assert _host_figures(capfd, vpt, monkeypatch, scene) == (f["scene_depth"], f["max_shape_depth"], f["scene_need4"], f["max_shape_need4"])
    assert f["line_entry_sp"] >= (256 if levels == 86 else 185)
    with_oracle = f["scene_depth"] + 1 <= ss.REFERENCE_STACK
    assert with_oracle == (levels == 62)
    rng = np.random.default_rng(86)
    rays = np.concatenate([ss.line_rays(rng, 3 * N_RAYS // 4), edge_rays(rng, (-0.3, -0.3, -0.3), (0.6, 0.6, 0.6), N_RAYS - 3 * N_RAYS // 4)])
    _intersect_everywhere(vpt, oracle if with_oracle else None, monkeypatch, scene, rays, (-1, f["deepest"][0]),
                          f"deep_{levels}{'' if chain_depth is None else f'+chain_{chain_depth}'}, {blocker} (line rays enter at stack depth {f['line_entry_sp']})",
                          {True: 0.5, False: 0.2}, deep=(f["deepest"], 0.3) if blocker == "shield" else None)


@pytest.mark.parametrize("scene_file,lo,hi", [
    ("03_volume/volume.json", (-0.7, -0.05, -0.45), (0.7, 0.45, 0.45)),
    ("05_head1ss_sub/head1ss_sub.json", (-0.25, -0.1, -0.25), (0.25, 0.4, 0.25)),
    ("triangles", (-0.7, -0.05, -0.3), (0.7, 0.35, 0.3)),
])
def test_intersect_golden_scenes_under_every_setting(vpt, oracle, monkeypatch, tmp_path, scene_file, lo, hi):
    path = _scene_of_triangles(tmp_path) if scene_file == "triangles" else os.path.join(GOLDEN, "scenes", scene_file)
    scene = vpt.HostScene(path)
    rays = edge_rays(np.random.default_rng(17), lo, hi, N_RAYS)
    _intersect_everywhere(vpt, oracle, monkeypatch, scene, rays, (-1, 3 if scene_file == "triangles" else 0), scene_file,
                          {True: 0.02 if scene_file == "triangles" else 0.05, False: 0.0})


def test_the_limit(vpt, oracle, tmp_path):
    """one binary stack entry past the limit is refused as unsupported (its message names the real bound); the next scene is created and
    intersects as usual"""
    path, f = ss.deep_scene(tmp_path / "past", chain_depth=81)
    assert f["need"] == ss.STACK_LIMIT + 1
    with pytest.raises(vpt.VptError, match=r"BVH depth 257 .* needs a 260-entry traversal stack; the LDS stack holds 256"):
        vpt.DeviceScene(vpt.HostScene(path), 0)
    scene = vpt.HostScene(ss.chain_scene(tmp_path / "next", 40)[0])
    dev = vpt.DeviceScene(scene, 0)
    rays = ss.line_rays(np.random.default_rng(1), 4096)
    ids, uvt = dev.intersect(rays)
    rids, ruvt = oracle.oracle_intersect(scene, rays)
    assert np.array_equal(ids, rids) and np.array_equal(uvt.view(np.uint32), ruvt.view(np.uint32))
    assert (ids[:, 0] >= 0).mean() > 0.5


def _scene_for(vpt, which, tmp_path):
    if which == "crowd":
        return vpt.HostScene(ss.crowd_scene(tmp_path, 33)[0])
    return vpt.HostScene(os.path.join(GOLDEN, "scenes", {"03": "03_volume/volume.json", "head": "05_head1ss_sub/head1ss_sub.json"}[which]))


@pytest.mark.parametrize("which,shader,res,bounces,spp", [
    ("crowd", "pathtrace", 128, 6, 4),
    ("crowd", "volpathtrace", 128, 16, 4),
    ("03", "volpathtrace", 160, 64, 4),
    ("03", "pathtrace", 160, 8, 4),
    ("head", "volpathtrace", 128, 64, 4),       # compact records: vpt_mesh_kernel<K, true, SMALL_LIGHTS | COMPACT_TRIS>
    ("head", "pathtrace", 128, 8, 4),
])
def test_spilled_stacks_do_not_change_a_bit(vpt, monkeypatch, tmp_path, which, shader, res, bounces, spp):
    """VPT_STACK_LDS=4: everything past four stack entries per lane lives in HBM.  The frame must come out bit for bit as with the default
    stack - radiance sums, hit counts, RNG streams - in one call and in 1 + (spp - 1)"""
    scene = _scene_for(vpt, which, tmp_path)
    p = vpt.PathtraceParams(resolution=res, samples=1 << 20, shader=shader, bounces=bounces)
    plain = _device(vpt, monkeypatch, scene, {})
    spilled = _device(vpt, monkeypatch, scene, {"VPT_STACK_LDS": "4"})
    for first in (spp, 1):
        a, b = scene.make_state(p), scene.make_state(p)
        plain.pathtrace_samples(a, p, spp)
        spilled.pathtrace_samples(b, p, first)
        if first < spp:
            spilled.pathtrace_samples(b, p, spp - first)
        assert a.samples == b.samples == spp
        assert np.array_equal(a.image.view(np.uint32), b.image.view(np.uint32)) and np.array_equal(a.rngs, b.rngs) and np.array_equal(a.hits, b.hits)
        assert a.hits.sum() > 0
    if which == "head":
        assert plain.record_bytes() == (48, 64)


def test_crowd_render_matches_the_reference(vpt, oracle, tmp_path):
    """33 instances with both kinds of emissive instances (the mesh-light pdf walk through the traversal for the large one) against the
    oracle, with the strict check of test_gpu_parity"""
    scene = _scene_for(vpt, "crowd", tmp_path)
    spp = 4
    p = vpt.PathtraceParams(resolution=96, samples=spp, shader="pathtrace", bounces=4)
    g = scene.make_state(p)
    ref = g.copy()
    vpt.DeviceScene(scene, 0).pathtrace_samples(g, p, spp)
    oracle.oracle_render(scene, p, ref, spp, nthreads=0)
    _check_against_reference(oracle, scene, p, spp, g, ref.image, ref.rngs, "crowd_33 path_96_4", 0.998, 0.998, 0.998)
