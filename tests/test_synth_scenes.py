"""What the synthetic scenes of tests/synth_scenes.py promise (the GPU tests in test_traversal_depth.py rely on it): instance counts on
either side of the traversal's 16-instance hoist and 32-bit reach mask, shape and scene BVHs deep enough for the HBM part of the stack and
for the 8-bit pop floor the group form used to carry, and the create-time limit on either side.  CPU only: the host BVH build, and the
library's scene preparation, which vpt_scene_create runs in full before it looks for a device."""
import ctypes as C
import re

import pytest

import synth_scenes as ss

VPT_ERR_INVALID_ARG, VPT_ERR_NO_DEVICE, VPT_ERR_UNSUPPORTED = -1, -2, -5


def _prepare(vpt, capfd, monkeypatch, path):
    """vpt_scene_create on device -1, which no machine has: the scene is prepared (and refused if past a limit) before the call looks for a
    device.  Returns (code, message, the library's BVH figures from its VPT_DEBUG line or None)"""
    scene = vpt.HostScene(path)
    capfd.readouterr()
    monkeypatch.setenv("VPT_DEBUG", "1")
    out = C.c_void_p()
    rc = vpt.hip.vpt_scene_create(scene.desc, -1, C.byref(out))
    monkeypatch.delenv("VPT_DEBUG")
    m = re.search(r"binary depth scene (\d+) shape (\d+); quad stack need scene (\d+) \+ shape (\d+)", capfd.readouterr().err)
    return rc, vpt.hip.vpt_last_error().decode(), tuple(int(g) for g in m.groups()) if m else None


def _check_figures(vpt, capfd, monkeypatch, path, f):
    """the library's figures are the model's (synth_scenes.bvh_depth / quad_need); refused for want of a device only"""
    rc, msg, figures = _prepare(vpt, capfd, monkeypatch, path)
    assert rc in (VPT_ERR_NO_DEVICE, VPT_ERR_INVALID_ARG), msg
    assert figures == (f["scene_depth"], f["max_shape_depth"], f["scene_need4"], f["max_shape_need4"])


def test_quad_need_and_depth_of_small_trees(vpt):
    import numpy as np
    # one box: a leaf root; eight boxes in a row: split in halves down to leaves of <= 4 (depth 1, one quad level with two leaves)
    one, _ = vpt.build_bvh(np.float32([[0, 0, 0, 1, 1, 1]]), device=None)
    assert ss.bvh_depth(one) == 0 and ss.quad_need(one) == 0
    row = np.float32([[i, 0, 0, i + 0.5, 1, 1] for i in range(8)])
    nodes, _ = vpt.build_bvh(row, device=None)
    assert ss.bvh_depth(nodes) == 1 and ss.quad_need(nodes) == 1
    # 16 boxes: two binary levels below the root, four leaves of four: one quad level with four slots
    nodes, _ = vpt.build_bvh(np.float32([[i, 0, 0, i + 0.5, 1, 1] for i in range(16)]), device=None)
    assert ss.bvh_depth(nodes) == 2 and ss.quad_need(nodes) == 3
    assert max(ss.line_entry_depths(nodes).values()) == 3


@pytest.mark.parametrize("count", [17, 33, 200])
def test_crowd_scenes(vpt, capfd, monkeypatch, tmp_path, count):
    path, f = ss.crowd_scene(tmp_path, count)
    print(f"crowd_{count}: scene depth {f['scene_depth']}, scene need4 {f['scene_need4']}, largest leaf {f['max_leaf']}, "
          f"shape depths {f['shape_depth']}, frames {f['frame_kinds']}")
    assert f["instances"] == count > ss.HOIST_MAX
    assert f["max_leaf"] == 4                                   # overlapping instances: scene leaves of four
    assert all(n > 0 for n in f["frame_kinds"].values())        # identity, translation, rotation, non-uniform scale, mirrored
    assert 0 in f["shape_depth"] and max(f["shape_depth"]) >= 4  # single-leaf shapes and shapes with real BVHs
    assert len(f["lights"]) == 2
    assert f["need"] <= ss.STACK_LIMIT
    scene = vpt.HostScene(path)                                 # the loader takes it
    assert scene.desc
    _check_figures(vpt, capfd, monkeypatch, path, f)


def test_chain_shape_spills_without_an_override(vpt, capfd, monkeypatch, tmp_path):
    path, f = ss.chain_scene(tmp_path, 40)
    print(f"chain: shape depth {f['shape_depth'][f['chain']]}, shape need4 {f['shape_need4'][f['chain']]}, need4 {f['need4']}")
    assert f["shape_depth"][f["chain"]] == 40                   # one primitive peeled per level
    assert f["need4"] > 24                                      # more than the LDS part holds (vpt_scene_prep.cpp: 22 in LDS, the rest in HBM)
    _check_figures(vpt, capfd, monkeypatch, path, f)


def test_deep_scene_passes_the_8_bit_floor_under_the_limit(vpt, capfd, monkeypatch, tmp_path):
    path, f = ss.deep_scene(tmp_path / "deep")
    print(f"deep: {f['instances']} instances, scene depth {f['scene_depth']}, scene need4 {f['scene_need4']}, max shape depth "
          f"{f['max_shape_depth']}, need {f['need']}, line rays enter the innermost leaf at stack depth {f['line_entry_sp']}")
    assert f["scene_need4"] >= 256 and f["line_entry_sp"] >= 256
    assert f["need"] <= ss.STACK_LIMIT
    assert all(f["depth_of"][i] == f["scene_depth"] - 1 for i in f["deepest"])
    assert f["scene_depth"] + 1 > ss.REFERENCE_STACK             # outside what the reference's traversal walks: GPU tests compare forms
    _check_figures(vpt, capfd, monkeypatch, path, f)
    # the deepest the reference walks: 124 binary levels, three leaf siblings per quad level
    path, f = ss.deep_scene(tmp_path / "ref", levels=62)
    print(f"deep_62: scene depth {f['scene_depth']}, scene need4 {f['scene_need4']}, line entry {f['line_entry_sp']}")
    assert f["scene_depth"] + 1 <= ss.REFERENCE_STACK and f["scene_need4"] >= 185
    _check_figures(vpt, capfd, monkeypatch, path, f)


@pytest.mark.parametrize("chain_depth,accepted", [(80, True), (81, False)])
def test_deep_scene_on_either_side_of_the_limit(vpt, capfd, monkeypatch, tmp_path, chain_depth, accepted):
    path, f = ss.deep_scene(tmp_path, chain_depth=chain_depth)
    print(f"deep + chain {chain_depth}: need {f['need']}, scene need4 {f['scene_need4']}, need4 {f['need4']}")
    assert f["scene_need4"] >= 256 and f["line_entry_sp"] >= 256
    assert f["need"] == (ss.STACK_LIMIT if accepted else ss.STACK_LIMIT + 1)
    if accepted:
        _check_figures(vpt, capfd, monkeypatch, path, f)
    else:   # refused on any machine, before a device is looked for (test_traversal_depth.py: test_the_limit)
        rc, msg, _ = _prepare(vpt, capfd, monkeypatch, path)
        assert rc == VPT_ERR_UNSUPPORTED
        assert re.search(r"BVH depth 257 .* needs a 260-entry traversal stack; the LDS stack holds 256", msg), msg
