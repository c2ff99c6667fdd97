"""What the synthetic scenes of tests/synth_scenes.py promise (the GPU tests in test_traversal_depth.py rely on it): instance counts on
either side of the traversal's 16-instance hoist and 32-bit reach mask, shape and scene BVHs deep enough for the HBM part of the stack and
for the 8-bit pop floor the group form used to carry, and the create-time limit on either side.  CPU only: the host BVH build."""
import pytest

import synth_scenes as ss


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
def test_crowd_scenes(vpt, tmp_path, count):
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


def test_chain_shape_spills_without_an_override(vpt, tmp_path):
    path, f = ss.chain_scene(tmp_path, 40)
    print(f"chain: shape depth {f['shape_depth'][f['chain']]}, shape need4 {f['shape_need4'][f['chain']]}, need4 {f['need4']}")
    assert f["shape_depth"][f["chain"]] == 40                   # one primitive peeled per level
    assert f["need4"] > 24                                      # more than the LDS part holds (vpt_capi.hip: 22 in LDS, the rest in HBM)
    vpt.HostScene(path)


def test_deep_scene_passes_the_8_bit_floor_under_the_limit(vpt, tmp_path):
    path, f = ss.deep_scene(tmp_path / "deep")
    print(f"deep: {f['instances']} instances, scene depth {f['scene_depth']}, scene need4 {f['scene_need4']}, max shape depth "
          f"{f['max_shape_depth']}, need {f['need']}, line rays enter the innermost leaf at stack depth {f['line_entry_sp']}")
    assert f["scene_need4"] >= 256 and f["line_entry_sp"] >= 256
    assert f["need"] <= ss.STACK_LIMIT
    assert all(f["depth_of"][i] == f["scene_depth"] - 1 for i in f["deepest"])
    assert f["scene_depth"] + 1 > ss.REFERENCE_STACK             # outside what the reference's traversal walks: GPU tests compare forms
    vpt.HostScene(path)
    # the deepest the reference walks: 124 binary levels, three leaf siblings per quad level
    path, f = ss.deep_scene(tmp_path / "ref", levels=62)
    print(f"deep_62: scene depth {f['scene_depth']}, scene need4 {f['scene_need4']}, line entry {f['line_entry_sp']}")
    assert f["scene_depth"] + 1 <= ss.REFERENCE_STACK and f["scene_need4"] >= 185


@pytest.mark.parametrize("chain_depth,accepted", [(80, True), (81, False)])
def test_deep_scene_on_either_side_of_the_limit(vpt, tmp_path, chain_depth, accepted):
    path, f = ss.deep_scene(tmp_path, chain_depth=chain_depth)
    print(f"deep + chain {chain_depth}: need {f['need']}, scene need4 {f['scene_need4']}, need4 {f['need4']}")
    assert f["scene_need4"] >= 256 and f["line_entry_sp"] >= 256
    assert f["need"] == (ss.STACK_LIMIT if accepted else ss.STACK_LIMIT + 1)
