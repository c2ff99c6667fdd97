"""The seven ways to edit a resident scene (include/vpt.h: vpt_scene_update, _update_lights, _update_textures, _update_volumes,
vpt_scene_rebuild_bvh, _update_instances, _update_shapes) on an EMPTY edit that follows a non-empty one of the same family: the
tables and the picture stay, and the counters of vpt_scene_update_stats are kept or reset as each entry point has always done.
The non-empty edits are cases of the tests/*_edits.py tables; 03_volume for the mesh-side edits, 06_gridsdf_synth for the volumes."""
import os

import pytest

import instance_edits as I
import light_edits as L
import rebuild_edits as R
import scene_edits as E
import shape_edits as S
import texture_edits as T
import volume_edits as V
from conftest import GOLDEN
from test_scene_update_gpu import same_state

pytestmark = pytest.mark.gpu


def scene_path(scene_file):
    return os.path.join(GOLDEN, "scenes", scene_file)


# entry point -> (scene file, shader of the render, the small edit(vpt, host, dev, work), the empty edit(vpt, dev),
#                 update_stats()[:2] after the empty edit)
# The pairs (launches, bytes) were observed on the commit before all seven went through one edit_scene().  The four older entry
# points start the counters again on an empty edit (an empty volume edit still sends the SDF records made from the resident tables:
# 736 bytes on this scene); the three that replace trees or lists return before they touch them, so theirs are the pairs of the
# case that ran before: 37 launches of vol_last_y005's rebuild, 40 of vol_add_remove, 58 of vol_lamp.
def _update(vpt, host, dev, work):
    E.PINNED["vol_inst1_x001"][1](host)
    dev.update(host.update_bvh())


def _update_lights(vpt, host, dev, work):
    L.CASES["vol_arealight1_off"][1](host)
    dev.update_lights(host.update_lights())


def _update_textures(vpt, host, dev, work):
    T.apply(vpt, "sky_13x5", host, work, after_step=dev.update_textures)


def _update_volumes(vpt, host, dev, work):
    V.apply(vpt, "region_one_grid", host, work, after_step=dev.update_volumes)


def _rebuild_bvh(vpt, host, dev, work):
    R.apply(host, R.CASES["vol_last_y005"], after_edit=dev.update_lights, after_rebuild=dev.rebuild_bvh)


def _update_instances(vpt, host, dev, work):
    I.apply(host, I.CASES["vol_add_remove"], after=dev.update_instances)


def _update_shapes(vpt, host, dev, work):
    S.apply(host, S.CASES["vol_lamp"], after_shapes=dev.update_shapes, after_instances=dev.update_instances)


ENTRY_POINTS = {
    "update": (I.S03, "volpathtrace", _update, lambda vpt, dev: dev.update(vpt.SceneEdit()), (0, 0)),
    "update_lights": (I.S03, "volpathtrace", _update_lights, lambda vpt, dev: dev.update_lights(vpt.SceneEdit()), (0, 0)),
    "update_textures": (I.S03, "volpathtrace", _update_textures, lambda vpt, dev: dev.update_textures(vpt.TextureEdit()), (0, 0)),
    "update_volumes": (V.GRID, "implicit", _update_volumes, lambda vpt, dev: dev.update_volumes(vpt.VolumeEdit()), (0, 736)),
    "rebuild_bvh": (I.S03, "volpathtrace", _rebuild_bvh, lambda vpt, dev: dev.rebuild_bvh(vpt.BvhRebuild((), False)), (37, 249248)),
    "update_instances": (I.S03, "volpathtrace", _update_instances, lambda vpt, dev: dev.update_instances(vpt.InstanceEdit()), (40, 1664)),
    "update_shapes": (I.S03, "volpathtrace", _update_shapes, lambda vpt, dev: dev.update_shapes(vpt.ShapeEdit()), (58, 2312)),
}


def snapshot(vpt, dev, host, shader):
    p = vpt.PathtraceParams(resolution=32, samples=1, shader=shader, bounces=4)
    st = host.make_state(p)
    dev.pathtrace_samples(st, p, 1)
    return (dev.light_tables_hash(), dev.instance_tables_hash(), dev.shape_tables_hash()), st


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_empty_edit_after_an_edit(vpt, tmp_path, name):
    scene_file, shader, edit, empty, expected = ENTRY_POINTS[name]
    host = vpt.HostScene(scene_path(scene_file))
    dev = vpt.DeviceScene(vpt.HostScene(scene_path(scene_file)), 0)
    edit(vpt, host, dev, tmp_path)
    before = dev.update_stats()[:2]
    hashes, picture = snapshot(vpt, dev, host, shader)
    assert before[0] > 0 and before[1] > 0, f"{name}: the edit before the empty one launched or sent nothing: {before}"
    empty(vpt, dev)
    after = dev.update_stats()[:2]
    print(f"{name}: (launches, bytes) {before} after the edit, {after} after the empty one", flush=True)
    again, picture_again = snapshot(vpt, dev, host, shader)
    assert again == hashes, f"{name}: an empty edit changed a table"
    assert same_state(picture_again, picture), f"{name}: an empty edit changed the picture"
    assert after == expected, f"{name}: the counters after an empty edit"
