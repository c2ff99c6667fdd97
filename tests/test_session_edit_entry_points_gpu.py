"""The eight ways a render session edits its scene (include/vpt.h: vpt_session_edit, _edit_lights, _edit_textures, _edit_volumes,
vpt_session_rebuild_bvh_quality at both qualities, _edit_instances, _edit_shapes): each is the scene's own entry point, the accounting of
vpt_scene_update_stats, then a reset.  So after the call the session holds the state of a fresh session over a DeviceScene that was given
the same edit through DeviceScene.update_*, it has no samples, and stats() is what the entry point has always counted; an edit the scene
refuses leaves the session where it was.  The edits are the ones tests/test_edit_entry_points_gpu.py takes from the tests/*_edits.py
tables: 03_volume for the mesh-side edits, 06_gridsdf_synth for the volumes."""
import os

import numpy as np
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


# Every edit(vpt, host, work, session, dev) changes `host` and hands each edit object it makes to the session first - noting stats()
# before any other call on the session - and then to `dev`, the plain DeviceScene the session is compared with.
def both(session, dev, session_call, dev_call, seen):
    def give(edit):
        getattr(session, session_call)(edit)
        seen.append(session.stats())
        getattr(dev, dev_call)(edit)
    return give


def _edit(vpt, host, work, session, dev, seen):
    E.PINNED["vol_inst1_x001"][1](host)
    both(session, dev, "edit", "update", seen)(host.update_bvh())


def _edit_lights(vpt, host, work, session, dev, seen):
    L.CASES["vol_arealight1_off"][1](host)
    both(session, dev, "edit_lights", "update_lights", seen)(host.update_lights())


def _edit_textures(vpt, host, work, session, dev, seen):
    T.apply(vpt, "sky_13x5", host, work, after_step=both(session, dev, "edit_textures", "update_textures", seen))


def _edit_volumes(vpt, host, work, session, dev, seen):
    V.apply(vpt, "region_one_grid", host, work, after_step=both(session, dev, "edit_volumes", "update_volumes", seen))


def _rebuild_bvh(quality):
    def edit(vpt, host, work, session, dev, seen):
        step, shapes = R.CASES["vol_last_y005"].steps[0]
        step(host)
        both(session, dev, "edit_lights", "update_lights", seen)(host.update_lights())
        rebuild = host.rebuild_bvh(R.shapes_of(host, shapes), True, quality=getattr(vpt, quality))
        both(session, dev, "rebuild_bvh", "rebuild_bvh", seen)(rebuild)
    return edit


def _edit_instances(vpt, host, work, session, dev, seen):
    I.apply(host, I.CASES["vol_add_remove"], after=both(session, dev, "edit_instances", "update_instances", seen))


def _edit_shapes(vpt, host, work, session, dev, seen):
    S.apply(host, S.CASES["vol_lamp"], after_shapes=both(session, dev, "edit_shapes", "update_shapes", seen),
            after_instances=both(session, dev, "edit_instances", "update_instances", seen))


def _texels():
    return np.zeros((1, 2, 4), np.uint8)


# entry point -> (scene file, shader, the small edit, the edit with an id out of range: refused(vpt, host, session),
#                 stats() = (kernel launches, bytes to the device, bytes to the host) right after the last session call of the edit)
# The triples were observed on the commit before session_edit() took its entry point as a callable.
ENTRY_POINTS = {
    "edit": (I.S03, "volpathtrace", _edit, lambda vpt, h, s: s.edit(vpt.SceneEdit(cameras={99: h.camera(0)})), (13, 112, 72)),
    "edit_lights": (I.S03, "volpathtrace", _edit_lights, lambda vpt, h, s: s.edit_lights(vpt.SceneEdit(materials={999: h.material(0)})), (7, 252, 72)),
    "edit_textures": (I.S03, "volpathtrace", _edit_textures, lambda vpt, h, s: s.edit_textures(vpt.TextureEdit(textures={999: (_texels(), False)})), (11, 1496, 72)),
    "edit_volumes": (V.GRID, "implicit", _edit_volumes,
                     lambda vpt, h, s: s.edit_volumes(vpt.VolumeEdit(vol_instances={99: h.volume_instance(0)})), (7, 764, 76)),
    "rebuild_bvh_middle": (I.S03, "volpathtrace", _rebuild_bvh("BVH_MIDDLE"),
                           lambda vpt, h, s: s.rebuild_bvh(vpt.BvhRebuild((999,), True, quality=vpt.BVH_MIDDLE)), (43, 249248, 72)),
    "rebuild_bvh_sah": (I.S03, "volpathtrace", _rebuild_bvh("BVH_SAH"),
                        lambda vpt, h, s: s.rebuild_bvh(vpt.BvhRebuild((999,), True, quality=vpt.BVH_SAH)), (62, 249440, 72)),
    "edit_instances": (I.S03, "volpathtrace", _edit_instances, lambda vpt, h, s: s.edit_instances(vpt.InstanceEdit(remove=(999,))), (46, 1664, 72)),
    "edit_shapes": (I.S03, "volpathtrace", _edit_shapes, lambda vpt, h, s: s.edit_shapes(vpt.ShapeEdit(remove=(999,))), (64, 2312, 72)),
}


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_a_session_edit_is_the_scene_edit_and_a_reset(vpt, tmp_path, name):
    scene_file, shader, edit, refused, expected = ENTRY_POINTS[name]
    params = vpt.PathtraceParams(resolution=32, samples=1, shader=shader, bounces=4)
    host = vpt.HostScene(scene_path(scene_file))
    dev = vpt.DeviceScene(vpt.HostScene(scene_path(scene_file)), 0)
    session = vpt.RenderSession(vpt.DeviceScene(vpt.HostScene(scene_path(scene_file)), 0), params, pratio=4)
    session.advance(1)
    assert session.samples == 1
    seen = []
    edit(vpt, host, tmp_path, session, dev, seen)
    print(f"{name}: stats() after each session call of the edit: {seen}", flush=True)
    assert session.samples == 0, f"{name}: the edit did not reset the session"
    fresh = vpt.RenderSession(dev, params, pratio=4)
    assert same_state(session.state(), fresh.state()), f"{name}: the session's state is not that of a fresh session over the edited scene"
    session.advance(1), fresh.advance(1)
    assert same_state(session.state(), fresh.state()), f"{name}: the session renders another picture than a fresh one over the edited scene"
    # an edit the scene refuses: nothing changes, here or there
    before = session.state()
    with pytest.raises(vpt.VptError):
        refused(vpt, host, session)
    assert session.samples == 1 and same_state(session.state(), before), f"{name}: a refused edit changed the session"
    fresh.close(), session.close()
    assert seen[-1] == expected, f"{name}: stats() after the edit"
