"""The host side of vpt_scene_update_volume_set: HostScene.add_volume / remove_volumes / add_volume_instance /
remove_volume_instances / add_sdf / remove_sdfs / update_volume_set(), the mirror over a scene whose implicit side was changed through
them, against the same scene loaded afresh from an edited scene file with its .sdf files (descriptor tables byte for byte), against the
reference's own render of six of those files (tests/golden/volume_set_states.npz, written by tests/golden/make_volume_set_fixtures.py)
through the oracle; the structs and the packing of VolumeSetEdit, the ledger's ordering rules, the lazy bake.  No device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import volume_edits as V
import volume_set_edits as W
from bake_meshes import bits
from conftest import GOLDEN
from test_volume_update_host import implicit_tables

F = np.float32


def path(scene_file):
    return os.path.join(GOLDEN, "scenes", scene_file)


@pytest.fixture(scope="module")
def originals(vpt):
    return {scene_file: vpt.HostScene(path(scene_file)) for scene_file in (W.GRID, W.SDFS, W.CLOUD)}


def edited(vpt, name, originals):
    scene_file = W.scene_of(vpt, name)
    h = vpt.HostScene(path(scene_file))
    edits = []
    W.apply(vpt, name, h, after_step=lambda kind, e: edits.append((kind, e)), original=originals[scene_file])
    return scene_file, h, edits


@pytest.mark.parametrize("name", W.AS_SCENE_FILE)
def test_the_setters_equal_the_edited_scene_loaded_afresh(vpt, originals, tmp_path, name):
    """volumes, vol_instances, sdfs, every volume's voxels, lights and light_cdf of the descriptor, byte for byte"""
    scene_file, h, edits = edited(vpt, name, originals)
    assert all(not e.empty() for _, e in edits) and h.update_volume_set().empty()
    fresh = vpt.HostScene(W.write_edited_scene(vpt, name, tmp_path, originals[scene_file]))
    got, want = implicit_tables(vpt, h), implicit_tables(vpt, fresh)
    for part, a, b in zip(("volumes", "vol_instances", "sdfs", "voxels"), got, want):
        assert a == b, f"{name}: {part}"
    (lights, cdf), (want_lights, want_cdf) = h.lights(), fresh.lights()
    assert lights.tobytes() == want_lights.tobytes() and cdf.tobytes() == want_cdf.tobytes()
    assert h._lazy_bakes == []   # reading the descriptor ran the host mirror of a bake
    assert got != implicit_tables(vpt, originals[scene_file])


@pytest.mark.parametrize("tag", W.TAGS)
def test_a_zero_dimension_and_a_one_voxel_volume(vpt, originals, tag):
    """no file holds an empty grid, so the descriptor is held to the lists themselves"""
    scene_file, h, _ = edited(vpt, f"add_tiny_{tag}", originals)
    d = vpt.VptSceneDescImplicit.from_address(h.desc + vpt.VptSceneDescImplicit.OFFSET)
    vols = (vpt.VptVolume * d.num_volumes).from_address(d.volumes)
    assert [tuple(v.whd) for v in vols] == [(48, 48, 48), (40, 40, 40), (1, 1, 1), (4, 0, 3)]
    assert [v.offset for v in vols] == [0, 48 ** 3, 48 ** 3 + 40 ** 3, 48 ** 3 + 40 ** 3 + 1]
    assert bits(h.volume(2)[0]).tolist() == [[[int(np.array(0.25, F).view(np.uint32))]]] and h.volume(3)[0].shape == (3, 0, 4)
    assert h.volume_instance(h.count_implicit("vol_instances") - 1).volume == 2
    for k in (0, 1):
        assert np.array_equal(bits(h.volume(k)[0]), bits(originals[scene_file].volume(k)[0]))


def test_ids_close_up_and_the_lights_follow(vpt, originals):
    _, h, _ = edited(vpt, "light_shifts_sdfs", originals)
    assert [int(l["sdf"]) for l in h.lights()[0]] == [-1, 0] and h.count_implicit("sdfs") == 9
    _, h, _ = edited(vpt, "light_removed_grid", originals)
    assert [int(l["sdf"]) for l in h.lights()[0]] == [-1]
    _, h, _ = edited(vpt, "light_added_grid", originals)
    lights, cdf = h.lights()
    assert [int(l["sdf"]) for l in lights] == [-1, 1, 2] and cdf[-1:].tobytes() == np.array([F(0.3) * F(0.2)], F).tobytes()
    _, h, _ = edited(vpt, "remove_first_grid", originals)
    assert [h.volume_instance(k).volume for k in range(2)] == [0, 0] and h.volume(0)[0].shape == (40, 40, 40)
    _, h, _ = edited(vpt, "copy_swap_grid", originals)
    assert np.array_equal(bits(h.volume(1)[0]), bits(originals[W.GRID].volume(0)[0]))


def _reference():
    f = os.path.join(GOLDEN, "volume_set_stats.json")
    return json.load(open(f)) if os.path.exists(f) else {}


def test_reference_fixtures_are_there():
    assert set(_reference()) == set(W.STATE_CASES) and len(W.STATE_CASES) == 6
    gold = np.load(os.path.join(GOLDEN, "volume_set_states.npz"))
    assert set(gold.files) == {k + s for k in W.STATE_CASES for s in ("_image", "_rngs")}
    for name, (shader, res, spp) in W.STATE_CASES.items():
        assert res == 96 and 2 <= spp <= 3
        assert (_reference()[name]["shader"], _reference()[name]["resolution"], _reference()[name]["samples"]) == (shader, res, spp)


@pytest.mark.parametrize("name", list(W.STATE_CASES))
def test_the_oracle_on_the_edited_scene_reproduces_the_references_render(vpt, oracle, originals, name):
    """the reference's own render of the edited scene FILE against the oracle over the HostScene edited through the setters: bit for bit"""
    shader, res, spp = W.STATE_CASES[name]
    _, h, _ = edited(vpt, name, originals)
    gold = np.load(os.path.join(GOLDEN, "volume_set_states.npz"))
    p = vpt.PathtraceParams(resolution=res, samples=spp, shader=shader, bounces=_reference()[name]["bounces"])
    st = h.make_state(p)
    oracle.oracle_render(h, p, st, spp, nthreads=0)
    assert np.array_equal(st.rngs, gold[name + "_rngs"])
    assert np.array_equal(st.image.view(np.uint32), gold[name + "_image"].view(np.uint32))


# ---- the structs and the packing ---------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_offsets(vpt):
    assert C.sizeof(vpt.VptVolumeNew) == 48 and C.sizeof(vpt.VptVolumeSetEdit) == 112
    assert [getattr(vpt.VptVolumeNew, f).offset for f in ("whd", "res", "source", "offset", "bake", "fill", "copy_of")] == [0, 12, 16, 24, 32, 40, 44]
    assert [getattr(vpt.VptVolumeSetEdit, f).offset for f in ("remove_vol_instance_ids", "remove_sdf_ids", "remove_volume_ids", "add_volumes", "add_vol_instances",
                                                              "add_sdfs", "num_voxels", "voxels")] == [8, 24, 40, 56, 72, 88, 96, 104]
    assert (vpt.VOLUME_FROM_HOST, vpt.VOLUME_FROM_BAKE, vpt.VOLUME_FILL, vpt.VOLUME_COPY) == (0, 1, 2, 3)


def test_packing_of_a_volume_set_edit(vpt):
    assert vpt.VolumeSetEdit().empty()
    abi, keep = vpt.VolumeSetEdit().to_abi()
    assert bytes(abi) == bytes(112)   # every count zero, every pointer null
    a, b = np.arange(30, dtype=F).reshape(2, 3, 5), np.arange(8, dtype=F).reshape(2, 2, 2) + F(100)
    nan = np.array([0x7fc12345], np.uint32).view(F)[0]
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    edit = vpt.VolumeSetEdit(remove_vol_instances=[3, 1], remove_sdfs=[0], remove_volumes=[1], add_volumes=[
        vpt.VolumeNew((5, 3, 2), 0.5, vpt.VOLUME_FROM_HOST, voxels=a), vpt.VolumeNew((9, 9, 9), 0.25, vpt.VOLUME_FILL, fill=nan),
        vpt.VolumeNew((48, 48, 48), 3.0, vpt.VOLUME_COPY, copy_of=0), vpt.VolumeNew((2, 2, 2), 1.0, vpt.VOLUME_FROM_HOST, voxels=b),
        vpt.VolumeNew((4, 3, 2), 0.125, vpt.VOLUME_FROM_BAKE, bake=(tri, [[0, 1, 2]], (0.5, 0, -0.5), 0.125))],
        add_vol_instances=[vpt.VptVolumeInstance(volume=2, material=1, scalef=0.5)], add_sdfs=[vpt.VptSdf(type=4, material=2)])
    assert not edit.empty()
    abi, keep = edit.to_abi()
    assert (abi.num_remove_vol_instances, abi.num_remove_sdfs, abi.num_remove_volumes, abi.num_add_volumes, abi.num_add_vol_instances, abi.num_add_sdfs) == (2, 1, 1, 5, 1, 1)
    ids = lambda ptr, n: np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int32)), (n,)).tolist()
    assert ids(abi.remove_vol_instance_ids, 2) == [3, 1] and ids(abi.remove_sdf_ids, 1) == [0] and ids(abi.remove_volume_ids, 1) == [1]
    new = (vpt.VptVolumeNew * 5).from_address(abi.add_volumes)
    assert [(tuple(n.whd), n.res, n.source) for n in new] == [((5, 3, 2), 0.5, 0), ((9, 9, 9), 0.25, 2), ((48, 48, 48), 3.0, 3), ((2, 2, 2), 1.0, 0), ((4, 3, 2), 0.125, 1)]
    assert (new[0].offset, new[3].offset, abi.num_voxels) == (0, 30, 38) and new[2].copy_of == 0
    pool = np.ctypeslib.as_array(C.cast(abi.voxels, C.POINTER(C.c_float)), (38,))
    assert np.array_equal(pool, np.concatenate([a.reshape(-1), b.reshape(-1)]))
    assert C.string_at(C.addressof(new[1]) + 40, 4) == np.array([0x7fc12345], np.uint32).tobytes()   # a NaN keeps its payload
    desc = vpt.VptBakeDesc.from_address(new[4].bake)
    assert tuple(desc.whd) == (4, 3, 2) and tuple(desc.origin) == (0.5, 0.0, -0.5) and tuple(desc.step) == (0.125,) * 3 and new[0].bake is None
    inst = (vpt.VptVolumeInstance * 1).from_address(abi.add_vol_instances)[0]
    assert (inst.volume, inst.material, inst.scalef) == (2, 1, 0.5)
    with pytest.raises(vpt.VptError):
        vpt.VolumeSetEdit(add_volumes=[vpt.VolumeNew((5, 3, 2), 0.5, vpt.VOLUME_FROM_HOST, voxels=b)]).to_abi()


# ---- the ledger ------------------------------------------------------------------------------------------------------------------------------
def test_the_ids_the_adders_return(vpt):
    h = vpt.HostScene(path(W.GRID))
    h.remove_volumes([0])
    h.remove_volume_instances([0, 1])
    assert h.add_volume(fill=1.0, whd=(2, 2, 2), res=0.1) == 1 and h.add_volume(copy_of=0) == 2
    assert h.add_volume_instance(W.frame_at(0, 0, 0), 2, 3) == 2
    h.remove_sdfs([0])
    assert h.add_sdf(type="sphere", p=(0.1,), material=0) == 1
    edit = h.update_volume_set()
    assert (edit.remove_volumes, edit.remove_vol_instances, edit.remove_sdfs) == ((0,), (0, 1), (0,))
    assert [h.count_implicit(k) for k in ("volumes", "vol_instances", "sdfs")] == [3, 3, 2]
    assert h.volume(2)[0].shape == (48, 48, 48) and h.update_volume_set().empty()


def test_pending_edits_over_the_old_lists_come_first(vpt):
    h = vpt.HostScene(path(W.GRID))
    h.set_sdf(0, material=1)
    with pytest.raises(vpt.VptError, match="update_volumes"):
        h.remove_sdfs([1])
    h.update_volumes()
    h.remove_sdfs([1])
    for call in (lambda: h.set_sdf(0, material=0), lambda: h.set_volume_instance(0, scalef=2.0), lambda: h.set_volume(0, np.zeros((2, 2, 2), F)),
                 lambda: h.sculpt_volume(0, [])):
        with pytest.raises(vpt.VptError, match="update_volume_set"):
            call()
    assert not h.update_volume_set().empty() and h.count_implicit("sdfs") == 1
    h.set_sdf(0, material=0)   # the lists are current again
    h.sculpt_volume(0, [])
    with pytest.raises(vpt.VptError, match="update_sculpts"):
        h.add_volume(fill=0.0, whd=(1, 1, 1), res=1.0)


def test_refused_notes_and_a_refused_hand_out_change_nothing(vpt):
    h = vpt.HostScene(path(W.GRID))
    before = implicit_tables(vpt, h)
    for call in (lambda: h.remove_volumes([2]), lambda: h.remove_sdfs([0, 0]), lambda: h.add_volume(), lambda: h.add_volume(fill=1.0, whd=(2, 2, 2)),
                 lambda: h.add_volume(np.zeros((2, 2), F), res=1.0), lambda: h.add_volume(fill=1.0, copy_of=0), lambda: h.add_volume(copy_of=5),
                 lambda: h.add_volume_instance(W.frame_at(0, 0, 0), 2, 0), lambda: h.add_volume_instance(W.frame_at(0, np.nan, 0), 0, 0),
                 lambda: h.add_volume_instance(W.frame_at(0, 0, 0), 0, 99), lambda: h.add_sdf(type=7, material=0), lambda: h.add_sdf(type="box", material=99),
                 lambda: h.add_sdf(type="box", material=0, whd=(np.inf, 1, 1))):
        with pytest.raises((vpt.VptError, ValueError)):
            call()
    assert h.update_volume_set().empty()
    h.remove_volumes([1])   # its instances stay: the hand-out is refused, the note stays pending
    with pytest.raises(vpt.VptError, match="still named"):
        h.update_volume_set()
    assert implicit_tables(vpt, h) == before
    h.remove_volume_instances([2, 3])
    assert not h.update_volume_set().empty() and h.count_implicit("volumes") == 1


def test_a_baked_addition_runs_on_the_host_only_when_the_copy_is_read(vpt, originals):
    h = vpt.HostScene(path(W.GRID))
    W.apply(vpt, "bake_new_grid", h)
    assert len(h._lazy_bakes) == 1 and h._lazy_bakes[0][0] == 2
    verts, tris = V.sphere_mesh()
    res, origin, step, _ = V.small_fit(vpt)
    want, _ = vpt.bake_sdf_grid(verts, tris, V.SMALL, origin, step, device=None)
    got, got_res = h.volume(2)
    assert h._lazy_bakes == [] and np.array_equal(bits(got), bits(want)) and got_res == F(res)
    h.add_volume(bake=(verts, tris, origin, step), whd=V.SMALL, res=res)   # a pending bake runs before the next set edit renumbers
    h.update_volume_set()
    h.remove_volumes([0])
    h.remove_volume_instances([0, 1])
    h.update_volume_set()
    assert h._lazy_bakes == [(2, h._lazy_bakes[0][1])]   # it followed its volume from id 3 without running
    assert np.array_equal(bits(h.volume(2)[0]), bits(want)) and np.array_equal(bits(h.volume(1)[0]), bits(want))
    h.add_volume(bake=(verts, tris, origin, step), whd=V.SMALL, res=res)
    h.update_volume_set()
    h.remove_volumes([3])
    h.update_volume_set()
    assert h._lazy_bakes == [] and h.count_implicit("volumes") == 3   # a bake whose volume goes is never run
