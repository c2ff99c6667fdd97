"""The host side of vpt_scene_update_volumes: HostScene.set_volume_instance / set_sdf / set_volume / bake_volume /
update_volumes(), the mirror over a scene whose implicit side was edited through the setters, against the same scene loaded afresh
from an edited scene file with its .sdf (descriptor tables byte for byte), against the reference's own render of that file
(tests/golden/volume_edit_states.npz, written by tests/golden/make_volume_edit_fixtures.py) through the oracle, and against a numpy
replay of op_union.  No device."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import volume_edits as V
from bake_meshes import bits
from conftest import GOLDEN, ROOT

F = np.float32


def path(scene_file):
    return os.path.join(GOLDEN, "scenes", scene_file)


@pytest.fixture(scope="module")
def originals(vpt):
    return {scene_file: vpt.HostScene(path(scene_file)) for scene_file in (V.GRID, V.SDFS)}


def edited(vpt, name, originals):
    scene_file = V.cases(vpt)[name][0]
    h = vpt.HostScene(path(scene_file))
    return scene_file, h, V.apply(vpt, name, h, original=originals[scene_file])


def implicit_tables(vpt, h):
    """volumes (whd, res and the voxels each names), vol_instances and sdfs of the descriptor, as bytes"""
    d = vpt.VptSceneDescImplicit.from_address(h.desc + vpt.VptSceneDescImplicit.OFFSET)
    grab = lambda ptr, n, size: C.string_at(ptr, n * size) if n else b""
    vols = (vpt.VptVolume * d.num_volumes).from_address(d.volumes) if d.num_volumes else []
    pool = vpt.VptSceneDescVoxels.from_address(h.desc + vpt.VptSceneDescVoxels.OFFSET)
    voxels = [C.string_at(pool.voxels + 4 * v.offset, 4 * v.whd[0] * v.whd[1] * v.whd[2]) for v in vols]
    assert sum(len(v) for v in voxels) == 4 * pool.num_voxels   # the descriptor's pool holds the volumes back to back, nothing else
    return (grab(d.volumes, d.num_volumes, 24), grab(d.vol_instances, d.num_vol_instances, 60), grab(d.sdfs, d.num_sdfs, 84), voxels)


@pytest.mark.parametrize("name", V.AS_SCENE_FILE)
def test_update_volumes_equals_the_edited_scene_loaded_afresh(vpt, originals, tmp_path, name):
    """volumes, vol_instances, sdfs, every volume's voxels, lights and light_cdf of the descriptor, byte for byte"""
    scene_file, h, edits = edited(vpt, name, originals)
    assert all(not e.empty() for e in edits) and h.update_volumes().empty()
    fresh = vpt.HostScene(V.write_edited_scene(vpt, name, tmp_path, originals[scene_file]))
    got, want = implicit_tables(vpt, h), implicit_tables(vpt, fresh)
    for part, a, b in zip(("volumes", "vol_instances", "sdfs", "voxels"), got, want):
        assert a == b, f"{name}: {part}"
    (lights, cdf), (want_lights, want_cdf) = h.lights(), fresh.lights()
    assert lights.tobytes() == want_lights.tobytes() and cdf.tobytes() == want_cdf.tobytes()
    if name in V.BAKES:
        assert h._lazy_bakes == []   # reading the descriptor ran the host mirror of the bake
    same = got == implicit_tables(vpt, originals[scene_file]) and lights.tobytes() == originals[scene_file].lights()[0].tobytes()
    assert same == (name in V.NO_OPS), name


def _reference():
    f = os.path.join(GOLDEN, "volume_edit_stats.json")
    return json.load(open(f)) if os.path.exists(f) else {}


def test_reference_fixtures_are_there():
    assert set(_reference()) == set(V.STATE_CASES)
    gold = np.load(os.path.join(GOLDEN, "volume_edit_states.npz"))
    assert set(gold.files) == {k + s for k in V.STATE_CASES for s in ("_image", "_rngs")}
    for name, (shader, res, spp) in V.STATE_CASES.items():
        assert res == 96 and 2 <= spp <= 4
        assert (_reference()[name]["shader"], _reference()[name]["resolution"], _reference()[name]["samples"]) == (shader, res, spp)


@pytest.mark.parametrize("name", list(V.STATE_CASES))
def test_the_oracle_on_the_edited_scene_reproduces_the_references_render(vpt, oracle, originals, name):
    """the reference's own render of the edited scene FILE against the oracle over the HostScene edited through the setters: bit for bit"""
    shader, res, spp = V.STATE_CASES[name]
    _, h, _ = edited(vpt, name, originals)
    gold = np.load(os.path.join(GOLDEN, "volume_edit_states.npz"))
    p = vpt.PathtraceParams(resolution=res, samples=spp, shader=shader, bounces=_reference()[name]["bounces"])
    st = h.make_state(p)
    oracle.oracle_render(h, p, st, spp, nthreads=0)
    assert np.array_equal(st.rngs, gold[name + "_rngs"])
    assert np.array_equal(st.image.view(np.uint32), gold[name + "_image"].view(np.uint32))


@pytest.mark.parametrize("resident_nans,incoming_nans", [(0, 0), (0, 40), (30, 0), (30, 40)])
def test_union_is_the_select(vpt, originals, resident_nans, incoming_nans):
    """the mirror's UNION against numpy's where(a < b, a, b): a NaN resident value is replaced, a NaN incoming value is taken; fmin
    would keep the number both times"""
    h = vpt.HostScene(path(V.GRID))
    lo, size = (8, 9, 10), (23, 21, 19)
    a = V.incoming(size[::-1], 21, resident_nans)
    b = V.incoming(size[::-1], 22, incoming_nans)
    h.set_volume(V.BUNNY, a, region=(lo, size))
    h.update_volumes()
    h.set_volume(V.BUNNY, b, region=(lo, size), mode=vpt.VOXELS_UNION)
    assert len(h.update_volumes().volumes) == 1
    got = V.box_of(h.volume(V.BUNNY)[0], lo, size)
    with np.errstate(invalid="ignore"):
        want = np.where(a < b, a, b)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(np.isnan(got), np.isnan(b))
    if resident_nans and incoming_nans:
        assert not np.array_equal(bits(got), bits(np.fmin(a, b)))
    outside = h.volume(V.BUNNY)[0].copy()
    V.box_of(outside, lo, size)[...] = V.box_of(originals[V.GRID].volume(V.BUNNY)[0], lo, size)
    assert np.array_equal(bits(outside), bits(originals[V.GRID].volume(V.BUNNY)[0]))


def test_a_bake_runs_on_the_host_only_when_the_copy_is_read(vpt, originals):
    h = vpt.HostScene(path(V.GRID))
    V.apply(vpt, "bake_region_grid", h, original=originals[V.GRID])
    assert len(h._lazy_bakes) == 1          # update_volumes() handed the edit out without baking
    resident = V.small_resident(vpt)[0]
    got, res = h.volume(V.BUNNY)            # reading the copy runs the host mirror of the bake
    assert h._lazy_bakes == [] and res == F(V.small_fit(vpt)[0])
    assert np.array_equal(bits(got), bits(V.baked_small(vpt, resident, V.REGION)))
    assert not np.array_equal(bits(got), bits(resident))


OK_VOXELS = np.zeros((1, 1, 1), F)
REFUSALS = {   # one per rule of include/vpt.h that the host setters can meet
    "instance id out of range": lambda h: h.set_volume_instance(4, scalef=1.0),
    "instance frame NaN": lambda h: h.set_volume_instance(0, frame=[1, 0, 0, 0, 1, 0, 0, 0, 1, float("nan"), 0, 0]),
    "instance scalef infinite": lambda h: h.set_volume_instance(0, scalef=float("inf")),
    "instance volume out of range": lambda h: h.set_volume_instance(0, volume=2),
    "instance material out of range": lambda h: h.set_volume_instance(0, material=-1),
    "sdf id out of range": lambda h: h.set_sdf(2, material=0),
    "sdf type out of range": lambda h: h.set_sdf(0, type=6),
    "sdf material out of range": lambda h: h.set_sdf(0, material=1000),
    "sdf whd NaN": lambda h: h.set_sdf(1, whd=(float("nan"), 1, 1)),
    "sdf parameter infinite": lambda h: h.set_sdf(1, p=(float("inf"),)),
    "volume id out of range": lambda h: h.set_volume(2, OK_VOXELS),
    "voxels of two dimensions": lambda h: h.set_volume(1, np.zeros((2, 2), F)),
    "res NaN": lambda h: h.set_volume(1, OK_VOXELS, float("nan")),
    "region past the grid": lambda h: h.set_volume(1, np.zeros((1, 1, 3), F), region=((38, 0, 0), (3, 1, 1))),
    "voxels of another shape than the region": lambda h: h.set_volume(1, np.zeros((1, 1, 2), F), region=((0, 0, 0), (3, 1, 1))),
    "mode 2": lambda h: h.set_volume(1, OK_VOXELS, region=((0, 0, 0), (1, 1, 1)), mode=2),
    "a new whd in UNION mode": lambda h: h.set_volume(1, np.zeros((8, 8, 8), F), mode=1),
}


@pytest.fixture(scope="module")
def untouched(vpt):
    h = vpt.HostScene(path(V.GRID))
    return h, (implicit_tables(vpt, h), h.lights()[0].tobytes(), h.lights()[1].tobytes(), h.stats())


@pytest.mark.parametrize("what", list(REFUSALS))
def test_setters_refuse_what_the_device_would(vpt, untouched, what):
    """after a refusal, the descriptor, lights(), stats() and the pending edit are unchanged"""
    h, before = untouched
    with pytest.raises(vpt.VptError):
        REFUSALS[what](h)
    assert h.update_volumes().empty()
    assert (implicit_tables(vpt, h), h.lights()[0].tobytes(), h.lights()[1].tobytes(), h.stats()) == before


def test_a_volume_is_named_once_per_edit(vpt):
    h = vpt.HostScene(path(V.GRID))
    h.set_volume(1, OK_VOXELS, region=((0, 0, 0), (1, 1, 1)))
    with pytest.raises(vpt.VptError):
        h.set_volume(1, OK_VOXELS, region=((1, 0, 0), (1, 1, 1)))
    with pytest.raises(vpt.VptError):
        h.bake_volume(1, *V.sphere_mesh())
    assert list(h.update_volumes().volumes) == [1]


def test_volume_edit_abi(vpt):
    """packing round-trips: two host volumes and a bake in one edit; offsets count voxels inside the edit's own pool, in entry order"""
    a, b = V.incoming((2, 3, 5), 1), V.incoming((4, 4, 4), 2)
    verts, tris = V.sphere_mesh()
    inst = vpt.VptVolumeInstance(volume=1, material=3, scalef=0.5)
    inst.frame.o[:] = [1.0, 2.0, 3.0]
    f = vpt.VptSdf(type=5, material=2)
    f.p[:] = [0.25, 0.125, 0.0, 0.0]
    edit = vpt.VolumeEdit(vol_instances={2: inst}, sdfs={7: f}, volumes={
        1: vpt.VolumeSource((40, 40, 40), 0.5, (1, 2, 3), (5, 3, 2), vpt.VOXELS_UNION, a),
        0: vpt.VolumeSource(V.SMALL, 0.25, (0, 0, 0), V.SMALL, vpt.VOXELS_REPLACE, None, (verts, tris, (-1.0, -2.0, -3.0), 0.125)),
        3: vpt.VolumeSource((4, 4, 4), 2.0, (0, 0, 0), (4, 4, 4), vpt.VOXELS_REPLACE, b)})
    abi, keep = edit.to_abi()
    assert (abi.num_vol_instances, abi.num_sdfs, abi.num_volumes, abi.num_voxels) == (1, 1, 3, 30 + 64)
    assert list(np.ctypeslib.as_array(C.cast(abi.volume_ids, C.POINTER(C.c_int32)), (3,))) == [1, 0, 3]
    assert C.cast(abi.vol_instance_ids, C.POINTER(C.c_int32))[0] == 2 and C.cast(abi.sdf_ids, C.POINTER(C.c_int32))[0] == 7
    e = C.cast(abi.volumes, C.POINTER(vpt.VptVolumeSource))
    assert [(tuple(e[k].whd), e[k].res, tuple(e[k].region_lo), tuple(e[k].region_whd), e[k].mode, e[k].offset) for k in range(3)] == [
        ((40, 40, 40), 0.5, (1, 2, 3), (5, 3, 2), 1, 0), (V.SMALL, 0.25, (0, 0, 0), V.SMALL, 0, -1), ((4, 4, 4), 2.0, (0, 0, 0), (4, 4, 4), 0, 30)]
    assert not e[0].bake and not e[2].bake
    pool = np.ctypeslib.as_array(C.cast(abi.voxels, C.POINTER(C.c_float)), (94,))
    assert np.array_equal(bits(pool[:30]), bits(a).reshape(-1)) and np.array_equal(bits(pool[30:]), bits(b).reshape(-1))
    desc = vpt.VptBakeDesc.from_address(e[1].bake)
    assert (desc.num_vertices, desc.num_triangles, tuple(desc.whd), tuple(desc.origin), tuple(desc.step)) == (len(verts), 320, V.SMALL, (-1.0, -2.0, -3.0), (0.125,) * 3)
    assert np.array_equal(np.ctypeslib.as_array(C.cast(desc.triangles, C.POINTER(C.c_int32)), (320, 3)), tris)
    assert bytes(C.cast(abi.vol_instances, C.POINTER(vpt.VptVolumeInstance))[0]) == bytes(inst)
    assert bytes(C.cast(abi.sdfs, C.POINTER(vpt.VptSdf))[0]) == bytes(f)
    assert (C.sizeof(vpt.VptVolume), C.sizeof(vpt.VptVolumeInstance), C.sizeof(vpt.VptSdf), C.sizeof(vpt.VptVolumeSource), C.sizeof(vpt.VptVolumeEdit)) == (24, 60, 84, 64, 88)
    assert vpt.VolumeEdit().empty() and not edit.empty()
    with pytest.raises(vpt.VptError):
        vpt.VolumeEdit(volumes={0: vpt.VolumeSource((4, 4, 4), 1.0, (0, 0, 0), (2, 2, 2), 0, np.zeros((2, 2, 3), F))}).to_abi()


NEW_SYMBOLS = ("vpt_scene_update_volumes", "vpt_multi_update_volumes", "vpt_session_edit_volumes", "vpt_scene_get_volumes", "vpt_scene_get_voxels")


def test_symbols_and_declarations(vpt):
    header = open(os.path.join(ROOT, "include", "vpt.h")).read()
    for name in NEW_SYMBOLS:
        assert getattr(vpt.hip, name) is not None
        assert re.search(r"^int\s+%s\(" % name, header, re.M), name
    for name in ("vpth_scene_set_vol_instance", "vpth_scene_set_sdf", "vpth_scene_set_volume", "vpth_scene_update_volumes"):
        assert getattr(vpt.host, name) is not None
    # the structs older binaries fill in keep their layout beside the new one
    assert "const float* const* shape_normals;     /* per entry: num_vertices float3 or NULL (keep); the array itself may be NULL    */\n} vpt_scene_edit;" in header
    assert "  int64_t num_texels_b; const uint8_t* texels_b;   /* uchar4 */\n} vpt_texture_edit;" in header
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "volumetric-path-tracer_amd", "libvpt_hip.so")], capture_output=True, text=True)
    if nm.returncode == 0:
        exported = {line.split()[-1] for line in nm.stdout.splitlines() if line.strip()}
        assert set(NEW_SYMBOLS) <= exported


def test_null_arguments_need_no_device(vpt):
    """the argument checks that come before any device call"""
    assert vpt.hip.vpt_scene_update_volumes(None, None) == -1
    assert vpt.hip.vpt_multi_update_volumes(None, None) == -1
    assert vpt.hip.vpt_session_edit_volumes(None, None) == -1
    assert vpt.hip.vpt_scene_get_volumes(None, None, 0, None, 0, None, 0) == -1
    assert vpt.hip.vpt_scene_get_voxels(None, 0, None, 0) == -1
