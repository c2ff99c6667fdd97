"""vpt_mesh_sdf and vpt_scene_mesh_volume on the GPU (include/vpt.h).  The criterion is equality of bits with the host mirror
(pinned to a numpy replay of the rule by tests/test_sdf_mesh_host.py): positions, normals and quads of every case there and of the grids
chosen here for what the four passes can get wrong; the three entries - host array, resident volume, resident volume with a region - give
the same bytes; meshing changes nothing of a scene; RenderSession.volume_to_shape leaves the scene a fresh DeviceScene of the host mirror
would be, with the mesh where the sphere trace finds the surface."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import bake_meshes
import sculpt_cases as S
from conftest import GOLDEN
from sdf_mesh_cases import CASES, F, _points, _sphere, arrays, case, replay, same_bytes, topology

pytestmark = pytest.mark.gpu
BLOCK = 256   # voxels per block of the four passes


def both(vpt, voxels, origin, step, iso=0.0, stats=None):
    return vpt.mesh_sdf(voxels, origin, step, iso, device=0, stats=stats), vpt.mesh_sdf(voxels, origin, step, iso, device=None)


@pytest.mark.parametrize("name", CASES)
def test_the_device_gives_the_mirrors_bytes(vpt, name):
    c, st = case(name), {}
    dev, host = both(vpt, c["voxels"], c["origin"], c["step"], c["iso"], st)
    print(f"{name}: {st}", flush=True)
    assert len(arrays(host)[0]) > 0 and same_bytes(dev, host)
    assert (st["num_vertices"], st["num_quads"], st["launches"]) == (len(dev["positions"]), len(dev["quads"]), 4)


def sphere_grid(whd, centre, radius):
    return _sphere(*_points(whd, (0, 0, 0), (1, 1, 1)), centre, radius)


def test_rows_and_grids_that_are_no_multiple_of_a_block(vpt):
    v = sphere_grid((33, 17, 9), (15.6, 8.3, 4.2), 3.7)
    dev, host = both(vpt, v, 0.0, 1.0)
    assert v.size % BLOCK and same_bytes(dev, host) and topology(*arrays(dev)[::2])["closed"]


def test_more_blocks_than_one_pass_of_the_scan(vpt):
    """268 800 voxels are 1 050 blocks: the scan of the block counts crosses its own blocks; about 20 k vertices"""
    v = sphere_grid((70, 64, 60), (34.6, 31.7, 29.8), 28.3)
    st = {}
    dev, host = both(vpt, v, (-3.0, 0.5, 2.0), (0.01, 0.012, 0.009), 0.0, st)
    print(f"70x64x60: {st}", flush=True)
    assert -(-v.size // BLOCK) > 1024 and 15000 < st["num_vertices"] < 25000
    assert same_bytes(dev, host)
    t = topology(*arrays(dev)[::2])
    assert t["closed"] and t["used"] and t["chi"] == 2 and t["volume"] > 0
    again = vpt.mesh_sdf(v, (-3.0, 0.5, 2.0), (0.01, 0.012, 0.009), 0.0, device=0)   # two calls in a row: the same bytes
    assert same_bytes(again, dev)


def test_a_surface_in_the_last_block_only(vpt):
    whd = (5, 6, 40)
    v = sphere_grid(whd, (2.1, 2.6, 36.9), 1.3)
    cells = replay(v, (0, 0, 0), (1, 1, 1), 0.0)["cells"]
    owner = cells[:, 0] + whd[0] * (cells[:, 1] + whd[1] * cells[:, 2])
    assert len(owner) and owner.min() >= (v.size // BLOCK) * BLOCK and v.size % BLOCK
    dev, host = both(vpt, v, 0.0, 1.0)
    assert same_bytes(dev, host) and len(dev["quads"]) > 0


def test_nothing_to_mesh_launches_nothing(vpt):
    for v in (np.full((1, 1, 1), -1, F), np.full((1, 1, 64), -1, F), np.full((9, 1, 7), -1, F), np.ones((12, 11, 10), F)):
        st = {}
        m = vpt.mesh_sdf(v, 0.0, 1.0, device=0, stats=st)
        assert m["positions"] is None and m["quads"] is None and st == {"num_vertices": 0, "num_quads": 0, "launches": 0, "device_ms": 0.0}
    # a sign change on the border alone: vertices (the counting passes and the vertex pass ran), no quad, no quad pass
    v = np.ones((4, 4, 4), F)
    v[0, 0, 0] = -1
    st = {}
    dev, host = both(vpt, v, 0.0, 1.0, 0.0, st)
    assert same_bytes(dev, host) and dev["quads"] is None and len(dev["positions"]) == 1 and st["launches"] == 3


# ---- the resident entry ----------------------------------------------------------------------------------------------------------------
def grid_step(vol, res):
    return np.array([F(res) * F(w) / F(w - 1) for w in vol.shape[::-1]], F)


def render(vpt, dev, host, shader):
    p = vpt.PathtraceParams(resolution=96, samples=2, shader=shader, bounces=4)
    st = host.make_state(p)
    dev.pathtrace_samples(st, p, 2)
    return st


def same_state(a, b):
    return (a.samples == b.samples and np.array_equal(a.image.view(np.uint32), b.image.view(np.uint32)) and np.array_equal(a.rngs, b.rngs)
            and np.array_equal(a.hits, b.hits))


def assert_three_entries_agree(vpt, A, host, what):
    """every volume: the resident entry, the host-array entry over get_voxels, the host mirror over the host scene's copy"""
    for k in (S.SACKBOY, S.BUNNY):
        vol, res = host.volume(k)
        got = A.get_voxels(k)
        assert got.tobytes() == vol.tobytes(), f"{what}: volume {k} differs from the host scene's"
        st = {}
        resident = A.mesh_volume(k, stats=st)
        assert len(resident["positions"]) > 100 and st["launches"] == 4, what
        assert same_bytes(resident, vpt.mesh_sdf(got, 0.0, grid_step(vol, res), device=0)), f"{what}: volume {k}, host-array entry"
        assert same_bytes(resident, host.mesh_volume(k)), f"{what}: volume {k}, host mirror"
        whole = ((0, 0, 0), vol.shape[::-1])
        assert same_bytes(A.mesh_volume(k, region=whole), resident), f"{what}: volume {k}, a region of the whole grid"


def test_a_resident_volume_meshes_like_its_voxels_through_every_edit(vpt):
    host = vpt.HostScene(S.GRID)
    A = vpt.DeviceScene(host, 0)
    hashes, renders = A.light_tables_hash(), [render(vpt, A, host, s) for s in ("implicit", "implicit_normal")]
    assert_three_entries_agree(vpt, A, host, "as loaded")
    # iso, origin and step of the caller's; a region: the rule on the sub-grid, vertices in place
    vol, res = host.volume(S.BUNNY)
    origin, step = np.array([0.3, -0.2, 1.5], F), np.array([0.011, 0.013, 0.009], F)
    assert same_bytes(A.mesh_volume(S.BUNNY, iso=0.004, origin=origin, step=step), vpt.mesh_sdf(vol, origin, step, 0.004, device=None))
    for region in (S.BOX, S.ROWS, ((0, 0, 0), (40, 40, 1)), ((7, 7, 7), (2, 2, 2)), ((39, 0, 17), (1, 1, 1)), ((5, 5, 5), (0, 7, 7))):
        got = A.mesh_volume(S.BUNNY, region=region)
        assert same_bytes(got, host.mesh_volume(S.BUNNY, region=region)), region
        lo, size = region
        if min(size) < 1:
            assert got["positions"] is None
            continue
        alone = vpt.mesh_sdf(vol[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]], 0.0, grid_step(vol, res), device=None)
        assert np.array_equal(arrays(got)[2], arrays(alone)[2]) and len(arrays(got)[0]) == len(arrays(alone)[0]), region
    assert len(A.mesh_volume(S.BUNNY, region=S.BOX)["quads"]) > 100
    # meshing changed nothing of the scene
    assert A.light_tables_hash() == hashes
    assert all(same_state(render(vpt, A, host, s), r) for s, r in zip(("implicit", "implicit_normal"), renders))
    # after a sculpt
    host.sculpt_volume(S.BUNNY, S.stroke(vpt, 4), region=S.BOX)
    A.sculpt_volumes(host.update_sculpts())
    assert_three_entries_agree(vpt, A, host, "after a sculpt")
    # after an update that grows a volume: the pool is allocated anew, the offsets move
    sack = host.volume(S.SACKBOY)[0]
    host.set_volume(S.SACKBOY, np.pad(sack, ((0, 1), (0, 2), (0, 0)), mode="edge"))
    A.update_volumes(host.update_volumes())
    assert tuple(A.get_volumes()[0][S.SACKBOY].whd) == (48, 50, 49)
    assert_three_entries_agree(vpt, A, host, "after the pool has grown")


def test_the_resident_entry_refuses_before_it_writes(vpt):
    A = vpt.DeviceScene(vpt.HostScene(S.GRID), 0)
    for kw, word in ((dict(index=2), "volume 2 out of range"), (dict(index=-1), "out of range"), (dict(index=1, step=(1, 0, 1)), "step must be > 0"),
                     (dict(index=1, iso=np.nan), "iso is not finite"), (dict(index=1, region=((38, 0, 0), (3, 1, 1))), "the region leaves the grid")):
        with pytest.raises(vpt.VptError, match=word):
            A.mesh_volume(**kw)
    desc = vpt.VptSdfMeshDesc((C.c_int32 * 3)(40, 40, 41), (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), 0.0)
    st = vpt.VptSdfMeshStats(-5, -5, -5, 0)
    assert vpt.hip.vpt_scene_mesh_volume(A.handle, 1, C.byref(desc), None, None, None, 0, None, 0, C.byref(st)) == -1
    assert "vpt_scene_mesh_volume: desc->whd is not the volume's" in vpt.hip.vpt_last_error().decode() and st.num_vertices == -5
    # the capacity convention on the device entry: counts set, nothing written
    positions = np.full((10, 3), 7, F)
    assert vpt.hip.vpt_scene_mesh_volume(A.handle, 1, None, None, positions.ctypes.data, None, 10, None, 0, C.byref(st)) == -1
    assert vpt.hip.vpt_last_error().decode() == f"vertex_capacity 10 < {st.num_vertices} vertices" and st.num_vertices > 100 and (positions == 7).all()


# ---- round trip and the gesture ----------------------------------------------------------------------------------------------------------
def test_bake_then_mesh_gives_the_sphere_back(vpt):
    verts, tris = bake_meshes.icosphere(3, radius=0.8)
    origin, step = np.full(3, -1, F), np.full(3, 2 / 32, F)
    grid, _ = vpt.bake_sdf_grid(verts, tris, 33, origin, step, device=0)
    m = vpt.mesh_sdf(grid, origin, step, device=0)
    positions, normals, quads = arrays(m)
    t = topology(positions, quads)
    assert t["closed"] and t["used"] and t["chi"] == 2 and t["volume"] > 0
    p = positions.astype(np.float64)
    # the icosphere's faces lie inside the sphere by at most r (1 - cos(half an edge's angle)) < 0.01 r at three subdivisions
    assert np.abs(np.linalg.norm(p, axis=1) - 0.8).max() <= np.linalg.norm(step) + 0.01 * 0.8
    assert (np.einsum("ij,ij->i", normals.astype(np.float64), p) > 0).all()


def grid_scene_with_a_mesh(tmp_path):
    """06_gridsdf_synth with one mesh out of sight (the shape edit's pools are those of a scene that holds shapes) under a material without a texture"""
    scenes = os.path.join(GOLDEN, "scenes")
    d = json.load(open(S.GRID))
    out = str(tmp_path)
    for key in ("textures", "volumes"):
        for item in d[key]:
            item["uri"] = os.path.relpath(os.path.join(scenes, "06_gridsdf_synth", item["uri"]), out)
    d["shapes"] = [{"name": "sphere", "uri": os.path.relpath(os.path.join(scenes, "03_volume", "shapes", "sphere.ply"), out)}]
    d["instances"] = [{"name": "sphere", "shape": 0, "material": 4, "frame": [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, -50, 0]}]
    path = os.path.join(out, "grid_and_mesh.json")
    json.dump(d, open(path, "w"))
    return path


def test_volume_to_shape_puts_the_mesh_where_the_sphere_trace_finds_the_surface(vpt, tmp_path):
    file = grid_scene_with_a_mesh(tmp_path)
    host = vpt.HostScene(file)
    dev = vpt.DeviceScene(host, 0)
    implicit = vpt.PathtraceParams(resolution=96, samples=4, shader="implicit", bounces=2)
    s = vpt.RenderSession(dev, implicit)
    s.advance(1)
    ids, _ = s.sdf_ids()
    target = S.BUNNY_INSTANCES[0]
    pixels = np.argwhere(ids[..., 0] == target)
    assert len(pixels) > 20
    y, x = (int(v) for v in pixels[np.argmin(np.linalg.norm(pixels - pixels.mean(axis=0), axis=1))])   # the pixel nearest the middle of the bunny
    seen = s.pick_sdf(x, y)
    assert seen is not None and seen["vol_instance"] == target and seen["volume"] == S.BUNNY
    shapes, instances = host.count("shapes"), host.count("instances")
    shape, instance = s.volume_to_shape(host, target, material=5)
    assert (shape, instance) == (shapes, instances) and host.count("shapes") == shapes + 1 and host.count("instances") == instances + 1 and s.samples == 0
    # the new shape is the resident grid's mesh in the instance's lookup space
    vol, res = host.volume(S.BUNNY)
    inst = host.volume_instance(target)
    expected = vpt.mesh_sdf(vol, 0.0, grid_step(vol, res) * F(inst.scalef), device=None)
    made = host.shape_arrays(shape)
    assert made["positions"].tobytes() == expected["positions"].tobytes() and np.array_equal(made["quads"], expected["quads"])
    # under a mesh shader the pixel shows the new instance, at the distance the sphere trace found (within a cell's diagonal)
    s.reset(vpt.PathtraceParams(resolution=96, samples=4, shader="eyelight", bounces=2))
    s.advance(1)
    hit = s.pick(x, y)
    assert hit is not None and hit["instance"] == instance and hit["shape"] == shape and hit["material"] == 5
    # the two surfaces lie within a cell's diagonal d of the field's zero set each; along a ray that meets it under the cosine c that is 2 d / c
    eye = np.array(host.camera(0).frame.o[:], np.float64)
    along = seen["position"].astype(np.float64) - eye
    c = abs(np.dot(along / np.linalg.norm(along), seen["normal"].astype(np.float64)))
    assert abs(hit["distance"] - seen["distance"]) <= 2 * np.linalg.norm(grid_step(vol, res) * F(inst.scalef)) / c
    s.close()
    # the scene the two edits left is the scene a fresh handle of the host mirror holds
    fresh = vpt.DeviceScene(host, 0)
    assert dev.shape_tables_hash() == fresh.shape_tables_hash() and dev.instance_tables_hash() == fresh.instance_tables_hash()
    assert dev.light_tables_hash() == fresh.light_tables_hash()
    for shader in ("pathtrace", "eyelight", "implicit"):
        assert same_state(render(vpt, dev, host, shader), render(vpt, fresh, host, shader)), shader
