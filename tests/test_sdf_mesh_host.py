"""vpt_mesh_sdf without a GPU: the host mirror (host/vpt_sdf_mesh.cpp, the rule header csrc/vpt_sdf_mesh_rule.h in serial
loops) against a numpy replay of the rule written from its text in sdf_mesh_cases.py, bit for bit; the topology and the geometry the rule
promises; what both entries refuse before they look for a device; the outputs' capacity convention; the PLY writer through the scene
loader; ypathtrace --mesh-sdf --mesh-host."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from sdf_mesh_cases import CASES, CLOSED, F, arrays, case, replay, replayed, same_bytes, topology

BIN = os.path.join(ROOT, "volumetric-path-tracer_amd", "ypathtrace")


def mirror(vpt, name, **kw):
    c = case(name)
    return vpt.mesh_sdf(c["voxels"], c["origin"], c["step"], c["iso"], device=None, **kw)


@pytest.mark.parametrize("name", CASES)
def test_the_mirror_gives_the_bits_of_the_replayed_rule(vpt, name):
    ref = replayed(name)
    assert len(ref["positions"]) > 0 and len(ref["quads"]) > 0
    assert same_bytes(mirror(vpt, name), ref)


def test_nonfinite_voxels_use_the_guard_and_leave_finite_vertices(vpt):
    ref = replayed("nonfinite")
    assert ref["guarded"] > 0, "no crossing parameter of the case left [0, 1]"
    positions, normals, _ = arrays(mirror(vpt, "nonfinite"))
    assert np.isfinite(positions).all() and np.isfinite(normals).all()


def test_a_region_is_the_sub_grid_with_its_vertices_in_place(vpt):
    c, region = case("torus"), ((3, 2, 5), (17, 20, 12))
    got = mirror(vpt, "torus", region=region)
    assert same_bytes(got, replay(c["voxels"], c["origin"], c["step"], c["iso"], region))
    lo, size = region
    sub = c["voxels"][lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]]
    alone = vpt.mesh_sdf(sub, c["origin"] + np.array(lo, F) * c["step"], c["step"], c["iso"], device=None)
    assert np.array_equal(got["quads"], alone["quads"])   # ids and order: those of the sub-grid alone
    assert np.allclose(got["positions"], alone["positions"], rtol=0, atol=1e-5) and np.array_equal(got["normals"], alone["normals"])
    whole = mirror(vpt, "torus", region=((0, 0, 0), (24, 24, 24)))
    assert same_bytes(whole, mirror(vpt, "torus"))


@pytest.mark.parametrize("name", CLOSED)
def test_an_interior_surface_gives_a_closed_outward_mesh(vpt, name):
    positions, normals, quads = arrays(mirror(vpt, name))
    t = topology(positions, quads)
    assert t["closed"] and t["used"]
    assert t["chi"] == case(name)["chi"]
    assert t["volume"] > 0


def test_a_surface_that_leaves_the_grid_gives_an_open_mesh(vpt):
    for name in ("clipped", "plane"):
        positions, _, quads = arrays(mirror(vpt, name))
        t = topology(positions, quads)
        assert not t["closed"] and t["volume"] != 0


@pytest.mark.parametrize("name", CLOSED)
def test_vertices_lie_in_their_cells_and_normals_point_out(vpt, name):
    c, ref = case(name), replayed(name)
    positions, normals, _ = arrays(mirror(vpt, name))
    origin, step = c["origin"].astype(np.float64), c["step"].astype(np.float64)
    low = origin + ref["cells"] * step
    slack = 4 * np.finfo(F).eps * (np.abs(origin) + (np.array(c["voxels"].shape[::-1]) + 1) * step)   # the three roundings of add, multiply, add
    p = positions.astype(np.float64)
    assert (p >= low - slack).all() and (p <= low + step + slack).all()
    # a cell that holds a vertex holds a sign change, so the surface passes through it: no further than the cell's diagonal
    assert np.abs(c["distance"](p)).max() <= np.linalg.norm(step) + slack.max()
    assert (np.einsum("ij,ij->i", normals.astype(np.float64), c["gradient"](p)) > 0).all()
    assert np.allclose(np.linalg.norm(normals.astype(np.float64), axis=1), 1, atol=1e-6)


def test_the_smallest_grids(vpt):
    one = np.ones((2, 2, 2), F)
    one[0, 0, 0] = -1
    positions, _, quads = arrays(vpt.mesh_sdf(one, 0.0, 1.0, device=None))
    assert len(positions) == 1 and len(quads) == 0
    assert np.array_equal(positions, np.full((1, 3), 1 / 6, F))   # three crossings at t = 0.5: {0.5, 0, 0}, {0, 0.5, 0}, {0, 0, 0.5}
    centre = np.ones((3, 3, 3), F)
    centre[1, 1, 1] = -1
    positions, _, quads = arrays(vpt.mesh_sdf(centre, 0.0, 1.0, device=None))
    t = topology(positions, quads)
    assert (len(positions), len(quads)) == (8, 6) and t["closed"] and t["used"] and t["chi"] == 2 and t["volume"] > 0
    for shape in ((1, 1, 1), (1, 1, 64), (5, 1, 4)):
        st = {}
        m = vpt.mesh_sdf(-np.ones(shape, F), 0.0, 1.0, device=None, stats=st)
        assert m["positions"] is None and m["quads"] is None and (st["num_vertices"], st["num_quads"]) == (0, 0)
    assert vpt.mesh_sdf(np.ones((4, 5, 6), F), 0.0, 1.0, device=None)["positions"] is None   # no sign change


def test_grids_without_cells_or_surface_look_for_no_device(vpt):
    """vpt_mesh_sdf itself, on a machine that may have no GPU: an axis of one voxel, or every voxel on one side, is answered on the host"""
    for shape, value in (((1, 1, 1), -1), ((1, 1, 64), -1), ((4, 5, 6), 1), ((4, 5, 6), -1), ((3, 3, 3), np.nan)):
        st = {"launches": -1}
        m = vpt.mesh_sdf(np.full(shape, value, F), 0.0, 1.0, device=0, stats=st)
        assert m["positions"] is None and st == {"num_vertices": 0, "num_quads": 0, "launches": 0, "device_ms": 0.0}


BAD = [("whd", dict(whd=(0, 4, 4))), ("whd", dict(whd=(4, -1, 4))), ("2^31", dict(whd=(2048, 1024, 1024))), ("finite", dict(origin=(0, np.nan, 0))),
       ("finite", dict(step=(1, 1, np.inf))), ("iso", dict(iso=np.nan)), ("step", dict(step=(1, 0, 1))), ("step", dict(step=(-1, 1, 1)))]


@pytest.mark.parametrize("word,change", BAD, ids=[f"{w}-{i}" for i, (w, _) in enumerate(BAD)])
def test_both_entries_refuse_a_bad_descriptor_before_anything_is_written(vpt, word, change):
    voxels = case("sphere")["voxels"]
    fields = dict(whd=voxels.shape[::-1], origin=(0, 0, 0), step=(1, 1, 1), iso=0.0)
    fields.update(change)
    desc = vpt.VptSdfMeshDesc((C.c_int32 * 3)(*fields["whd"]), (C.c_float * 3)(*fields["origin"]), (C.c_float * 3)(*fields["step"]), fields["iso"])
    positions, normals, quads = np.full((200, 3), 7, F), np.full((200, 3), 7, F), np.full((200, 4), 7, np.int32)
    outputs = lambda: (positions.ctypes.data, normals.ctypes.data, 200, quads.ctypes.data, 200)
    untouched = lambda st: (positions == 7).all() and (normals == 7).all() and (quads == 7).all() and (st.num_vertices, st.num_quads, st.launches) == (-5, -5, -5)
    st = vpt.VptSdfMeshStats(-5, -5, -5, 0)
    assert vpt.hip.vpt_mesh_sdf(0, C.byref(desc), voxels.ctypes.data, *outputs(), C.byref(st)) == -1   # VPT_ERR_INVALID_ARG
    message = vpt.hip.vpt_last_error().decode()
    assert message.startswith("vpt_mesh_sdf: ") and word in message and untouched(st)
    err = C.create_string_buffer(256)
    assert vpt.host.vpth_mesh_sdf(C.byref(desc), voxels.ctypes.data, None, *outputs(), C.byref(st), err, 256) == -1
    assert err.value.decode() == "mesh_sdf: " + message[len("vpt_mesh_sdf: "):] and untouched(st)


def test_null_pointers_and_bad_regions_are_refused(vpt):
    c = case("sphere")
    desc, st = vpt.VptSdfMeshDesc((C.c_int32 * 3)(9, 8, 7), (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), 0.0), vpt.VptSdfMeshStats(-5, -5, -5, 0)
    for args in ((None, c["voxels"].ctypes.data, C.byref(st)), (C.byref(desc), None, C.byref(st)), (C.byref(desc), c["voxels"].ctypes.data, None)):
        assert vpt.hip.vpt_mesh_sdf(0, args[0], args[1], None, None, 0, None, 0, args[2]) == -1
        assert "null" in vpt.hip.vpt_last_error().decode() and st.num_vertices == -5
    assert vpt.hip.vpt_mesh_sdf(0, C.byref(desc), c["voxels"].ctypes.data, None, None, -1, None, 0, C.byref(st)) == -1 and st.num_vertices == -5
    with pytest.raises(vpt.VptError, match="null voxels"):
        vpt._abi._host_call(vpt.host.vpth_mesh_sdf, C.byref(desc), None, None, None, None, 0, None, 0, C.byref(st))
    for region in (((0, 0, -1), (2, 2, 2)), ((0, 0, 0), (10, 2, 2)), ((8, 0, 0), (2, 2, 2)), ((0, 0, 0), (2, -2, 2))):
        with pytest.raises(vpt.VptError, match="the region leaves the grid"):
            vpt.mesh_sdf(c["voxels"], 0.0, 1.0, device=None, region=region)
    with pytest.raises(vpt.VptError, match="region"):
        vpt.mesh_sdf(c["voxels"], 0.0, 1.0, device=0, region=((0, 0, 0), (2, 2, 2)))
    with pytest.raises(vpt.VptError, match="voxels"):
        vpt.mesh_sdf(np.zeros((4, 4), F), 0.0, 1.0, device=None)


def test_the_capacity_convention_is_that_of_get_lights(vpt):
    """counts first; a null array is not written; an array that is given with too small a capacity is refused, counts set, nothing written"""
    c, ref = case("sphere"), replayed("sphere")
    nv, nq = len(ref["positions"]), len(ref["quads"])
    desc = vpt.VptSdfMeshDesc((C.c_int32 * 3)(*c["voxels"].shape[::-1]), (C.c_float * 3)(*c["origin"]), (C.c_float * 3)(*c["step"]), c["iso"])
    err = C.create_string_buffer(256)
    call = lambda p, n, vc, q, qc, st: vpt.host.vpth_mesh_sdf(C.byref(desc), c["voxels"].ctypes.data, None, p, n, vc, q, qc, C.byref(st), err, 256)
    st = vpt.VptSdfMeshStats()
    assert call(None, None, 0, None, 0, st) == 0 and (st.num_vertices, st.num_quads) == (nv, nq)
    positions, quads = np.full((nv, 3), 7, F), np.full((nq, 4), 7, np.int32)
    st = vpt.VptSdfMeshStats()
    assert call(positions.ctypes.data, None, nv - 1, quads.ctypes.data, nq, st) != 0
    assert err.value.decode() == f"vertex_capacity {nv - 1} < {nv} vertices" and (st.num_vertices, st.num_quads) == (nv, nq)
    assert call(positions.ctypes.data, None, nv, quads.ctypes.data, nq - 1, st) != 0
    assert err.value.decode() == f"quad_capacity {nq - 1} < {nq} quads" and (positions == 7).all() and (quads == 7).all()
    assert call(None, None, 0, quads.ctypes.data, nq, st) == 0 and np.array_equal(quads, ref["quads"]) and (positions == 7).all()
    assert call(positions.ctypes.data, None, nv + 3, None, 0, st) == 0 and positions.tobytes() == ref["positions"].tobytes()


def load_shape(vpt, directory, uri):
    """a shape file through the scene loader: a one-shape scene written beside it"""
    path = os.path.join(directory, "scene.json")
    with open(path, "w") as f:
        json.dump({"asset": {"version": "4.2"}, "cameras": [{"name": "default", "frame": [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1]}],
                   "materials": [{"name": "m"}], "shapes": [{"name": "mesh", "uri": uri}], "instances": [{"name": "mesh", "shape": 0, "material": 0}]}, f)
    return vpt.HostScene(path).shape_arrays(0)


@pytest.mark.parametrize("with_normals", [True, False])
def test_the_ply_writer_reads_back_bit_for_bit(vpt, tmp_path, with_normals):
    m = mirror(vpt, "nonfinite")   # signed zeros among its normals
    vpt.save_mesh_ply(str(tmp_path / "mesh.ply"), m["positions"], m["quads"], m["normals"] if with_normals else None)
    back = load_shape(vpt, str(tmp_path), "mesh.ply")
    assert back["positions"].tobytes() == m["positions"].tobytes() and np.array_equal(back["quads"], m["quads"])
    assert len(back["triangles"]) == 0
    if with_normals:
        assert back["normals"].tobytes() == m["normals"].tobytes()
    with pytest.raises(vpt.VptError):
        vpt.save_mesh_ply(str(tmp_path / "none" / "mesh.ply"), m["positions"], m["quads"])


def run_cli(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=120)


def test_ypathtrace_mesh_host_writes_the_python_apis_bytes(vpt, tmp_path):
    c = case("iso")
    res = 0.7
    vpt.save_volume(str(tmp_path / "grid.sdf"), c["voxels"], res)
    r = run_cli("--mesh-sdf", str(tmp_path / "grid.sdf"), "--mesh-iso", "0.1", "--mesh-host", "--output", str(tmp_path / "cli.ply"))
    assert r.returncode == 0, r.stderr
    step = np.array([F(res) * F(w) / F(w - 1) for w in c["voxels"].shape[::-1]], F)
    m = vpt.mesh_sdf(c["voxels"], 0.0, step, F(0.1), device=None)
    vpt.save_mesh_ply(str(tmp_path / "api.ply"), m["positions"], m["quads"], m["normals"])
    assert (tmp_path / "cli.ply").read_bytes() == (tmp_path / "api.ply").read_bytes()
    assert f"into {len(m['positions'])} vertices and {len(m['quads'])} quads" in r.stdout and "host mirror" in r.stdout
    assert topology(*arrays(m)[::2])["closed"]


def test_ypathtrace_refuses_mesh_options_without_mesh_sdf(tmp_path):
    for args in (("--mesh-host",), ("--mesh-iso", "0.5")):
        r = run_cli(*args, "--output", str(tmp_path / "x.ply"))
        assert r.returncode != 0 and "needs --mesh-sdf" in r.stderr and not (tmp_path / "x.ply").exists()
    r = run_cli("--mesh-sdf", str(tmp_path / "grid.sdf"), "--mesh-host")
    assert r.returncode != 0 and "missing value for output" in r.stderr
    r = run_cli("--mesh-sdf", str(tmp_path / "no_such.sdf"), "--mesh-host", "--output", str(tmp_path / "x.ply"))
    assert r.returncode != 0 and not (tmp_path / "x.ply").exists()
