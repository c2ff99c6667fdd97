"""vpt_bake_sdf on the GPU (include/vpt.h): the kernel's BVH walk must give the bits of the host mirror, which runs the same rule
header over every triangle - on grids that are no multiple of the 4^3 brick, on a single voxel, on a tree as deep as the stack
allows, on meshes with acute apexes, lopsided fans and needle triangles (the host tests hold the mirror to an exact float64 reference on
them); the BVH form must give the bits of the brute form (VPT_BAKE_BRUTE=1), also with coordinates near 1000 where the pruning
margin matters, and on 1 440 needle triangles turned out of the axes; a tree deeper than the stack is refused before any launch; a baked grid renders like the reference renders it;
and the CLI writes the file the Python API writes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bake_meshes import BIPYRAMID_TURN, TOOTHED, F, bipyramid_grid, bits, box_mesh, flat_bipyramid, icosphere, toothed_grid, torus, write_volume_scene
from conftest import ROOT
from synth_scenes import chain_geometry

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "volumetric-path-tracer_amd", "ypathtrace")
STACK = 48   # csrc/vpt_bake.hip: BAKE_STACK


@pytest.fixture(scope="module", autouse=True)
def need_device(vpt):
    if vpt.device_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible (the HIP path has no CPU fallback)")


def both(vpt, verts, tris, whd, origin, step):
    dev, stats = vpt.bake_sdf_grid(verts, tris, whd, origin, step, device=0)
    ref, _ = vpt.bake_sdf_grid(verts, tris, whd, origin, step, device=None)
    assert stats["launches"] == 1 and stats["bvh_nodes"] >= 1
    return dev, ref, stats


def test_box_equals_mirror(vpt):
    dev, ref, _ = both(vpt, *box_mesh(0.3137, 0.7211), 17, 0.0, 1 / 16)
    assert np.array_equal(bits(dev), bits(ref))
    assert int((dev < 0).sum()) == 216


@pytest.mark.parametrize("whd", [(5, 4, 3), (33, 17, 9), (1, 1, 1), (64, 1, 1)])
def test_icosphere_equals_mirror(vpt, whd):
    verts, tris = icosphere(2, 0.8, (0.1, -0.05, 0.02))
    assert len(tris) == 320
    origin = F([-1.0, -0.9, -0.7]) if whd != (1, 1, 1) else F([0.1, 0.0, 0.0])
    step = F([2.0 / max(whd[0] - 1, 1), 1.8 / max(whd[1] - 1, 1), 1.4 / max(whd[2] - 1, 1)])
    dev, ref, stats = both(vpt, verts, tris, whd, origin, step)
    assert dev.shape == whd[::-1]
    assert np.array_equal(bits(dev), bits(ref))
    assert stats["bvh_nodes"] > 100 and 6 <= stats["bvh_depth"] <= STACK
    if whd == (1, 1, 1):
        assert dev[0, 0, 0] < 0           # inside the sphere


@pytest.mark.parametrize("scale,offset", [(1.0, 0.0), (1000.0, 1000.0)])
def test_bvh_equals_brute(vpt, monkeypatch, scale, offset):
    verts, tris = torus(40, 40)
    assert len(tris) == 3200
    verts = (verts * F(scale) + F(offset)).astype(F)
    origin, step = F((-1.0) * scale + offset), F(2.0 * scale / 23)
    monkeypatch.delenv("VPT_BAKE_BRUTE", raising=False)
    bvh, s_bvh = vpt.bake_sdf_grid(verts, tris, 24, origin, step, device=0)
    monkeypatch.setenv("VPT_BAKE_BRUTE", "1")
    brute, s_brute = vpt.bake_sdf_grid(verts, tris, 24, origin, step, device=0)
    assert s_bvh["bvh_nodes"] > 1000 and s_brute["bvh_nodes"] == 0 and s_bvh["launches"] == s_brute["launches"] == 1
    assert np.array_equal(bits(bvh), bits(brute))
    assert (bvh < 0).any() and (bvh > 0).any() and np.isfinite(bvh).all()
    # the torus: |value| is the distance to a tube of radius 0.25 around a circle of radius 0.6, to the tessellation's accuracy
    g = origin + np.arange(24, dtype=np.float64) * step
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    lx, ly, lz = (x - offset) / scale, (y - offset) / scale, (z - offset) / scale
    exact = np.hypot(np.hypot(lx, ly) - 0.6, lz) - 0.25
    assert np.abs(bvh / scale - exact).max() < 0.01 and np.array_equal((bvh < 0)[np.abs(exact) > 0.01], (exact < 0)[np.abs(exact) > 0.01])


def toothed_case(case):
    """(verts, tris, whd, origin, step)"""
    if case == "bipyramid":
        return (*flat_bipyramid(), *bipyramid_grid())
    name, whd = {"spiky": ("spiky_1.0", 21), "fan": ("fan_16", (25, 21, 19))}[case]   # (25, 21, 19): lanes outside the grid on every axis
    return (*TOOTHED[name][0](), whd, *toothed_grid(name, whd))


@pytest.mark.parametrize("case", ["spiky", "fan", "bipyramid"])
def test_toothed_meshes_equal_mirror(vpt, case):
    dev, ref, stats = both(vpt, *toothed_case(case))
    assert np.array_equal(bits(dev), bits(ref))
    assert (dev < 0).sum() >= 30 and np.isfinite(dev).all()


@pytest.mark.parametrize("rim", [720, 1000])
@pytest.mark.parametrize("turn,scale,offset", [(None, 1.0, 0.0), (BIPYRAMID_TURN, 1000.0, 1000.0)])
def test_bvh_equals_brute_on_needles(vpt, monkeypatch, turn, scale, offset, rim):
    """the flat bipyramid, and its copy turned out of the axes, scaled by 1000 and moved by 1000: DESIGN.md §16's own stress case for
    the pruning margin, slivers seen from far away with coordinates where reach = 2^-14 M is 0.13.  A rim of 720 points (1 440
    needles of 1 : 115) gives a tree of 863 nodes; the rim of 1 000 (2 000 needles of 1 : 159) is there for a tree of more than 1 000."""
    verts, tris = flat_bipyramid(rim, turn=turn, scale=scale, offset=offset)
    whd, origin, step = bipyramid_grid(scale, offset)
    monkeypatch.delenv("VPT_BAKE_BRUTE", raising=False)
    bvh, s_bvh = vpt.bake_sdf_grid(verts, tris, whd, origin, step, device=0)
    monkeypatch.setenv("VPT_BAKE_BRUTE", "1")
    brute, s_brute = vpt.bake_sdf_grid(verts, tris, whd, origin, step, device=0)
    assert s_bvh["bvh_nodes"] > (1000 if rim == 1000 else 800) and s_brute["bvh_nodes"] == 0 and s_bvh["launches"] == s_brute["launches"] == 1
    assert s_bvh["dropped_triangles"] == s_brute["dropped_triangles"] == 0 and len(tris) == 2 * rim
    differ = bits(bvh) != bits(brute)
    print(f"rim {rim}, scale {scale}: {int(differ.sum())} voxels differ, {int((bvh < 0).sum())} inside, tree of {s_bvh['bvh_nodes']} nodes, depth {s_bvh['bvh_depth']}")
    assert not differ.any()
    assert (bvh < 0).sum() >= 30 and (bvh > 0).any() and np.isfinite(bvh).all()


def test_deep_tree(vpt):
    verts, tris = chain_geometry(40)
    dev, ref, stats = both(vpt, verts, tris, 9, -2.0, 0.5)
    assert stats["bvh_depth"] == 40
    assert np.array_equal(bits(dev), bits(ref))


def test_tree_deeper_than_the_stack_is_refused(vpt):
    verts, tris = chain_geometry(STACK + 2)
    verts, tris = np.ascontiguousarray(verts, F), np.ascontiguousarray(tris, np.int32)
    desc = vpt.VptBakeDesc(len(verts), verts.ctypes.data, len(tris), tris.ctypes.data, (C.c_int32 * 3)(9, 9, 9), (C.c_float * 3)(-2, -2, -2),
                           (C.c_float * 3)(0.5, 0.5, 0.5))
    out = np.full(9 ** 3, 12345.0, F)
    stats = vpt.VptBakeStats(launches=9)
    assert vpt.hip.vpt_bake_sdf(0, C.byref(desc), out.ctypes.data, C.byref(stats)) == -5   # VPT_ERR_UNSUPPORTED
    assert "traversal stack" in vpt.hip.vpt_last_error().decode()
    assert stats.launches == 0 and stats.bvh_depth == STACK + 2 and np.all(out == F(12345.0))


def test_two_calls_same_bits_inputs_unchanged(vpt):
    verts, tris = icosphere(2, 0.8)
    v0, t0 = verts.copy(), tris.copy()
    a, _ = vpt.bake_sdf_grid(verts, tris, (13, 11, 10), -1.0, 0.17, device=0)
    b, _ = vpt.bake_sdf_grid(verts, tris, (13, 11, 10), -1.0, 0.17, device=0)
    assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(verts), bits(v0)) and np.array_equal(tris, t0)


def test_baked_grid_renders(vpt, oracle, tmp_path):
    """an icosphere of radius 0.3 baked at 32^3, saved, loaded as a scene's only volume and rendered with implicit_normal on the GPU
    and by the oracle: the criterion and the floors tests/test_gpu_parity.py applies to its implicit_normal cases
    (_check_against_reference, test_gpu_parity.py:39; floors of "sdf_normal_96_2" / "sdfn_normal_128_2", :310 and :313)"""
    from test_gpu_parity import _check_against_reference
    verts, tris = icosphere(2, 0.3)
    baked = vpt.bake_sdf(verts, tris, 32, device=0)
    assert np.array_equal(bits(baked.voxels), bits(vpt.bake_sdf(verts, tris, 32, device=None).voxels))
    baked.save(str(tmp_path / "sphere.sdf"))
    write_volume_scene(tmp_path / "scene.json", "sphere.sdf", baked.frame, baked.scalef)
    scene = vpt.HostScene(str(tmp_path / "scene.json"))
    dev = vpt.DeviceScene(scene, 0)
    spp = 2
    p = vpt.PathtraceParams(resolution=48, samples=spp, shader="implicit_normal", bounces=4)
    g = scene.make_state(p)
    dev.pathtrace_samples(g, p, spp)
    ref = scene.make_state(p)
    oracle.oracle_render(scene, p, ref, spp, nthreads=0)
    _check_against_reference(oracle, scene, p, spp, g, ref.image, ref.rngs, "baked_sphere_normal_48_2", 0.998, 0.998, 0.998)
    cy, cx = g.height // 2, g.width // 2
    assert g.hits[cy, cx] == spp
    # the centre pixel's rays meet the sphere within 0.03 of its axis, where the true normal is within 6 degrees of +z; the gradient
    # of a trilinear 32^3 grid is piecewise, so this only asks for a normal within 25 degrees of +z: n * 0.5 + 0.5 with n.z >= 0.9
    colour = vpt.get_render(g)[cy, cx, :3]
    print("centre pixel", colour)
    assert colour[2] >= 0.95 and abs(colour[0] - 0.5) <= 0.21 and abs(colour[1] - 0.5) <= 0.21
    assert np.allclose(vpt.get_render(g)[0, 0, :3], vpt.get_render(ref)[0, 0, :3])   # and a corner ray misses it on both


def test_cli_writes_the_same_file(vpt, scene03, tmp_path):
    shape = scene03.shape_arrays(1)   # 03_volume's sphere.ply as the host loader reads it: 6144 quads
    assert len(shape["positions"]) == 6534 and len(shape["quads"]) == 6144
    ply = os.path.join(ROOT, "tests", "golden", "scenes", "03_volume", "shapes", "sphere.ply")
    files = {}
    for device, flags in ((0, []), (None, ["--bake-host"])):
        out = tmp_path / f"cli_{device}.sdf"
        r = subprocess.run([BIN, "--bake-sdf", ply, "--bake-res", "16", "--output", str(out)] + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        baked = vpt.bake_sdf(shape["positions"], shape["quads"], 16, device=device)
        baked.save(str(tmp_path / f"py_{device}.sdf"))
        files[device] = out.read_bytes()
        assert files[device] == (tmp_path / f"py_{device}.sdf").read_bytes()
        assert f"res: {baked.res:.9g}" in r.stdout and '"frame": [1, 0, 0, 0, 1, 0, 0, 0, 1, ' in r.stdout
    assert files[0] == files[None] and len(files[0]) == 80 + 4 * 16 ** 3
