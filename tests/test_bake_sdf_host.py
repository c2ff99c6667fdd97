"""Baking a mesh into a signed-distance grid without a GPU (include/vpt.h: vpt_bake_sdf).  The host mirror (bake_sdf with device None:
csrc/vpt_bake_rule.h over every voxel and every triangle) against the exact distance to a box, and against an independent float64
reference (tests/sdf_exact.py: plane and segment distances, winding numbers) on meshes with acute apexes, concave valleys, saddles,
lopsided fans and needle triangles, where a wrong pseudonormal is a wrong sign; the properties the rule promises -
adjacency by position bits, independence of the triangle order, +0 on the surface, finite values on an open mesh, dropped triangles;
fit_volume and save_volume against the scene loader; and every refusal of the C-ABI with its message."""
import ctypes as C

import numpy as np
import pytest

import sdf_exact as X
from bake_meshes import TOOTHED, F, bipyramid_grid, bits, box_mesh, check_outward, flat_bipyramid, toothed_grid, unweld, write_volume_scene

LO, HI = 0.3137, 0.7211


@pytest.fixture(scope="module")
def box():
    verts, tris = box_mesh(LO, HI)
    assert verts.shape == (8, 3) and tris.shape == (12, 3) and check_outward(verts, tris)
    return verts, tris


@pytest.fixture(scope="module")
def box17(vpt, box):
    """the box on the 17^3 grid with origin 0 and step 1/16, by the mirror: baked once, shared, never written to"""
    voxels, stats = vpt.bake_sdf_grid(*box, 17, 0.0, 1 / 16, device=None)
    voxels.setflags(write=False)
    return voxels, stats


def exact_box_distance(verts, n, step):
    """float64 signed distance to the box spanned by the (float32) vertices at the n^3 grid points k * step: array [z, y, x]"""
    lo, hi = verts.astype(np.float64).min(axis=0), verts.astype(np.float64).max(axis=0)
    g = np.arange(n, dtype=np.float64) * step
    p = np.stack(np.meshgrid(g, g, g, indexing="ij")[::-1], axis=-1)   # [z, y, x] -> (x, y, z)
    q = np.abs(p - (lo + hi) / 2) - (hi - lo) / 2
    return np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(axis=-1), 0)


def test_analytic_box(box, box17):
    voxels, stats = box17
    exact = exact_box_distance(box[0], 17, 1 / 16)
    assert voxels.shape == exact.shape == (17, 17, 17) and voxels.dtype == np.float32
    # no grid point near a face (0.3137 - 5/16 = 1.2e-3, less the float32 rounding of the corner): all 4913 voxels take part in both comparisons
    assert np.abs(exact).min() > 1.1999e-3
    assert int((exact < 0).sum()) == 216
    assert np.array_equal(voxels < 0, exact < 0) and np.array_equal(np.signbit(voxels), exact < 0)
    err = float(np.abs(voxels.astype(np.float64) - exact).max())
    print(f"max |mirror - exact| = {err:.3g}")
    assert err <= 1e-6
    assert stats["dropped_triangles"] == 0


def test_duplicated_vertices_weld_by_position(vpt, box, box17):
    verts, tris = unweld(*box)
    assert verts.shape == (36, 3)
    voxels, _ = vpt.bake_sdf_grid(verts, tris, 17, 0.0, 1 / 16, device=None)
    assert np.array_equal(bits(voxels), bits(box17[0]))
    # a vertex at -0 is the vertex at +0: the cube [0, 0.5]^3 with one copy of its corners written as -0
    cv, ct = box_mesh(0.0, 0.5)
    welded, _ = vpt.bake_sdf_grid(cv, ct, 9, -0.25, 1 / 8, device=None)
    uv, ut = unweld(cv, ct)
    uv[::2][uv[::2] == 0] = -0.0
    assert np.signbit(uv).any()
    split, _ = vpt.bake_sdf_grid(uv, ut, 9, -0.25, 1 / 8, device=None)
    assert np.array_equal(bits(split), bits(welded))


def test_triangle_order(vpt, box, box17):
    verts, tris = box
    for seed in (1, 2):
        order = np.random.default_rng(seed).permutation(len(tris))
        voxels, _ = vpt.bake_sdf_grid(verts, tris[order], 17, 0.0, 1 / 16, device=None)
        assert np.array_equal(bits(voxels), bits(box17[0]))


def test_cube_on_grid_points(vpt):
    verts, tris = box_mesh(0.25, 0.75)
    voxels, _ = vpt.bake_sdf_grid(verts, tris, 9, 0.0, 1 / 8, device=None)
    k = np.arange(9)
    z, y, x = np.meshgrid(k, k, k, indexing="ij")
    cheb = np.maximum(np.maximum(np.abs(x - 4), np.abs(y - 4)), np.abs(z - 4))   # 2: on the surface
    assert np.all(bits(voxels)[cheb == 2] == 0)                                  # +0, not -0
    assert np.all(voxels[cheb < 2] < 0) and np.all(voxels[cheb > 2] > 0)
    assert voxels[4, 4, 4] == F(-0.25) and voxels[4, 4, 0] == F(0.25) and voxels[0, 0, 0] == F(np.sqrt(F(3 * 0.25 ** 2)))


def test_open_mesh(vpt, box):
    verts, tris = box
    top = np.all(verts[tris][:, :, 1] == verts[:, 1].max(), axis=1)
    assert top.sum() == 2
    voxels, _ = vpt.bake_sdf_grid(verts, tris[~top], 17, 0.0, 1 / 16, device=None)
    assert np.isfinite(voxels).all()
    assert np.all(voxels[:, :5, :] > 0)   # below the floor plane y = 0.3137 (rows 0..4), outside the box


def test_zero_cross_product(vpt, box, box17):
    verts, tris = box
    v2 = np.concatenate([verts, np.array([[0, 0, 0], [0.5, 0.5, 0.5], [1, 1, 1]], F)])
    t2 = np.concatenate([tris[:5], [[8, 9, 10]], tris[5:]]).astype(np.int32)
    voxels, stats = vpt.bake_sdf_grid(v2, t2, 17, 0.0, 1 / 16, device=None)
    assert stats["dropped_triangles"] == 1
    assert np.array_equal(bits(voxels), bits(box17[0]))
    normals, kept = np.full((len(t2), 21), 7, F), np.full(len(t2), 7, np.int32)
    desc, _keep = _desc(vpt, v2, t2, (17, 17, 17), (0, 0, 0), (1 / 16,) * 3)
    assert vpt.hip.vpt_bake_feature_normals(C.byref(desc), normals.ctypes.data, kept.ctypes.data) == 0
    assert kept.tolist() == [1] * 5 + [0] + [1] * 7 and np.all(normals[5] == 0)
    with pytest.raises(vpt.VptError, match="zero cross product"):
        vpt.bake_sdf_grid(v2, [[8, 9, 10], [8, 8, 9]], 17, 0.0, 1 / 16, device=None)


def test_feature_normals_of_the_box(vpt, box):
    """face: the unit normal; edge: the sum of its two faces' normals; vertex: angle-weighted sum - the box's are known in closed form"""
    verts, tris = box
    desc, _keep = _desc(vpt, verts, tris, (2, 2, 2), (0, 0, 0), (1, 1, 1))
    normals = np.zeros((12, 7, 3), F)
    assert vpt.hip.vpt_bake_feature_normals(C.byref(desc), normals.ctypes.data, None) == 0
    c = verts.astype(np.float64).mean(axis=0)
    for t, tri in enumerate(tris):
        p = verts[tri].astype(np.float64)
        n = np.cross(p[1] - p[0], p[2] - p[0])
        assert np.allclose(normals[t, 0], n / np.linalg.norm(n), atol=1e-7)
        for e, (i, j) in enumerate([(0, 1), (1, 2), (2, 0)]):
            out = np.sign(np.round((p[i] + p[j]) / 2 - c, 6))   # a box edge: the two faces' normals; a face diagonal: twice the face's
            expect = out if np.count_nonzero(out) == 2 else 2 * n / np.linalg.norm(n)
            assert np.allclose(normals[t, 1 + e], expect, atol=1e-6)
        for k in range(3):   # three right angles meet at a corner, however the faces are cut
            assert np.allclose(normals[t, 4 + k], np.sign(p[k] - c) * np.pi / 2, atol=1e-6)


def test_fit_and_save_round_trip(vpt, box, tmp_path):
    verts, tris = box
    verts = verts * F([1.0, 0.5, 0.75]) + F([0.3, -0.2, 0.1])
    whd, padding = (11, 9, 8), 2
    baked = vpt.bake_sdf(verts, tris, whd, padding=padding, device=None)
    assert baked.voxels.shape == (8, 9, 11) and baked.scalef == 1.0
    res, origin, step, frame = vpt.fit_volume(verts.min(axis=0), verts.max(axis=0), whd, padding)
    assert res == baked.res and np.array_equal(frame, baked.frame)
    assert np.array_equal(frame[:3], np.eye(3, dtype=F)) and np.array_equal(frame[3], -origin)
    for a in range(3):
        w = whd[a]
        assert step[a] == F(F(F(res) * F(w)) / F(w - 1))                      # the step formula
        last, full = F(F(w - 1) * step[a]), F(F(res) * F(w))                    # voxel W - 1 sits at res * W
        assert abs(float(last) - float(full)) <= float(np.spacing(full))
        assert origin[a] + padding * step[a] <= verts[:, a].min() + 1e-6        # `padding` voxels to spare on each side
        assert origin[a] + (w - 1 - padding) * step[a] >= verts[:, a].max() - 1e-6
    tight = max((verts[:, a].max() - verts[:, a].min()) * (whd[a] - 1) / (whd[a] * (whd[a] - 1 - 2 * padding)) for a in range(3))
    assert tight <= res <= tight * (1 + 1e-6)                                   # the smallest res that fits
    grid, _ = vpt.bake_sdf_grid(verts, tris, whd, origin, step, device=None)
    assert np.array_equal(bits(grid), bits(baked.voxels))
    baked.save(str(tmp_path / "baked.sdf"))
    raw = (tmp_path / "baked.sdf").read_bytes()
    assert len(raw) == 80 + 4 * 11 * 9 * 8 and np.frombuffer(raw, np.int32, 3).tolist() == [11, 9, 8]
    assert np.array_equal(np.frombuffer(raw, F, 16, 16), np.eye(4, dtype=F).reshape(-1))
    write_volume_scene(tmp_path / "scene.json", "baked.sdf", baked.frame, baked.scalef)
    scene = vpt.HostScene(str(tmp_path / "scene.json"))
    loaded, loaded_res = scene.volume(0)
    assert loaded.shape == (8, 9, 11) and F(loaded_res) == F(baked.res)
    assert np.array_equal(bits(loaded), bits(baked.voxels))
    with pytest.raises(vpt.VptError, match="padding"):
        vpt.fit_volume([0, 0, 0], [1, 1, 1], (11, 6, 8), 2)


def test_quads_split_like_the_reference(vpt):
    quads = np.array([[0, 1, 2, 3], [4, 5, 6, 6]], np.int32)
    assert vpt.bake_triangles(quads).tolist() == [[0, 1, 3], [2, 3, 1], [4, 5, 6]]
    assert vpt.bake_triangles(quads[:, :3]).tolist() == quads[:, :3].tolist()


# ---- against the exact float64 reference (tests/sdf_exact.py), on meshes where a wrong pseudonormal is a wrong sign ------------------
@pytest.fixture(scope="module")
def toothed(vpt):
    """(name, n) -> (verts, tris, exact signed distance, inside, the mirror's voxels) on the n^3 grid: computed once, never written to.
    From the reference alone: the mesh is closed (winding numbers are integers), some voxels are inside, none lies within 1e-5 of
    the surface - ten times the distance bar - so every voxel takes part in the sign comparison."""
    cache = {}

    def get(name, n):
        if (name, n) not in cache:
            verts, tris = TOOTHED[name][0]()
            origin, step = toothed_grid(name, n)
            exact, inside = X.signed_distance(X.sample_points(n, origin, step), verts, tris)
            assert np.abs(exact).min() >= 1e-5 and 40 <= inside.sum() < inside.size // 4
            mirror, stats = vpt.bake_sdf_grid(verts, tris, n, origin, step, device=None)
            assert stats["dropped_triangles"] == 0
            for a in (verts, tris, exact, inside, mirror):
                a.setflags(write=False)
            cache[name, n] = (verts, tris, exact, inside, mirror)
        return cache[name, n]
    return get


@pytest.mark.parametrize("n", [21, 25])
@pytest.mark.parametrize("name", list(TOOTHED))
def test_mirror_equals_exact(toothed, name, n):
    """sign = the winding number's on every voxel, |value| = the distance to 1e-6, the bar of test_analytic_box (coordinates <= 1.02).
    Measured: at most 2.1e-7 over the ten cases.  With |p - c| on the face, as the rule first stood, fan_16 gave 1.08e-6 at 21^3 and
    3.44e-6 at 25^3 (one voxel 1.8e-4 from a 1 : 37 triangle of the fan)."""
    verts, tris, exact, inside, mirror = toothed(name, n)
    assert mirror.shape == exact.shape == (n, n, n)
    wrong = int((np.signbit(mirror) != inside).sum())
    err = float(np.abs(mirror.astype(np.float64) - exact).max())
    print(f"{name} {n}^3: {len(tris)} triangles, {int(inside.sum())} voxels inside, min |exact| = {np.abs(exact).min():.3g}, wrong signs {wrong}, "
          f"max |mirror - exact| = {err:.3g}")
    assert wrong == 0
    assert err <= 1e-6


@pytest.mark.parametrize("name", ["fan_8", "fan_16", "spiky_0.8_fine"])
def test_feature_normals_equal_exact(vpt, name):
    verts, tris = TOOTHED[name][0]()
    desc, _keep = _desc(vpt, verts, tris, (2, 2, 2), (0, 0, 0), (1, 1, 1))
    normals = np.zeros((len(tris), 7, 3), F)
    assert vpt.hip.vpt_bake_feature_normals(C.byref(desc), normals.ctypes.data, None) == 0
    want = X.feature_normals(verts, tris)
    assert np.allclose(normals, want, rtol=0, atol=1e-6), float(np.abs(normals - want).max())
    # the reference's table tells the features apart: a fan's apex sums many narrow angles, its edges two different faces
    assert np.abs(want[:, 4:] - want[:, :1]).max() > 0.1 and np.abs(want[:, 1:4] - 2 * want[:, :1]).max() > 0.1


def test_boundary_edge_normal_is_its_face_normal(vpt):
    """fan_8 without its side (apex, B1, B2): the edges apex-B2 and B1-B2 have one face left, and their normals are that face's"""
    verts, tris = TOOTHED["fan_8"][0]()
    assert tris[16].tolist() == [0, 10, 1] and tris[17].tolist() == [0, 1, 2] and tris[15].tolist() == [1, 10, 9]
    opened = np.delete(tris, 16, axis=0)
    desc, _keep = _desc(vpt, verts, opened, (2, 2, 2), (0, 0, 0), (1, 1, 1))
    normals = np.zeros((len(opened), 7, 3), F)
    assert vpt.hip.vpt_bake_feature_normals(C.byref(desc), normals.ctypes.data, None) == 0
    assert np.array_equal(normals[16, 1], normals[16, 0])                      # (apex, B2, B0): its edge ab is apex-B2
    assert np.array_equal(normals[15, 1], normals[15, 0])                      # (B2, B1, P7): its edge ab is B2-B1
    assert not np.allclose(normals[16, 3], normals[16, 0], atol=0.1)           # B0-apex still has two faces
    assert np.allclose(normals, X.feature_normals(verts, opened), rtol=0, atol=1e-6)


def test_duplicated_vertices_weld_by_position_on_a_spiky_mesh(vpt, toothed):
    """as test_duplicated_vertices_weld_by_position - but here a weld that fails turns edge and vertex normals into face normals and
    hundreds of signs with them, so the bits are held to the exact signs as well"""
    verts, tris, exact, inside, welded = toothed("spiky_1.0", 21)
    origin, step = toothed_grid("spiky_1.0", 21)
    uv, ut = unweld(verts, tris)
    assert uv.shape == (180, 3)
    split, _ = vpt.bake_sdf_grid(uv, ut, 21, origin, step, device=None)
    assert np.array_equal(bits(split), bits(welded)) and np.array_equal(np.signbit(split), inside)
    zeros = np.flatnonzero(uv.reshape(-1) == 0)
    assert len(zeros) >= 20
    uv.reshape(-1)[zeros[::2]] = -0.0
    assert np.signbit(uv.reshape(-1)[zeros]).sum() == (len(zeros) + 1) // 2
    split, _ = vpt.bake_sdf_grid(uv, ut, 21, origin, step, device=None)
    assert np.array_equal(bits(split), bits(welded)) and np.array_equal(np.signbit(split), inside)


def test_triangle_order_of_a_fan(vpt, toothed):
    verts, tris, exact, inside, mirror = toothed("fan_16", 21)
    origin, step = toothed_grid("fan_16", 21)
    for seed in (1, 2):
        order = np.random.default_rng(seed).permutation(len(tris))
        assert not np.array_equal(order, np.arange(len(tris)))
        voxels, _ = vpt.bake_sdf_grid(verts, tris[order], 21, origin, step, device=None)
        assert np.array_equal(bits(voxels), bits(mirror))


def test_flat_bipyramid(vpt):
    """1 440 needle triangles (1 : 115) that meet at the rim under 2.3 degrees, on a 24^3 slab around the disc.  Signs equal to the
    winding number's wherever |exact| >= 1e-3, which leaves out at most 2 % of the voxels (0.91 % here; in fact no sign is wrong on
    any voxel, the nearest 3.4e-5 from the surface).  Distance: max |mirror - exact| measured 5.4e-8 against the float64 reference;
    asserted at twice that."""
    verts, tris = flat_bipyramid()
    assert len(tris) == 1440
    n, origin, step = bipyramid_grid()
    exact, inside = X.signed_distance(X.sample_points(n, origin, step), verts, tris)
    far = np.abs(exact) >= 1e-3
    assert np.abs(exact).min() >= 1e-5 and (~far).mean() <= 0.02 and inside.sum() >= 400 and (inside & far).sum() >= 300
    mirror, stats = vpt.bake_sdf_grid(verts, tris, n, origin, step, device=None)
    assert stats["dropped_triangles"] == 0
    wrong = np.signbit(mirror) != inside
    err = float(np.abs(mirror.astype(np.float64) - exact).max())
    print(f"flat bipyramid: {int(inside.sum())} voxels inside, {(~far).mean():.2%} nearer than 1e-3, wrong signs {int(wrong.sum())} "
          f"({int(wrong[far].sum())} beyond 1e-3), max |mirror - exact| = {err:.3g}")
    assert not wrong[far].any()
    assert err <= 2 * 5.4e-8


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _desc(vpt, verts, tris, whd, origin, step):
    verts, tris = np.ascontiguousarray(verts, F), np.ascontiguousarray(tris, np.int32)
    d = vpt.VptBakeDesc(len(verts), verts.ctypes.data, len(tris), tris.ctypes.data, (C.c_int32 * 3)(*whd), (C.c_float * 3)(*origin), (C.c_float * 3)(*step))
    return d, (verts, tris)


def _refusals(box):
    verts, tris = box
    nan_v, inf_v = verts.copy(), verts.copy()
    nan_v[3, 1], inf_v[7, 2] = np.nan, np.inf
    high, neg = tris.copy(), tris.copy()
    high[4, 2], neg[0, 0] = 8, -1
    ok = dict(verts=verts, tris=tris, whd=(3, 3, 3), origin=(0, 0, 0), step=(0.5, 0.5, 0.5))
    return [
        ("null positions", dict(ok, null="positions"), "positions"),
        ("null triangles", dict(ok, null="triangles"), "triangles"),
        ("no triangles", dict(ok, tris=tris[:0]), "num_triangles 0 < 1"),
        ("index too high", dict(ok, tris=high), "triangle 4 names vertex 8 of 8"),
        ("negative index", dict(ok, tris=neg), "triangle 0 names vertex -1"),
        ("NaN position", dict(ok, verts=nan_v), "vertex 3 has a component that is not finite"),
        ("inf position", dict(ok, verts=inf_v), "vertex 7 has a component that is not finite"),
        ("inf origin", dict(ok, origin=(0, np.inf, 0)), "origin[1] is not finite"),
        ("NaN step", dict(ok, step=(0.5, 0.5, np.nan)), "step[2] is not finite"),
        ("zero size", dict(ok, whd=(3, 0, 3)), "whd[1] = 0 < 1"),
        ("negative size", dict(ok, whd=(-3, 3, 3)), "whd[0] = -3 < 1"),
        ("2^31 voxels", dict(ok, whd=(2048, 2048, 512)), "2^31 voxels or more"),
        ("only dropped triangles", dict(ok, tris=np.array([[0, 0, 1], [2, 2, 2]], np.int32)), "zero cross product"),
    ]


@pytest.mark.parametrize("case", range(13))
def test_validation(vpt, box, case):
    """every refusal comes before a device is looked for (this runs without one), is VPT_ERR_INVALID_ARG, names the entry point and
    what is wrong, and leaves the output untouched - through the C-ABI and through the mirror"""
    name, a, text = _refusals(box)[case]
    desc, _keep = _desc(vpt, a["verts"], a["tris"], a["whd"], a["origin"], a["step"])
    if a.get("null"):
        setattr(desc, a["null"], None)
    out = np.full(64, 12345.0, F)
    stats = vpt.VptBakeStats(launches=9)
    assert vpt.hip.vpt_bake_sdf(0, C.byref(desc), out.ctypes.data, C.byref(stats)) == -1, name
    msg = vpt.hip.vpt_last_error().decode()
    assert msg.startswith("vpt_bake_sdf: ") and text in msg, (name, msg)
    assert np.all(out == F(12345.0)) and stats.launches == 0
    normals = np.full(21 * max(1, len(a["tris"])), 12345.0, F)
    assert vpt.hip.vpt_bake_feature_normals(C.byref(desc), normals.ctypes.data, None) == -1
    msg = vpt.hip.vpt_last_error().decode()
    assert msg.startswith("vpt_bake_feature_normals: ") and text in msg and np.all(normals == F(12345.0))
    if not a.get("null"):   # the mirror takes arrays, not pointers
        err = C.create_string_buffer(512)
        whd, origin, step = np.array(a["whd"], np.int32), np.array(a["origin"], F), np.array(a["step"], F)
        verts, tris = _keep
        assert vpt.host.vpth_bake_grid(verts.ctypes.data, len(verts), tris.ctypes.data, len(tris), whd.ctypes.data, origin.ctypes.data, step.ctypes.data,
                                       -1, out.ctypes.data, None, err, len(err)) == -1
        assert text in err.value.decode() and np.all(out == F(12345.0))


def test_null_outputs(vpt, box):
    desc, _keep = _desc(vpt, *box, (3, 3, 3), (0, 0, 0), (0.5, 0.5, 0.5))
    assert vpt.hip.vpt_bake_sdf(0, C.byref(desc), None, None) == -1 and "null voxels" in vpt.hip.vpt_last_error().decode()
    assert vpt.hip.vpt_bake_feature_normals(C.byref(desc), None, None) == -1 and "null normals" in vpt.hip.vpt_last_error().decode()
    assert vpt.hip.vpt_bake_sdf(0, None, None, None) == -1 and "null descriptor" in vpt.hip.vpt_last_error().decode()


# ---- the CLI without a GPU ---------------------------------------------------------------------------------------------------------
def _cli(*args):
    import os
    import subprocess
    from conftest import ROOT
    return subprocess.run([os.path.join(ROOT, "volumetric-path-tracer_amd", "ypathtrace"), *args], capture_output=True, text=True, timeout=120)


def test_cli_bake_host(vpt, scene03, tmp_path):
    """--bake-sdf --bake-host writes the file the Python mirror writes, prints res and the instance entry, and renders nothing"""
    import os
    from conftest import GOLDEN
    ply = os.path.join(GOLDEN, "scenes", "03_volume", "shapes", "sphere.ply")
    r = _cli("--bake-sdf", ply, "--bake-res", "9", "--bake-padding", "1", "--bake-host", "--output", str(tmp_path / "cli.sdf"))
    assert r.returncode == 0, r.stderr
    shape = scene03.shape_arrays(1)
    baked = vpt.bake_sdf(shape["positions"], shape["quads"], 9, padding=1, device=None)
    baked.save(str(tmp_path / "py.sdf"))
    assert (tmp_path / "cli.sdf").read_bytes() == (tmp_path / "py.sdf").read_bytes()
    assert f"res: {baked.res:.9g}" in r.stdout and '"vol_instances"' not in r.stdout and '"frame": [1, 0, 0, 0, 1, 0, 0, 0, 1, ' in r.stdout
    assert (baked.voxels < 0).any() and baked.voxels[0, 0, 0] > 0


def test_cli_bake_options(tmp_path):
    r = _cli("--bake-res", "16")
    assert r.returncode == 1 and "option bake-res needs --bake-sdf" in r.stderr
    r = _cli("--bake-sdf", "x.ply", "--output", str(tmp_path / "o.sdf"))
    assert r.returncode == 1 and "missing value for bake-res" in r.stderr
    r = _cli("--bake-sdf", "x.ply", "--bake-res", "6", "--output", str(tmp_path / "o.sdf"))
    assert r.returncode == 1 and "bad value for bake-res" in r.stderr          # 6 < 2 * padding + 3
    r = _cli("--bake-sdf", str(tmp_path / "missing.ply"), "--bake-res", "8", "--bake-host", "--output", str(tmp_path / "o.sdf"))
    assert r.returncode == 1 and "missing.ply" in r.stderr and not (tmp_path / "o.sdf").exists()
    assert "--bake-sdf" in _cli("--help").stdout
