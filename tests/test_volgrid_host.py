"""The volgrid shader's rule on the CPU (include/vpt.h: VPT_SHADER_VOLGRID): the host mirror of the brick majorants against a numpy
maximum, the host mirror of the density lookup against a float64 trilerp within a derived bound, density <= majorant, and the shader
name / id tables.  No GPU: the host mirror is compiled from the header the kernel compiles (csrc/vpt_volgrid_rule.h)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

DIR = os.path.join(GOLDEN, "scenes", "10_volgrid_synth")
F = np.float32
U = 2.0 ** -24   # unit roundoff of float32


def load(vpt, name):
    return vpt.HostScene(os.path.join(DIR, name + ".json"))


def clean(v):
    v = np.asarray(v)
    return np.where(np.isfinite(v) & (v > 0), v, 0).astype(v.dtype)


def numpy_majorants(voxels):
    """brick (bx, by, bz): the maximum of clean(node) over the nodes [8 b, min(8 b + 8, W - 1)] per axis; voxels (d, h, w)"""
    c = clean(voxels)
    nb = [max(1, -(-(n - 1) // 8)) for n in c.shape]
    out = np.zeros(nb, F)
    for z in range(nb[0]):
        for y in range(nb[1]):
            for x in range(nb[2]):
                out[z, y, x] = c[8 * z:8 * z + 9, 8 * y:8 * y + 9, 8 * x:8 * x + 9].max()
    return out


# ---- 1. majorants, bit for bit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,volume", [("volgrid", 0), ("constant", 0), ("ramp", 0), ("messy", 0), ("messy", 1)])
def test_host_majorants_equal_a_numpy_maximum_over_nine_node_neighbourhoods(vpt, name, volume):
    scene = load(vpt, name)
    voxels, _ = scene.volume(volume)
    got = scene.volgrid_majorants(volume)
    want = numpy_majorants(voxels)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_the_messy_grid_holds_what_clean_is_for(vpt):
    voxels, _ = load(vpt, "messy").volume(0)
    assert voxels.shape == (30, 17, 9)   # 9, 17, 30 nodes: no multiple of 8 on any axis
    assert np.isnan(voxels).any() and np.isposinf(voxels).any() and np.isneginf(voxels).any() and (voxels < 0).any() and (voxels == 0).any()
    m = load(vpt, "messy").volgrid_majorants(0)
    assert m.shape == (4, 2, 1) and np.isfinite(m).all() and (m >= 0).all()
    assert m[0, 0, 0] == 0   # a brick without one positive node


@pytest.mark.parametrize("shape", [(9, 9, 9), (17, 9, 30), (1, 5, 10), (2, 2, 2), (25, 33, 8)])
def test_host_majorants_of_edited_grids_of_odd_sizes(vpt, shape):
    scene = load(vpt, "constant")
    g = np.random.default_rng(sum(shape))
    voxels = g.uniform(-1, 2, shape).astype(F)
    voxels.reshape(-1)[::7] = np.nan
    scene.set_volume(0, voxels, res=0.1)
    scene.update_volumes()
    got, want = scene.volgrid_majorants(0), numpy_majorants(voxels)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- 2. / 3. the density lookup -----------------------------------------------------------------------------------------------------------
# The bound on |sigma_float32 - sigma_float64| for a grid of finite voxels, |v| <= V, adjacent nodes differing by at most D, in a grid
# instance whose frame is a translation (the fixtures'), from the operations of csrc/vpt_volgrid_rule.h (u = 2^-24, the unit roundoff):
#   pl = p + o          the products by 1 and 0 and the sums with 0 are exact, the sum with o rounds once: |pl| <= 2, so |d pl| <= 2 u
#   q = pl * 2 / bbox   the product by 2 is exact; the fixtures' boxes have sides >= 0.3, so pl's error arrives as <= 2 * 2 u / 0.3 < 14 u;
#                       the quotient itself (<= 2) rounds once: 2 u more
#   c = (q - 1 + 1) * 0.5   the difference and the sum round once each on values <= 2: 2 * 2 u; the product by 0.5 is exact and halves
#                       everything: |dc| <= (14 + 2 + 4) u / 2 = 10 u - the bound below keeps 20 u
#   s = c * (W - 1)     one more rounding on a value <= W - 1: |ds| <= 21 u (W - 1)
#   the trilerp is continuous and piecewise linear in (s, t, r) with slope <= D per axis, so the three coordinates cost
#                       <= 3 * 21 u (W - 1) D, whichever cells the two sides read;
#   its arithmetic: s - i is exact; 1 - u rounds once; a term is v times three weights - three products and up to three rounded
#                       weights, 6 u |v| w; the weights sum to 1, so the terms cost 6 u V; seven sums of partial sums <= V: 7 u V;
#   / trdepth           one rounding: relative u, u V more.
# In all (14 u V + 63 u (W - 1) D) / trdepth, times (1 + 1e-3) for the second-order terms.
def density_bound(voxels, trdepth):
    v = np.where(np.isfinite(voxels), voxels, 0).astype(np.float64)
    V = np.abs(v).max()
    D = max(np.abs(np.diff(v, axis=a)).max() if v.shape[a] > 1 else 0.0 for a in range(3))
    W = max(voxels.shape)
    return (14 * U * V + 63 * U * (W - 1) * D) / trdepth * (1 + 1e-3)


def reference_density(voxels, res, scalef, origin, trdepth, points):
    """float64 throughout from the float32 inputs: (sigma, inside, node coordinates); the frame is a translation by `origin`"""
    d, h, w = voxels.shape
    bbox = np.array([F(F(res) * F(n)) * F(scalef) for n in (w, h, d)], np.float64)   # the record's float32 box
    pl = points.astype(np.float64) + np.asarray(origin, np.float64)
    inside = np.all((pl >= 0) & (pl <= bbox), axis=1)
    c = np.clip((pl * 2 / bbox - 1 + 1) * 0.5, 0, 1)
    s = c * (np.array([w, h, d]) - 1)
    i = np.minimum(s.astype(np.int64), np.array([w, h, d]) - 1)
    ii = np.minimum(i + 1, np.array([w, h, d]) - 1)
    f = s - i
    vox = voxels.astype(np.float64)
    out = np.zeros(len(points))
    with np.errstate(invalid="ignore"):
        for dz, wz in ((0, 1 - f[:, 2]), (1, f[:, 2])):
            for dy, wy in ((0, 1 - f[:, 1]), (1, f[:, 1])):
                for dx, wx in ((0, 1 - f[:, 0]), (1, f[:, 0])):
                    z, y, x = (ii if dz else i)[:, 2], (ii if dy else i)[:, 1], (ii if dx else i)[:, 0]
                    out = out + vox[z, y, x] * wx * wy * wz
    out = np.where(np.isfinite(out) & (out > 0), out, 0) / np.float64(trdepth)
    return np.where(inside, out, 0), inside, s


def random_points(seed, n=4096):
    g = np.random.default_rng(seed)
    p = g.uniform(-0.25, 1.25, (n, 3)).astype(F)
    p[: n // 8] = g.uniform(0.35, 0.65, (n // 8, 3)).astype(F)   # the sparse grid's block is small: some points for certain inside it
    return p


@pytest.mark.parametrize("name", ["volgrid", "constant", "ramp"])
def test_host_density_agrees_with_a_float64_trilerp_within_the_derived_bound(vpt, name):
    scene = load(vpt, name)
    voxels, res = scene.volume(0)
    trdepth = scene.material(0).trdepth
    points = random_points(11)
    sigma, instance = scene.volgrid_density(points)
    want, inside, _ = reference_density(voxels, res, 1.0, (0, 0, 0), trdepth, points)
    assert 1000 < inside.sum() < len(points) - 1000          # both sides of the box are tested
    assert np.array_equal(instance, np.where(inside, 0, -1))
    assert np.all(sigma[~inside] == 0)                        # the density is 0 outside the box
    bound = density_bound(voxels, trdepth)
    err = np.abs(sigma.astype(np.float64) - want)
    print(f"{name}: max error {err.max():.3e}, bound {bound:.3e}, non-zero densities {np.count_nonzero(sigma)}")
    assert np.count_nonzero(sigma) > 100
    assert err.max() <= bound


def test_host_density_sums_overlapping_instances_and_divides_by_each_trdepth(vpt):
    scene = load(vpt, "overlap")
    voxels, res = scene.volume(0)
    points = random_points(12)
    sigma, instance = scene.volgrid_density(points)
    a, in_a, _ = reference_density(voxels, res, 1.0, (0, 0, 0), scene.material(0).trdepth, points)
    b, in_b, _ = reference_density(voxels, res, 1.0, (-0.25, -0.25, 0), scene.material(1).trdepth, points)
    assert np.array_equal(instance, np.where(in_a, 0, np.where(in_b, 1, -1)))
    bound = density_bound(voxels, scene.material(0).trdepth) + density_bound(voxels, scene.material(1).trdepth) + U * 2   # + the sum's rounding
    assert np.abs(sigma - (a + b)).max() <= bound
    assert (in_a & in_b).sum() > 500 and np.all(sigma[~in_a & ~in_b] == 0)


def test_host_density_cleans_what_the_trilerp_of_a_messy_grid_gives(vpt):
    scene = load(vpt, "messy")
    scene.set_volume_instance(1, frame=[1, 0, 0, 0, 1, 0, 0, 0, 1, 5, 5, 5])   # the second instance out of the way
    scene.update_volumes()
    voxels, res = scene.volume(0)
    points = (np.random.default_rng(13).uniform(-0.1, 1.1, (4096, 3)) * np.array([0.3, 17 / 30, 1.0])).astype(F)
    sigma, _ = scene.volgrid_density(points)
    want, inside, _ = reference_density(voxels, res, 1.0, (0, 0, 0), scene.material(0).trdepth, points)
    assert np.isfinite(sigma).all() and (sigma >= 0).all() and np.all(sigma[~inside] == 0)
    assert np.count_nonzero(sigma) > 200 and np.count_nonzero(sigma[inside] == 0) > 200   # NaN, Inf and negative neighbourhoods give 0
    assert np.abs(sigma - want).max() <= density_bound(voxels, scene.material(0).trdepth)


@pytest.mark.parametrize("name", ["volgrid", "ramp", "messy"])
def test_density_never_exceeds_the_brick_majorant_by_more_than_the_bound(vpt, name):
    scene = load(vpt, name)
    if name == "messy":
        scene.set_volume_instance(1, frame=[1, 0, 0, 0, 1, 0, 0, 0, 1, 5, 5, 5])
        scene.update_volumes()
    voxels, res = scene.volume(0)
    trdepth = scene.material(0).trdepth
    scale = np.array(voxels.shape[::-1]) * res
    points = (random_points(14) * scale).astype(F)
    sigma, _ = scene.volgrid_density(points)
    _, inside, s = reference_density(voxels, res, 1.0, (0, 0, 0), trdepth, points)
    m = scene.volgrid_majorants(0)
    b = np.minimum(s.astype(np.int64) // 8, np.array(m.shape[::-1]) - 1)
    major = m[b[:, 2], b[:, 1], b[:, 0]].astype(np.float64) / trdepth
    excess = (sigma - major)[inside]
    print(f"{name}: largest excess {excess.max():.3e}")
    assert excess.max() <= density_bound(voxels, trdepth)
    assert np.count_nonzero(sigma) > 100


def test_density_from_sdf_is_a_clipped_ramp(vpt):
    sdf = np.array([[[-2.0, -0.5, -0.25, 0.0, 0.25, np.inf]]], F)
    assert np.array_equal(vpt.density_from_sdf(sdf, 0.5), np.array([[[1, 1, 0.5, 0, 0, 0]]], F))
    assert vpt.density_from_sdf(sdf, 0.5).dtype == F
    with pytest.raises(vpt.VptError):
        vpt.density_from_sdf(sdf, 0.0)


def test_a_material_without_a_usable_trdepth_is_refused_by_name(vpt):
    scene = load(vpt, "constant")
    m = scene.material(0)
    m.trdepth = 0.0
    scene.set_material(0, m)
    with pytest.raises(vpt.VptError, match="vol_instance 0"):
        scene.volgrid_density(np.zeros((1, 3), F))


# ---- 4. names and ids -----------------------------------------------------------------------------------------------------------------------
def test_shader_names_and_ids(vpt):
    assert vpt.SHADER_NAMES == ["volpathtrace", "pathtrace", "naive", "eyelight", "normal", "texcoord", "color", "implicit", "implicit_normal"]
    assert vpt.EXTENSION_SHADERS == {"volgrid": 16}
    assert vpt.shader_id("volgrid") == 16 and vpt.shader_name(16) == "volgrid"
    assert vpt.PathtraceParams(shader="volgrid").to_abi().shader == 16
    assert [vpt.shader_id(n) for n in vpt.SHADER_NAMES] == list(range(9))
    for ident in list(range(9, 16)) + [-1, 17]:
        assert vpt.hip.vpt_shader_known(ident) == 0
        with pytest.raises(vpt.VptError, match="sampler unknown"):
            vpt.shader_name(ident)
    assert all(vpt.hip.vpt_shader_known(ident) == 1 for ident in list(range(9)) + [16])
    with pytest.raises(vpt.VptError, match="sampler unknown"):
        vpt.PathtraceParams(shader="raytrace").to_abi()
