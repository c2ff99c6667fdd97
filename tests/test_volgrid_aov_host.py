"""The first-collision pass of the volgrid shader on the CPU (include/vpt.h: vpt_render_volgrid_aov_device): the gradient behind its
`normal` plane, through the host mirror of csrc/vpt_volgrid_rule.h (HostScene.volgrid_gradient), against a float64 analytic gradient of
the trilerp; and the closed forms the statistical GPU test holds the pass to, checked against
flights drawn from the reference distribution itself.  No GPU."""
import numpy as np
import pytest

from test_volgrid_exact_host import scene_rotated
from test_volgrid_host import F, U, clean, load

# The bound on |g_float32 - g_float64| per component of the WORLD gradient, from the operations of the rule header (u = 2^-24).  The
# reference takes the cell the rule reads (a gradient jumps across a node plane: there is no bound between different cells) and
# evaluates that cell's polynomial in float64 from the float32 inputs.  With the cleaned nodes' largest adjacent difference D1, the
# largest difference of two parallel edge differences of a cell D2, K = max (W - 1) / bbox and M the largest |partial sum| of the frame:
#   pl       three products and three sums on values <= M: |d pl| <= 6 u M
#   s        test_volgrid_host.py's chain: q = pl * 2 / bbox costs 2 |d pl| / bbox + 2 u, the two sums 4 u, the half halves them, the
#            product by W - 1 rounds once more: |ds| <= ((2 * 6 u M / bbox + 6 u) / 2 + u) (W - 1)
#   cell     a component is bilinear in the two other fractions with slope <= D2 per fraction: 2 |ds| D2; its arithmetic: an edge
#            difference (1 rounding), two weights 1 - f (1 each), two products: 5 u per term, the weights sum to 1: 5 u D1; three
#            sums of partial sums <= D1: 3 u D1
#   scale    (W - 1) / bbox rounds once, the product once: 2 u K D1 on top of K times the cell's error
#   frame    three products by entries <= 1 and two sums over |gl| <= K D1 each: 5 u * 3 K D1, and the three errors of gl add up
# times (1 + 1e-3) for the second-order terms.
def gradient_bound(voxels, whd, bbox, M):
    v = clean(voxels).astype(np.float64)
    d = [np.abs(np.diff(v, axis=a)) for a in range(3)]
    D1 = max(x.max() for x in d)
    D2 = max(np.abs(np.diff(np.diff(v, axis=a), axis=b)).max() for a in range(3) for b in range(3) if a != b)
    K = ((whd - 1) / bbox).max()
    ds = (((2 * 6 * U * M / bbox + 6 * U) / 2 + U) * (whd - 1)).max()
    cell = 2 * ds * D2 + 8 * U * D1
    return (3 * (K * cell + 2 * U * K * D1) + 15 * U * K * D1) * (1 + 1e-3)


def reference_gradient(voxels, res, scalef, frame, points):
    """(world gradient (n, 3) float64, inside (n,)) of the trilerp of the cleaned nodes; the cell and `inside` are the float32 rule's"""
    whd = np.array(voxels.shape[::-1])
    bbox32 = np.array([F(F(F(res) * F(n)) * F(scalef)) for n in whd], F)
    f = np.asarray(frame, F)
    p = points.astype(F)
    pl32 = np.stack([F(F(F(f[k] * p[:, 0]) + F(f[3 + k] * p[:, 1])) + F(f[6 + k] * p[:, 2])) + f[9 + k] for k in range(3)], axis=1)
    inside = np.all((pl32 >= 0) & (pl32 <= bbox32), axis=1)
    c32 = np.clip((((pl32 * F(2)) / bbox32 - F(1)) + F(1)) * F(0.5), F(0), F(1))
    i = np.minimum((c32 * (whd - 1).astype(F)).astype(np.int64), whd - 1)         # the cell the rule reads
    ii = np.minimum(i + 1, whd - 1)
    f64, bbox = f.astype(np.float64), bbox32.astype(np.float64)
    pl = p.astype(np.float64) @ f64[:9].reshape(3, 3) + f64[9:]
    fr = np.clip(pl / bbox, 0, 1) * (whd - 1) - i
    v = clean(voxels).astype(np.float64)
    g = np.zeros((len(p), 3))
    for a in range(3):
        b, c = [k for k in range(3) if k != a]
        for db in (0, 1):
            for dc in (0, 1):
                lo, hi = [None] * 3, [None] * 3
                lo[a], hi[a] = i[:, a], ii[:, a]
                lo[b] = hi[b] = (ii if db else i)[:, b]
                lo[c] = hi[c] = (ii if dc else i)[:, c]
                wgt = (fr[:, b] if db else 1 - fr[:, b]) * (fr[:, c] if dc else 1 - fr[:, c])
                g[:, a] += (v[hi[2], hi[1], hi[0]] - v[lo[2], lo[1], lo[0]]) * wgt
    g = g * (whd - 1) / bbox
    return np.where(inside[:, None], g @ f64[:9].reshape(3, 3).T, 0), inside


def points_in(voxels, res, scalef, frame, seed):
    """world points of an instance: inside cells, on node planes of each axis, on the box's faces, and a few outside"""
    g = np.random.default_rng(seed)
    whd = np.array(voxels.shape[::-1])
    bbox = np.array([F(F(F(res) * F(n)) * F(scalef)) for n in whd], np.float64)
    local = g.uniform(0, 1, (3072, 3)) * bbox
    for k in range(3):
        rows = slice(512 * k, 512 * k + 256)
        local[rows, k] = g.integers(0, whd[k], 256) * bbox[k] / (whd[k] - 1)          # node planes, the first and the last included
        local[512 * k + 256:512 * k + 320, k] = np.where(g.uniform(size=64) < 0.5, 0.0, bbox[k])   # the faces
    local[2900:] = g.uniform(-0.3, 1.3, (172, 3)) * bbox
    f = np.asarray(frame, np.float64)
    R = f[:9].reshape(3, 3)                                                             # local = p @ R + o, R orthonormal
    return ((local - f[9:]) @ R.T).astype(F)


CASES = {"ramp": lambda vpt: load(vpt, "ramp"), "messy": lambda vpt: load(vpt, "messy"), "rotated": scene_rotated}


@pytest.mark.parametrize("name", list(CASES))
def test_the_rule_gradient_agrees_with_a_float64_analytic_gradient_within_the_derived_bound(vpt, name):
    scene = CASES[name](vpt)
    vi = scene.volume_instance(0)
    voxels, res = scene.volume(vi.volume)
    frame = [*vi.frame.x, *vi.frame.y, *vi.frame.z, *vi.frame.o]
    if name == "messy":
        assert not np.isfinite(voxels).all() and (voxels < 0).any()      # the gradient is that of the cleaned nodes
    points = points_in(voxels, res, vi.scalef, frame, 31)
    got, normal, inside = scene.volgrid_gradient(0, points)
    want, ref_inside = reference_gradient(voxels, res, vi.scalef, frame, points)
    assert np.array_equal(inside, ref_inside) and 2500 < inside.sum() < len(points)
    assert np.all(got[~inside] == 0) and np.all(normal[~inside] == 0) and np.isfinite(got).all()
    whd = np.array(voxels.shape[::-1])
    bbox = np.array([F(F(F(res) * F(n)) * F(vi.scalef)) for n in whd], np.float64)
    M = np.abs(points).max() * 3 + np.abs(frame[9:]).max()
    bound = gradient_bound(voxels, whd, bbox, M)
    err = np.abs(got - want).max()
    print(f"{name}: max error {err:.3e}, bound {bound:.3e}, largest component {np.abs(want).max():.3e}")
    assert err <= bound and bound < 1e-3 * np.abs(want).max()
    # n = -g / |g| from the float32 gradient (five roundings under the root, the root, the quotient: 4 u of a unit vector); 0 for g = 0
    length = np.linalg.norm(got.astype(np.float64), axis=1)
    some = length > 0
    assert some.sum() > 1000 and np.all(normal[~some] == 0)
    assert np.abs(normal[some] + got[some] / length[some, None]).max() <= 4 * U


# ---- the closed forms of the statistical GPU test, against flights drawn from the reference distribution itself ------------------------
SLAB = {"tau": 1.0, "near": 2.0, "depth": 1.0}   # `constant` from its cameras: the box [0, 1]^3 of voxel value 1, trdepth 1, seen from z = 3
PIXELS, SAMPLES = 196, 512                       # what the GPU test flies: 14 x 14 interior pixels at 48 x 48, 512 samples each


def slab_scores(count, distance_sum, samples, tau, near, depth):
    """per pixel z of the collided fraction count / samples against 1 - exp(-tau) and of the mean collision distance distance_sum / count
    against its closed form (a truncated exponential behind `near`), each with the closed-form standard error: (z_opacity, z_depth)"""
    sigma, p, q = tau / depth, -np.expm1(-tau), np.exp(-tau)
    mean, var = near + 1 / sigma - depth * q / p, 1 / sigma ** 2 - depth ** 2 * q / p ** 2
    return (count / samples - p) / np.sqrt(p * q / samples), (distance_sum / count - mean) / np.sqrt(var / count)


def slab_passes(z):
    """every pixel within 5 standard errors and the mean z within 5 / sqrt(M), the form test_volgrid_gpu.py uses"""
    return bool(np.abs(z).max() <= 5 and abs(z.mean()) <= 5 / np.sqrt(z.size))


def test_the_closed_forms_pass_on_their_own_distribution_and_reject_a_medium_five_percent_denser():
    g, seed = np.random.default_rng(1), 1
    for scale, ok in ((1.0, True), (1.05, False)):
        t = -np.log1p(-g.uniform(size=(PIXELS, SAMPLES))) / (SLAB["tau"] * scale / SLAB["depth"])
        hit = t < SLAB["depth"]
        z_o, z_d = slab_scores(hit.sum(axis=1), np.where(hit, SLAB["near"] + t, 0).sum(axis=1), SAMPLES, **SLAB)
        print(f"seed {seed}, density x {scale}: opacity max |z| {np.abs(z_o).max():.2f}, mean {z_o.mean():+.3f}; depth max |z| "
              f"{np.abs(z_d).max():.2f}, mean {z_d.mean():+.3f}; limit on a mean {5 / np.sqrt(PIXELS):.3f}")
        if ok:   # with margin: 4 standard errors, not 5
            assert np.abs(z_o).max() <= 4 and np.abs(z_d).max() <= 4 and abs(z_o.mean()) <= 4 / np.sqrt(PIXELS) and abs(z_d.mean()) <= 4 / np.sqrt(PIXELS)
        else:    # the opacity alone rejects it: its mean z is expected at 0.84, the limit is 0.36, the mean's own standard error 0.071
            assert not slab_passes(z_o)
