"""The rule of vpt_scene_filter_volumes on the CPU (include/vpt.h, csrc/vpt_filter_rule.h): the host mirror of each op against a plain
float64 numpy restatement within a bound derived from the op's operation count, to_density against density_from_sdf, the Gaussian
weights, the struct sizes, and every refusal.  No GPU: the host mirror is compiled from the header the kernels compile."""
import ctypes as C

import numpy as np
import pytest

F = np.float32
U = 2.0 ** -24   # unit roundoff of float32
WHD = (9, 17, 30)
ORIGIN, STEP = (-0.7, 0.1, 0.02), (0.11, 0.07, 0.05)


def run(vpt, grid, ops, region=None, origin=ORIGIN, step=STEP, first=0, count=None):
    """vpth_filter_voxels on a copy of the (d, h, w) grid: (return code, message, the filtered copy)"""
    out = np.ascontiguousarray(grid, F).copy()
    whd = np.array(out.shape[::-1], np.int32)
    lo, size = ((0, 0, 0), tuple(whd)) if region is None else region
    abi, keep = vpt.FilterEdit([vpt.FilterEntry(0, lo, size, origin, step, list(ops))]).to_abi()
    entry = C.cast(abi.entries, C.POINTER(vpt.VptFilterEntry))
    entry[0].first_op, entry[0].num_ops = first, len(ops) if count is None else count
    err = C.create_string_buffer(256)
    rc = vpt.host.vpth_filter_voxels(out.ctypes.data, whd.ctypes.data, entry, abi.ops, abi.num_ops, err, len(err))
    return rc, err.value.decode(), out


@pytest.fixture(scope="module")
def grid():
    return np.random.default_rng(7).normal(0, 2, WHD[::-1]).astype(F)


def samples():
    """the float32 sample coordinate of every voxel per axis, operation by operation, as (d, h, w) float64 grids"""
    axes = [(F(ORIGIN[k]) + (np.arange(WHD[k]).astype(F) * F(STEP[k])).astype(F)).astype(F) for k in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return x, y, z


def test_remap_against_float64(vpt, grid):
    d, s, o, lo, hi = (float(F(v)) for v in (0.3, -1.7, 0.25, -2.0, 3.0))
    rc, _, got = run(vpt, grid, [vpt.FilterOp.remap(d, s, o, lo, hi)])
    x = grid.astype(np.float64) / d * s
    # the quotient, the product and the sum round once each: 3 u (1 + u)^2 |x| + u |o|; the clamps are 1-Lipschitz
    bound = (3 * np.abs(x) + abs(o)) * U * (1 + U) ** 2
    assert rc == 0 and (np.abs(got - np.clip(x + o, lo, hi)) <= bound).all() and (got != grid).any()


@pytest.mark.parametrize("radius", [1, 4])
def test_blur_against_float64(vpt, grid, radius):
    op = vpt.FilterOp.blur(0.9 * radius, radius)
    rc, _, got = run(vpt, grid, [op])
    w, ref = np.array(op.p, np.float64), grid.astype(np.float64)
    for axis in (2, 1, 0):   # x, then y, then z, clamped to the edge
        pad = np.pad(ref, [(radius, radius) if a == axis else (0, 0) for a in range(3)], mode="edge")
        n = ref.shape[axis]
        ref = sum(w[abs(i)] * np.take(pad, np.arange(n) + radius + i, axis=axis) for i in range(-radius, radius + 1))
    # one pass: a sum of R + 1 terms, each term at most R + 2 roundings deep (a + b, the product, the sums above it): (1 + g) S M per
    # pass with g = (R + 2) u / (1 - (R + 2) u), S = w0 + 2 sum wi and M the largest input - three passes
    g, S, M = (radius + 2) * U / (1 - (radius + 2) * U), w[0] + 2 * w[1:].sum(), np.abs(grid).max()
    assert rc == 0 and np.abs(got - ref).max() <= M * S ** 3 * ((1 + g) ** 3 - 1)
    assert np.abs(got - grid).max() > 0.1


def hash64(ix, iy, iz, seed):
    """csrc/vpt_filter_rule.h's hash in numpy integers: uint64 words masked to 32 bits"""
    m = np.uint64(0xffffffff)
    word = lambda a: np.asarray(a, np.int64).astype(np.uint64) & m
    h = ((word(ix) * np.uint64(0x8da6b343)) ^ (word(iy) * np.uint64(0xd8163841)) ^ (word(iz) * np.uint64(0xcb1ab31f)) ^ (word(seed) * np.uint64(0x9e3779b9))) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7feb352d)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846ca68b)) & m
    return h ^ (h >> np.uint64(16))


def vnoise64(x, y, z, seed):
    c = [np.floor(a) for a in (x, y, z)]
    i, j, k = (a.astype(np.int64) for a in c)
    u, v, w = ((f * f) * (3 - 2 * f) for f in (x - c[0], y - c[1], z - c[2]))
    lat = lambda a, b, cc: (hash64(i + a, j + b, k + cc, seed) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return (lat(0, 0, 0) * (1 - u) * (1 - v) * (1 - w) + lat(1, 0, 0) * u * (1 - v) * (1 - w) + lat(0, 1, 0) * (1 - u) * v * (1 - w) +
            lat(0, 0, 1) * (1 - u) * (1 - v) * w + lat(0, 1, 1) * (1 - u) * v * w + lat(1, 0, 1) * u * (1 - v) * w + lat(1, 1, 0) * u * v * (1 - w) +
            lat(1, 1, 1) * u * v * w)


def test_noise_against_float64(vpt, grid):
    gain, freq, pers, octaves, seed = float(F(0.8)), (3.0, 5.5, 7.25), float(F(0.6)), 5, 0xfffffffe   # seed + o wraps
    rc, _, got = run(vpt, grid, [vpt.FilterOp.noise(gain, freq, pers, octaves, seed)])
    # the lattice coordinates are the rule's own float32 products (a cell may not change sides); everything after them is float64
    q = [(s * F(f)).astype(F).astype(np.float64) for s, f in zip(samples(), freq)]
    total, a = 0.0, 1.0
    for o in range(octaves):
        total = total + a * vnoise64(*(c * 2.0 ** o for c in q), (seed + o) & 0xffffffff)
        a *= pers
    ref = grid.astype(np.float64) + gain * (total - 0.5)
    # vnoise: a weight is off by at most 4 u (3 roundings of the fade, 1 of 1 - fade), a term is a lattice value < 1 times three weights
    # <= 1 with three rounded products: 3 * 4 u + 3 u; eight terms and seven rounded sums of values <= 1: 8 * 15 u + 7 u = 127 u.  fbm: the
    # amplitude carries o roundings, the product and the sum one each.  Then fbm - 0.5, the product by gain and the sum with v round once each.
    A = sum(pers ** o for o in range(octaves))
    bound = (abs(gain) * (A * (127 + octaves + 2) * U + 2 * U * (A + 0.5)) + U * (np.abs(grid) + abs(gain) * (A + 0.5))) * (1 + 1e-3)
    assert rc == 0 and (np.abs(got - ref) <= bound).all()
    assert np.std(got - grid) > 0.05 and np.floor(q[0]).min() < 0 <= np.floor(q[0]).max()   # cells on both sides of 0


def test_to_density_equals_density_from_sdf_on_finite_voxels(vpt, grid):
    width = 0.37
    sdf = grid.copy()
    sdf.reshape(-1)[:4] = (0.0, -0.0, width, -width)
    rc, _, got = run(vpt, sdf, [vpt.FilterOp.to_density(width)])
    assert rc == 0 and np.array_equal(got, vpt.density_from_sdf(sdf, width)) and 0 < got.mean() < 1
    assert run(vpt, np.full((1, 1, 1), np.nan, F), [vpt.FilterOp.to_density(width)])[2][0, 0, 0] == 0   # a NaN voxel becomes lo


@pytest.mark.parametrize("radius,sigma", [(1, 0.5), (2, 1.0), (3, 1.7), (4, 2.0)])
def test_gaussian_weights(vpt, radius, sigma):
    w = np.array(vpt.FilterOp.blur(sigma, radius).p, F)
    g = np.exp(-np.arange(radius + 1, dtype=np.float64) ** 2 / (2 * float(F(sigma)) ** 2))
    assert np.array_equal(w, (g / (g[0] + 2 * g[1:].sum())).astype(F))
    assert abs(float(w[0]) + 2 * w[1:].astype(np.float64).sum() - 1) <= (radius + 1) * 2.0 ** -23


def test_struct_sizes_are_the_headers(vpt):
    assert (C.sizeof(vpt.VptFilterOp), C.sizeof(vpt.VptFilterEntry), C.sizeof(vpt.VptFilterEdit), vpt.FILTER_RECORD_BYTES) == (44, 60, 32, 48)
    assert (vpt.FILTER_REMAP, vpt.FILTER_BLUR, vpt.FILTER_NOISE, vpt.FILTER_MAX_RADIUS, vpt.FILTER_MAX_OCTAVES) == (0, 1, 2, 4, 8)


def _raw(vpt, type, count=0, p=()):
    return vpt.FilterOp(type, count=count, p=tuple(p))


REFUSALS = {   # name -> (keywords of run(), what the message names)
    "region": (lambda vpt: dict(ops=[vpt.FilterOp.to_density(1)], region=((5, 0, 0), (5, 1, 1))), "entry 0: the region leaves the grid"),
    "op_range": (lambda vpt: dict(ops=[vpt.FilterOp.to_density(1)], first=1), "entry 0: the op range leaves the edit's list"),
    "type": (lambda vpt: dict(ops=[vpt.FilterOp.to_density(1), _raw(vpt, 3)]), "op 1: type is not one of 0..2"),
    "float": (lambda vpt: dict(ops=[vpt.FilterOp.remap(1, np.inf, 0, 0, 1)]), "op 0: a value is not finite"),
    "weight": (lambda vpt: dict(ops=[_raw(vpt, 1, 2, (0.5, 0.25, np.nan))]), "op 0: a weight is not finite"),
    "step": (lambda vpt: dict(ops=[vpt.FilterOp.to_density(1)], step=(0.1, np.nan, 0.1)), "entry 0: origin or step is not finite"),
    "divisor": (lambda vpt: dict(ops=[vpt.FilterOp.remap(0, 1, 0, 0, 1)]), "op 0: divisor is 0"),
    "lo_hi": (lambda vpt: dict(ops=[vpt.FilterOp.remap(1, 1, 0, 1, 0)]), "op 0: lo is above hi"),
    "radius_0": (lambda vpt: dict(ops=[_raw(vpt, 1, 0, (1,))]), "op 0: the radius is not one of 1..4"),
    "radius_5": (lambda vpt: dict(ops=[_raw(vpt, 1, 5, (1,) * 6)]), "op 0: the radius is not one of 1..4"),
    "octaves_0": (lambda vpt: dict(ops=[vpt.FilterOp.noise(1, 1, octaves=0)]), "op 0: octaves is not one of 1..8"),
    "octaves_9": (lambda vpt: dict(ops=[vpt.FilterOp.noise(1, 1, octaves=9)]), "op 0: octaves is not one of 1..8"),
    "lattice": (lambda vpt: dict(ops=[vpt.FilterOp.noise(1, (1, 1, 2.0 ** 15), octaves=8)], origin=(0, 0, 0), step=(1, 1, 1)), "entry 0: a noise op's coordinates can reach 2^22"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_a_refusal_names_its_entry_or_op_and_writes_nothing(vpt, grid, name):
    make, named = REFUSALS[name]
    rc, message, got = run(vpt, grid, **make(vpt))
    assert rc == -1 and named in message and np.array_equal(got.view(np.uint32), grid.view(np.uint32))


def test_scene_refusals_and_the_three_ledgers(vpt):
    """the volume id, a region of more than 2^30 voxels (refused from the descriptor alone), and a volume pending in one ledger refused by the others"""
    from test_volgrid_host import load
    host = load(vpt, "messy")
    before = host.volume(0)[0].copy()
    with pytest.raises(vpt.VptError, match="entry 0: volume 2 out of range"):
        vpt._abi._host_call(vpt.host.vpth_scene_filter_volume, host.handle, C.byref(vpt.VptFilterEntry(volume=2)), None, 0)
    whd, entry, err = np.array([1024, 1024, 1025], np.int32), vpt.VptFilterEntry(num_ops=1), C.create_string_buffer(256)
    entry.region_whd[:] = list(whd)
    op = vpt.FilterOp.to_density(1).to_abi()
    assert vpt.host.vpth_filter_voxels(before.ctypes.data, whd.ctypes.data, C.byref(entry), C.byref(op), 1, err, 256) == -1 and b"2^30" in err.value
    host.filter_volume(0, [vpt.FilterOp.to_density(0.5)])
    for call in (lambda: host.sculpt_volume(0, []), lambda: host.set_volume(0, before)):
        with pytest.raises(vpt.VptError, match="filters pending"):
            call()
    with pytest.raises(vpt.VptError, match="update_filters"):
        host.remove_volumes([1])
    assert len(host.update_filters().entries) == 1 and not np.array_equal(host.volume(0)[0], before, equal_nan=True)
    host.set_volume(1, host.volume(1)[0])
    with pytest.raises(vpt.VptError, match="pending volume edit"):
        host.filter_volume(1, [vpt.FilterOp.to_density(0.5)])
