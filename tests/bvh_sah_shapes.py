"""Synthetic point shapes for the SAH build's tests (tests/test_bvh_sah_host.py, tests/test_bvh_sah_gpu.py) and for the script that
pins them to the reference (tests/golden/make_bvh_sah_fixtures.py).  A shape is (positions float32 (n, 3), radius float32 (n,)): a
shape of n points, one per vertex; its element boxes are point_bounds(p, r) = {min(p - r, p + r), max(p - r, p + r)}."""
import numpy as np


def _random(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (n, 3)).astype(np.float32), rng.uniform(0.01, 0.1, n).astype(np.float32)


def _identical():
    return np.tile(np.float32([0.25, -0.5, 0.75]), (100, 1)), np.full(100, 0.125, np.float32)


def _collinear():   # centres on one line, many of them equal: ties between primitives and whole bins without a primitive
    x = np.float32([i // 3 for i in range(90)]) * np.float32(0.5)
    return np.stack([x, np.zeros(90, np.float32), np.zeros(90, np.float32)], 1), np.full(90, 0.25, np.float32)


def _lattice():     # a 4 x 4 x 2 lattice, every centre four times: candidates of different axes cost the same
    pts = np.float32([[x, y, z] for x in range(4) for y in range(4) for z in range(2)] * 4)
    return pts, np.full(len(pts), 0.5, np.float32)


def _huge():        # radii far above the spread of the centres: areas overflow, no candidate wins, halves
    i = np.arange(64, dtype=np.float32)
    return np.stack([(i - np.float32(20)) * np.float32(1e9), np.zeros(64, np.float32), np.zeros(64, np.float32)], 1), np.full(64, 1e14, np.float32)


def _clusters():    # two far clusters of 40 points
    rng = np.random.default_rng(7)
    p = rng.uniform(-1, 1, (80, 3)).astype(np.float32)
    p[40:, 0] += np.float32(1000)
    return p, np.full(80, 0.05, np.float32)


def _skewed():      # 1 000 points, positions skewed towards a corner, every 50th large
    rng = np.random.default_rng(11)
    p = (rng.uniform(0, 1, (1000, 3)) ** 4).astype(np.float32)
    r = np.full(1000, 0.002, np.float32)
    r[::50] = np.float32(0.2)
    return p, r


def tie(seed):
    """12 points on small integers with one radius: the candidate costs are ratios of small integers, and equal ones are common"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 4, (12, 3)).astype(np.float32), np.full(12, 0.5, np.float32)


SHAPES = {
    "random_5": lambda: _random(5, 1), "random_65": lambda: _random(65, 2), "random_257": lambda: _random(257, 3),
    "identical_100": _identical, "collinear_ties": _collinear, "lattice_repeated": _lattice, "huge_radius_64": _huge, "two_clusters": _clusters,
    "skewed_1000": _skewed,
}


def boxes(positions, radius):
    """point_bounds of every point, float32: (n, 6)"""
    r = radius[:, None]
    lo, hi = positions - r, positions + r
    return np.concatenate([np.minimum(lo, hi), np.maximum(lo, hi)], 1).astype(np.float32)


def fnv1a(data: bytes) -> str:
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return f"{h:016x}"


def root_costs(bx):
    """The 45 candidate costs of the root over boxes bx, float32 operation by operation in the rule's order: [(saxis, b, cost, left set)]"""
    f = np.float32
    ctr = ((bx[:, :3] + bx[:, 3:]) / f(2)).astype(np.float32)
    cmin, cmax = ctr.min(0), ctr.max(0)
    csize = (cmax - cmin).astype(np.float32)

    def area(s):
        return f(f(f(f(1e-12) + f(f(2) * s[0]) * s[1]) + f(f(2) * s[0]) * s[2]) + f(f(2) * s[1]) * s[2])

    out = []
    with np.errstate(all="ignore"):
        for a in range(3):
            for b in range(1, 16):
                bsplit = f(cmin[a] + f(f(b) * csize[a]) / f(16))
                left = ctr[:, a] < bsplit
                sides = []
                for m in (left, ~left):
                    lo = bx[m, :3].min(0) if m.any() else np.full(3, np.finfo(f).max, f)
                    hi = bx[m, 3:].max(0) if m.any() else np.full(3, -np.finfo(f).max, f)
                    sides.append(f(f(int(m.sum())) * area((hi - lo).astype(f))) / area(csize))
                out.append((a, b, f(f(f(1) + sides[0]) + sides[1]), tuple(np.flatnonzero(left))))
    return out


def uneven_scene(dirpath, n=60000, seed=13):
    """A scene file of one shape of n triangles as uneven as skewed_1000 - centres skewed towards a corner of the unit cube, every 50th
    triangle large - over a floor, under a sky: the kind of shape on which the two builds differ most.  Returns the scene's path."""
    import synth_scenes
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, 1, (n, 3)) ** 4
    size = np.full((n, 1, 1), 0.004)
    size[::50] = 0.25
    verts = (c[:, None, :] + size * rng.normal(size=(n, 3, 3))).reshape(-1, 3)
    w = synth_scenes._Writer(str(dirpath))
    shape = w.shape("uneven", verts, np.arange(3 * n).reshape(n, 3))
    floor = w.shape("floor", [[-4, -0.6, -4], [4, -0.6, -4], [4, -0.6, 4], [-4, -0.6, 4]], [[0, 1, 2], [0, 2, 3]])
    identity = np.concatenate([np.eye(3).reshape(-1), [0, 0, 0]])
    w.instance(floor, identity, 0), w.instance(shape, identity, 1)
    return w.write("uneven", synth_scenes._look_at([2.2, 1.6, 2.6], [0.3, 0.3, 0.3]), env=1.0)[0]
