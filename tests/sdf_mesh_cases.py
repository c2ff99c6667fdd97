"""What the two SDF-meshing test files share: the grids, a numpy replay of the rule of vpt_mesh_sdf (include/vpt.h) written from its text -
float32 operation by operation, vectorised over the cells - and the checks of a quad mesh's topology.  Every grid and every replay is
made once per process."""
import functools

import numpy as np

F = np.float32


def _points(whd, origin, step):
    """the sample points of a grid as three (d, h, w) float32 arrays: origin + (float)i * step"""
    w, h, d = whd
    ax = [F(origin[k]) + np.arange(n, dtype=F) * F(step[k]) for k, n in enumerate((w, h, d))]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return x, y, z


def _sphere(x, y, z, c, r):
    return (np.sqrt((x - F(c[0])) ** 2 + (y - F(c[1])) ** 2 + (z - F(c[2])) ** 2) - F(r)).astype(F)


def _torus(x, y, z, r1, r2):
    return (np.sqrt((np.sqrt(x * x + z * z) - F(r1)) ** 2 + y * y) - F(r2)).astype(F)


@functools.lru_cache(maxsize=None)
def case(name):
    """{voxels (d, h, w) float32, origin, step (3,) float32, iso, and for the closed cases: chi, distance(points), gradient(points)}"""
    f3 = lambda *v: np.array(v, F)
    if name == "sphere":   # 9 x 8 x 7, the surface interior
        whd, origin, step, c, r = (9, 8, 7), f3(-1.0, -0.9, -0.8), f3(0.25, 0.25, 0.25), (0.03, -0.04, -0.02), 0.55
        return dict(voxels=_sphere(*_points(whd, origin, step), c, r), origin=origin, step=step, iso=0.0, chi=2,
                    distance=lambda p: np.linalg.norm(p - np.array(c), axis=1) - r, gradient=lambda p: p - np.array(c))
    if name == "torus":    # 24^3, around the y axis
        whd, origin, step, r1, r2 = (24, 24, 24), f3(-1.5, -1.5, -1.5), f3(3 / 23, 3 / 23, 3 / 23), 0.8, 0.35
        ring = lambda p: np.hypot(p[:, 0], p[:, 2])

        def gradient(p):
            k = (ring(p) - r1) / ring(p)
            return np.stack([p[:, 0] * k, p[:, 1], p[:, 2] * k], 1)
        return dict(voxels=_torus(*_points(whd, origin, step), r1, r2), origin=origin, step=step, iso=0.0, chi=0,
                    distance=lambda p: np.hypot(ring(p) - r1, p[:, 1]) - r2, gradient=gradient)
    if name == "pair":     # two disjoint spheres on 20 x 12 x 12
        whd, origin, step = (20, 12, 12), f3(0, 0, 0), f3(0.1, 0.1, 0.1)
        a, b, r = (0.5, 0.55, 0.56), (1.4, 0.57, 0.53), 0.3
        x, y, z = _points(whd, origin, step)
        nearest = lambda p: np.where((np.linalg.norm(p - np.array(a), axis=1) < np.linalg.norm(p - np.array(b), axis=1))[:, None], np.array(a), np.array(b))
        return dict(voxels=np.minimum(_sphere(x, y, z, a, r), _sphere(x, y, z, b, r)), origin=origin, step=step, iso=0.0, chi=4,
                    distance=lambda p: np.linalg.norm(p - nearest(p), axis=1) - r, gradient=lambda p: p - nearest(p))
    if name == "clipped":  # a sphere that leaves the 8^3 grid on three sides
        whd, origin, step = (8, 8, 8), f3(0, 0, 0), f3(0.2, 0.2, 0.2)
        return dict(voxels=_sphere(*_points(whd, origin, step), (0.3, 0.4, 1.2), 0.62), origin=origin, step=step, iso=0.0)
    if name == "plane":    # a plane through voxel values that equal iso exactly
        x, y, z = _points((6, 7, 5), f3(0, 0, 0), f3(1, 1, 1))
        return dict(voxels=(y - F(3)).astype(F) + F(0) * x, origin=f3(-3, 0, 2), step=f3(0.5, 0.5, 0.5), iso=0.0)
    if name == "nonfinite":  # NaN and +-inf voxels beside the surface, and a difference that overflows
        v = case("sphere")["voxels"].copy()
        v[3, 4, 1], v[3, 3, 6], v[2, 2, 4], v[4, 5, 3] = np.nan, np.inf, -np.inf, np.nan
        v[3, 1, 3], v[3, 1, 4] = F(3e38), F(-3e38)
        v[1, 4, 4], v[5, 3, 4] = F(-0.0), F(0.0)
        return dict(voxels=v, origin=case("sphere")["origin"], step=case("sphere")["step"], iso=0.0)
    if name == "iso":      # the sphere's level set at 0.1
        return dict(case("sphere"), iso=0.1, chi=2, distance=lambda p: case("sphere")["distance"](p) - 0.1)
    if name == "anisotropic":
        whd, origin, step, c, r = (11, 9, 14), f3(-0.7, 0.1, 2.0), f3(0.15, 0.21, 0.11), (0.05, 0.9, 2.7), 0.5
        return dict(voxels=_sphere(*_points(whd, origin, step), c, r), origin=origin, step=step, iso=0.0, chi=2,
                    distance=lambda p: np.linalg.norm(p - np.array(c), axis=1) - r, gradient=lambda p: p - np.array(c))
    raise KeyError(name)


CASES = ("sphere", "torus", "pair", "clipped", "plane", "nonfinite", "iso", "anisotropic")
CLOSED = ("sphere", "torus", "pair", "iso", "anisotropic")   # the surface is interior: a closed mesh


def replay(voxels, origin, step, iso, region=None):
    """the rule, from its text.  Returns positions, normals (n, 3) float32, quads (m, 4) int32, cells (n, 3) int: the cell (x, y, z) of
    every vertex in the meshed grid, guarded: how many crossing parameters fell outside [0, 1] and became 0.5"""
    origin, step, iso = np.asarray(origin, F), np.asarray(step, F), F(iso)
    lo = (0, 0, 0) if region is None else tuple(region[0])
    size = voxels.shape[::-1] if region is None else tuple(region[1])
    v = np.ascontiguousarray(voxels[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]], F)
    D, H, W = v.shape
    empty = dict(positions=np.zeros((0, 3), F), normals=np.zeros((0, 3), F), quads=np.zeros((0, 4), np.int32), cells=np.zeros((0, 3), int), guarded=0)
    if min(D, H, W) < 2:
        return empty
    inside = v < iso   # a NaN voxel is outside
    corner = lambda a, k: a[(k >> 2):D - 1 + (k >> 2), ((k >> 1) & 1):H - 1 + ((k >> 1) & 1), (k & 1):W - 1 + (k & 1)]
    count = sum(corner(inside, k).astype(int) for k in range(8))
    cz, cy, cx = np.nonzero((count >= 1) & (count <= 7))   # index order: x fastest
    n = len(cx)
    ids = np.full((D, H, W), -1, np.int64)
    ids[cz, cy, cx] = np.arange(n)
    c = [corner(v, k)[cz, cy, cx] for k in range(8)]
    s = [np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)]
    crossings, guarded = np.zeros(n, int), 0
    with np.errstate(all="ignore"):
        for e in range(12):
            axis, p, q = e >> 2, e & 1, (e >> 1) & 1
            sa, sb, sc = 1 << axis, 1 << ((axis + 1) % 3), 1 << ((axis + 2) % 3)
            va, vb = c[p * sb + q * sc], c[p * sb + q * sc + sa]
            cross = (va < iso) != (vb < iso)
            t = (iso - va) / (vb - va)
            ok = (t >= 0) & (t <= 1)
            guarded += int((cross & ~ok).sum())
            t = np.where(ok, t, F(0.5)).astype(F)
            for k, term in ((axis, t), ((axis + 1) % 3, np.full(n, F(p))), ((axis + 2) % 3, np.full(n, F(q)))):
                s[k] = np.where(cross, s[k] + term, s[k]).astype(F)
            crossings += cross
        u = [(s[k] / crossings.astype(F)).astype(F) for k in range(3)]
        cell = (cx, cy, cz)
        positions = np.stack([origin[k] + ((cell[k] + lo[k]).astype(F) + u[k]) * step[k] for k in range(3)], 1).astype(F)
        one = F(1)
        ax, ay, az = one - u[0], one - u[1], one - u[2]
        gx = ((c[1] - c[0]) * ay + (c[3] - c[2]) * u[1]) * az + ((c[5] - c[4]) * ay + (c[7] - c[6]) * u[1]) * u[2]
        gy = ((c[2] - c[0]) * ax + (c[3] - c[1]) * u[0]) * az + ((c[6] - c[4]) * ax + (c[7] - c[5]) * u[0]) * u[2]
        gz = ((c[4] - c[0]) * ax + (c[5] - c[1]) * u[0]) * ay + ((c[6] - c[2]) * ax + (c[7] - c[3]) * u[0]) * u[1]
        nx, ny, nz = gx / step[0], gy / step[1], gz / step[2]
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        unit = [np.where(length != 0, g / length, g) for g in (nx, ny, nz)]
        normals = np.stack([np.where(np.isnan(g), F(0), g) for g in unit], 1).astype(F)
    # quads: by owner voxel, then by axis
    Z, Y, X = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    coord, dim = (X, Y, Z), (W, H, D)
    unit_step = lambda k: tuple(int(k == a) for a in range(3))
    keys, quads = [], []
    for a in range(3):
        b, cc = (a + 1) % 3, (a + 2) % 3
        nxt = np.roll(inside, -1, axis=2 - a)
        emit = (coord[a] + 1 < dim[a]) & (inside != nxt) & (coord[b] >= 1) & (coord[b] <= dim[b] - 2) & (coord[cc] >= 1) & (coord[cc] <= dim[cc] - 2)
        z, y, x = np.nonzero(emit)
        at = lambda off: ids[z - off[2], y - off[1], x - off[0]]
        eb, ec = unit_step(b), unit_step(cc)
        ebc = tuple(eb[k] + ec[k] for k in range(3))
        flip = nxt[z, y, x]
        first, second, third, fourth = at(ebc), at(ec), at((0, 0, 0)), at(eb)
        quads.append(np.stack([first, np.where(flip, fourth, second), third, np.where(flip, second, fourth)], 1))
        keys.append((x + y * W + z * W * H) * 3 + a)
    quads, keys = np.concatenate(quads), np.concatenate(keys)
    quads = quads[np.argsort(keys, kind="stable")].astype(np.int32)
    assert quads.size == 0 or quads.min() >= 0
    return dict(positions=positions, normals=normals, quads=quads, cells=np.stack([cx, cy, cz], 1), guarded=guarded)


@functools.lru_cache(maxsize=None)
def replayed(name):
    c = case(name)
    return replay(c["voxels"], c["origin"], c["step"], c["iso"])


def arrays(m):
    """(positions, normals, quads) of a mesh(...) dictionary, empty arrays for None"""
    get = lambda key, width, dtype: np.zeros((0, width), dtype) if m[key] is None else m[key]
    return get("positions", 3, F), get("normals", 3, F), get("quads", 4, np.int32)


def same_bytes(m, ref):
    """a mesh(...) dictionary against positions / normals / quads of `ref` (a dictionary of arrays, or another mesh), bit for bit"""
    ours, theirs = arrays(m), arrays(ref)
    return all(a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(ours, theirs))


def topology(positions, quads):
    """{closed: every undirected edge in exactly two quads and every directed edge once, used: every vertex in a quad, chi: V - E + F,
    volume: the signed volume (> 0: the quads face outward)}"""
    a, b = quads.reshape(-1), np.roll(quads, -1, axis=1).reshape(-1)
    directed = a.astype(np.int64) * (len(positions) + 1) + b
    undirected = np.minimum(a, b).astype(np.int64) * (len(positions) + 1) + np.maximum(a, b)
    _, per_edge = np.unique(undirected, return_counts=True)
    p = positions.astype(np.float64)
    tri = np.concatenate([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]])
    volume = float(np.einsum("ij,ij->i", p[tri[:, 0]], np.cross(p[tri[:, 1]], p[tri[:, 2]])).sum() / 6)
    return dict(closed=bool((per_edge == 2).all() and len(np.unique(directed)) == len(directed)), used=len(np.unique(quads)) == len(positions),
                chi=len(positions) - len(per_edge) + len(quads), volume=volume)
