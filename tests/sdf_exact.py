"""An independent float64 reference for the signed-distance bake (include/vpt.h: vpt_bake_sdf), in plain numpy.  It shares nothing with
csrc/vpt_bake_rule.h: the distance is the plane distance where the projection falls inside the triangle and the nearest of the three
clamped segment distances elsewhere (no region scheme), the sign is the generalised winding number (no pseudonormals), and the
feature normals are summed by vertex index (no welding by position).  The sample points are the contract's own float32 points."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

F = np.float32
CHUNK = 1024   # points per block of the point x triangle arrays


def sample_points(whd, origin, step):
    """the points the kernel samples, origin + float32(i) * step rounded as float32 does, widened to float64: (d, h, w, 3) as [z, y, x]"""
    whd = np.broadcast_to(np.asarray(whd, np.int64), (3,))
    origin, step = np.broadcast_to(np.asarray(origin, F), (3,)), np.broadcast_to(np.asarray(step, F), (3,))
    axes = []
    for a in range(3):
        prod = (np.arange(whd[a]).astype(F) * step[a]).astype(F)
        axes.append((origin[a] + prod).astype(F).astype(np.float64))
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x, y, z], axis=-1)


def _corners(verts, tris):
    v = np.asarray(verts).astype(np.float64)
    t = np.asarray(tris)
    return v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]


def _dot(u, v):
    """the dot products along the last axis of (m, n, 3) against (m, n, 3) or (n, 3): (m, n)"""
    return np.einsum("mnk,mnk->mn" if np.ndim(v) == 3 else "mnk,nk->mn", u, v)


def _segment(r, e):
    """distance from the points to the segments t e, t in [0, 1]: r (m, n, 3) from a segment's start to a point, e (n, 3): (m, n)"""
    t = np.clip(_dot(r, e) / (e * e).sum(-1), 0.0, 1.0)
    q = r - t[..., None] * e
    return np.sqrt(_dot(q, q))


def _per_block(points, block):
    """block((m, 1, 3) points) -> (m,) over blocks of CHUNK points, four at a time (numpy drops the lock inside its loops)"""
    flat = np.asarray(points, np.float64).reshape(-1, 3)
    with ThreadPoolExecutor(4) as pool:
        parts = list(pool.map(lambda lo: block(flat[lo:lo + CHUNK, None, :]), range(0, len(flat), CHUNK)))
    return np.concatenate(parts).reshape(np.shape(points)[:-1])


def distance(points, verts, tris):
    """the unsigned distance from every point to the mesh: points' shape without its last axis.  Per triangle: the point's projection
    q onto the plane; inside when cross(edge, q - corner) . n >= 0 for the three edges - written as (q - corner) . cross(n, edge),
    the same triple product - and then the height over the plane; else the nearest of the three clamped segment distances."""
    a, b, c = _corners(verts, tris)
    n = np.cross(b - a, c - a)
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)

    def block(p):
        ra, rb, rc = p - a, p - b, p - c
        h = _dot(ra, n)                                  # signed height over the plane
        down = h[..., None] * n                          # p - q
        inside = (_dot(ra - down, np.cross(n, b - a)) >= 0) & (_dot(rb - down, np.cross(n, c - b)) >= 0) & (_dot(rc - down, np.cross(n, a - c)) >= 0)
        edges = np.minimum(np.minimum(_segment(ra, b - a), _segment(rb, c - b)), _segment(rc, a - c))
        return np.where(inside, np.abs(h), edges).min(axis=1)
    return _per_block(points, block)


def winding(points, verts, tris):
    """the generalised winding number: the signed solid angles of the triangles seen from the point (Van Oosterom & Strackee 1983),
    summed, over 4 pi.  Asserts that it is an integer to 1e-6 at every point: the mesh is closed and no point lies on it."""
    a, b, c = _corners(verts, tris)

    def block(p):
        u, v, w = a - p, b - p, c - p
        lu, lv, lw = np.sqrt(_dot(u, u)), np.sqrt(_dot(v, v)), np.sqrt(_dot(w, w))
        det = (u[..., 0] * (v[..., 1] * w[..., 2] - v[..., 2] * w[..., 1]) + u[..., 1] * (v[..., 2] * w[..., 0] - v[..., 0] * w[..., 2])
               + u[..., 2] * (v[..., 0] * w[..., 1] - v[..., 1] * w[..., 0]))
        den = lu * lv * lw + _dot(u, v) * lw + _dot(v, w) * lu + _dot(w, u) * lv
        return (2.0 * np.arctan2(det, den)).sum(axis=1) / (4.0 * np.pi)
    out = _per_block(points, block)
    off = np.abs(out - np.round(out)).max()
    assert off < 1e-6, f"winding number off an integer by {off:.3g}: the mesh is open or a point lies on it"
    return out


def signed_distance(points, verts, tris):
    """(exact signed distance, inside): negative where the winding number is above 0.5"""
    inside = winding(points, verts, tris) > 0.5
    return np.where(inside, -1.0, 1.0) * distance(points, verts, tris), inside


def feature_normals(verts, tris):
    """(n, 7, 3) as include/vpt.h states the table: the unit face normal; per edge ab, bc, ca the sum of the unit face normals of all
    triangles on it; per vertex a, b, c the sum of angle x unit face normal over the triangles around it.  Adjacency by vertex index."""
    v, t = np.asarray(verts).astype(np.float64), np.asarray(tris)
    p = v[t]                                                          # (n, 3 corners, 3)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    vertex, edge = np.zeros((len(v), 3)), {}
    for i, tri in enumerate(t):
        for k in range(3):
            e0, e1 = p[i, (k + 1) % 3] - p[i, k], p[i, (k + 2) % 3] - p[i, k]
            cosine = np.dot(e0, e1) / (np.linalg.norm(e0) * np.linalg.norm(e1))
            vertex[tri[k]] += np.arccos(np.clip(cosine, -1.0, 1.0)) * n[i]
            key = frozenset((int(tri[k]), int(tri[(k + 1) % 3])))
            edge[key] = edge.get(key, 0.0) + n[i]
    out = np.empty((len(t), 7, 3))
    out[:, 0] = n
    for i, tri in enumerate(t):
        for k in range(3):
            out[i, 1 + k] = edge[frozenset((int(tri[k]), int(tri[(k + 1) % 3])))]
            out[i, 4 + k] = vertex[tri[k]]
    return out
