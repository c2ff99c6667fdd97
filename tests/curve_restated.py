"""intersect_point and intersect_line (yocto_geometry.h:683-746) restated in float32 numpy, in the reference's operation order: dot as
x x + y y + z z from left to right, every intermediate a float32 (numpy rounds each operation and fuses nothing).  The ray goes into
shape space as intersect_bvh does it, transform_ray(inverse(frame, non_rigid = true), ray) (yocto_math.h:2802-2808, 2948-2956,
3097-3102).  A brute force over all elements: the nearest accepted t wins, the last element wins among equals (tmax shrinks to the last
accepted t, and t > tmax rejects).  `mutation` plants one defect, for the tests that show the certificate (tests/curve_exact.py)
rejects it."""
import numpy as np

F = np.float32
TMIN = F(1e-4)
MUTATIONS = ("r0_only", "s_unclamped", "t_recomputed", "u_flipped", "bare_box", "point_before_tmin", "d2_against_r")


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def shape_space(frame, rays):
    """(o, d) float32 (n, 3): transform_point / transform_vector by inverse(frame, true); frame (12,) float32 x, y, z, o"""
    x, y, z, f = np.asarray(frame, F).reshape(4, 3)
    inv = np.stack([_cross(y, z), _cross(z, x), _cross(x, y)]).T * (F(1) / _dot(x, _cross(y, z)))   # columns of adjoint * (1 / det)
    ix, iy, iz = inv[0], inv[1], inv[2]
    io = -(ix * f[0] + iy * f[1] + iz * f[2])
    o, d = rays[:, :3].astype(F), rays[:, 3:].astype(F)
    return (ix * o[:, 0:1] + iy * o[:, 1:2] + iz * o[:, 2:3] + io).astype(F), (ix * d[:, 0:1] + iy * d[:, 1:2] + iz * d[:, 2:3]).astype(F)


def intersect(points, o, d, p0, p1, r0, r1, mutation=None):
    """one element per row of the broadcast of o, d (.., 3) against p0, p1 (.., 3), r0, r1 (..): (hit, u, v, t) float32"""
    with np.errstate(all="ignore"):
        if points:
            w = p0 - o
            t = _dot(w, d) / _dot(d, d)
            ok = np.ones(t.shape, bool) if mutation == "point_before_tmin" else ~(t < TMIN)
            prp = p0 - (o + d * t[..., None])
            ok &= ~(_dot(prp, prp) > r0 * r0)
            zero = np.zeros(t.shape, F)
            return ok, zero, zero, t
        v, w = p1 - p0, o - p0
        a, b, c, dd, e = _dot(d, d), _dot(d, v), _dot(v, v), _dot(d, w), _dot(v, w)
        det = a * c - b * b
        ok = ~(det == 0)
        t, s = (b * e - c * dd) / det, (a * e - b * dd) / det
        ok &= ~(t < TMIN)
        if mutation != "s_unclamped":
            s = np.clip(s, F(0), F(1))
        pl = p0 + (p1 - p0) * s[..., None]
        if mutation == "t_recomputed":
            t = _dot(pl - o, d) / a
        pr = o + d * t[..., None]
        prl = pr - pl
        d2 = _dot(prl, prl)
        r = r0 * (F(1) - s) + r1 * s
        if mutation == "r0_only":
            r = r0 + F(0) * s
        ok &= ~(d2 > (r if mutation == "d2_against_r" else r * r))
        if mutation == "bare_box":   # a leaf box of the two vertices without their radii: the ray's point must lie inside it
            ok &= ((pr >= np.minimum(p0, p1)) & (pr <= np.maximum(p0, p1))).all(-1)
        return ok, (F(1) - s if mutation == "u_flipped" else s), np.sqrt(d2) / r, t


def _f32(el):
    return el.p0.astype(F), el.p1.astype(F), el.r0.astype(F), el.r1.astype(F)


def _frame(el):
    return np.concatenate([el.M.T.reshape(9), el.f]).astype(F)


def on_elements(el, rays, element, mutation=None):
    """(hit, uvt (n, 3)) of ray i against element[i] of the instance"""
    o, d = shape_space(_frame(el), rays)
    p0, p1, r0, r1 = (a[element] for a in _f32(el))
    ok, u, v, t = intersect(el.points, o, d, p0, p1, r0, r1, mutation)
    return ok, np.stack([u, v, t], -1)


def brute_force(elements, rays, mutation=None, chunk=128):
    """intersect_bvh's answer without a BVH over a list of curve_exact.Elements: ids (n, 2) int32 ({-1, -1}: a miss), uvt (n, 3) float32"""
    n = len(rays)
    ids, uvt = np.full((n, 2), -1, np.int32), np.zeros((n, 3), F)
    for lo in range(0, n, chunk):
        sl = slice(lo, min(n, lo + chunk))
        best = np.full(sl.stop - lo, np.inf, F)
        for el in elements:
            o, d = shape_space(_frame(el), rays[sl])
            p0, p1, r0, r1 = (a[None] for a in _f32(el))
            ok, u, v, t = intersect(el.points, o[:, None], d[:, None], p0, p1, r0, r1, mutation)
            t = np.where(ok, t, np.inf).astype(F)
            m = len(el) - 1 - np.argmin(t[:, ::-1], 1)          # the last of the nearest
            rows = np.arange(len(m))
            take = t[rows, m] <= best                            # a later instance wins a tie too
            take &= np.isfinite(t[rows, m])
            best = np.where(take, t[rows, m], best)
            at = np.nonzero(take)[0]
            ids[lo + at, 0], ids[lo + at, 1] = el.instance, m[at]
            uvt[lo + at] = np.stack([np.broadcast_to(u, t.shape)[at, m[at]], np.broadcast_to(v, t.shape)[at, m[at]], t[at, m[at]]], -1)
    return ids, uvt
