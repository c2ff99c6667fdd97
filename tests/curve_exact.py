"""An independent float64 reference for rays against shapes of points and lines, with a forward error bound of the float32 evaluation
beside every value, and a certificate that holds an answer {instance, element, u, v, t} per ray to both.  Plain numpy; it shares nothing
with csrc/vpt_scene.hip.h.  Its inputs are what the scene holds as float32 (HostScene.shape_arrays, instance_frame, material, camera),
widened to float64.

The operation is intersect_point and intersect_line of yocto_geometry.h:683-746, formula for formula.  The ray {o, d} goes into shape
space by the full inverse of the instance frame (the reference inverts with non_rigid = true), t stays the ray parameter.
  point  w = p - o, t = w.d / d.d; miss when t < tmin; q = p - (o + d t), d2 = q.q; miss when d2 > r r; uv = {0, 0}
  line   v = p1 - p0, w = o - p0, a = d.d, b = d.v, c = v.v, dd = d.w, e = v.w, det = a c - b b; det == 0 misses;
         t = (b e - c dd) / det, s = (a e - b dd) / det; miss when t < tmin; s = clamp(s, 0, 1), t NOT recomputed;
         q = (o + d t) - (p0 + v s), d2 = q.q, r = r0 (1 - s) + r1 s; miss when d2 > r r; uv = {s, sqrt(d2) / r}

The error bounds.  eps = 2^-24 is the unit roundoff of float32: fl(x op y) = (x op y)(1 + h), |h| <= eps, so every rounding adds eps
times the magnitude of what is rounded.  Second-order terms (eps^2) are covered by taking K = 4 where the count below gives 3 or less.
Norms are Euclidean; |x| of a vector is its length.  For every quantity x, e_x bounds |float32 value - float64 value|.
  the frame  The reference builds the inverse as adjoint(M) (1 / det M), rows cross(y, z), cross(z, x), cross(x, y) of the columns x, y, z.
       A cross product of u, v is off by at most 4 eps |u||v| (two products and a difference per component, Cauchy-Schwarz over the
       components), det M = x . cross(y, z) by (4 + 3) eps |x||y||z|.  With h = |x||y||z| / |det M| (1 for orthogonal columns) the
       reciprocal 1 / det is off by (7 h + 1) eps relatively, so with G = sqrt(sum over the three pairs of (|u||v|)^2) / |det M|, which
       is at least the Frobenius norm of the inverse, the float32 inverse N~ is within (4 + 1 + 7 h + 1) eps G <= (8 h + 8) eps G of the
       exact N.  Its origin is -(N~ f) rounded, f the frame's origin, and the point transform adds it after N~ o; N~ o - N~ f is
       N~ (o - f) exactly, so what is left are the roundings of the two matrix-vector products and the sum, each at most 4 eps G times
       the length of its operand, |o| or |f|:
         e_o = (8 h + 8) eps G |o - f| + 4 eps G (|o| + |f|)      e_d = (8 h + 12) eps G |d|
       Both are 0 under the identity frame: x 1 + y 0 + z 0 + (-0) is exact.  Below o, d are the exact shape-space ray.
  The roundings of the function itself and what the ray carries in are bounded apart: |f~(o~, d~) - f(o, d)| <= |f~(o~, d~) - f(o~, d~)|
  + |f(o~, d~) - f(o, d)|, the first by counting roundings, the second by the exact function's sensitivity to its inputs.
  sums       v = p1 - p0 and w = o - p0 are single roundings of exact float32 differences: e_v = eps |v|, e_w = eps |w|
  dots       a dot product of three terms is off by at most 3 eps |x||y| (gamma_3, Cauchy-Schwarz), K = 4, plus what its operands carry:
         e_a = 4 eps a      e_b = 4 eps |d||v| + |d| e_v      e_c = 4 eps c + 2 |v| e_v
         e_dd = 4 eps |d||w| + |d| e_w      e_e = 4 eps |v||w| + |w| e_v + |v| e_w
  det        two products and a difference, each rounding at most eps (a c + b b): e_det0 = 4 eps (a c + b b) + c e_a + a e_c + 2 |b| e_b.
         As a function of d, det = |d|^2 |v|^2 sin^2 of the angle between ray and segment, and its gradient is 2 (c d - b v), of length
         2 c |d| sin: e_det = e_det0 + 2 (2 c |d| sin e_d + c e_d^2), the first-order term and the exact second-order one, doubled
  t, s       the numerators likewise: e_nt = 4 eps (|b e| + |c dd|) + |e| e_b + |b| e_e + |dd| e_c + c e_dd, and
         e_ns = 4 eps (|a e| + |b dd|) + |e| e_a + a e_e + |dd| e_b + |b| e_dd.  A quotient n / det: |n~/det~ - n/det| <=
         (e_n + |n/det| e_det0) / (|det| - e_det0), and the division rounds once.  t and s are the parameters of the closest approach of
         two lines: moving the ray's origin by x moves t by at most |x| / (|d| sin) and s by at most |x| / (|v| sin); turning d by y
         moves the ray's point at t by |t||y|, which acts as such a shift, and rescales t by at most |y| / |d|.  These first-order
         sensitivities are doubled for the higher orders (|det| > 2 e_det keeps sin from halving under e_d):
         e_t = (e_nt + |t| e_det0) / (|det| - e_det0) + 4 eps |t| + 2 (e_o + 2 |t| e_d) / (|d| sin)
         e_s = (e_ns + |s| e_det0) / (|det| - e_det0) + 4 eps |s| + 2 (e_o + |t| e_d) / (|v| sin)
       After the clamp e_s is 0 where s lies outside [-e_s, 1 + e_s]: the float32 s is then outside [0, 1] too and clamps to the same end.
  points     w = p - o carries e_w = e_o + eps |w|; e_n = 4 eps |w||d| + |d| e_w + |w| e_d, e_a = 4 eps a + 2 |d| e_d,
         e_t = (e_n + |t| e_a) / (a - e_a) + 4 eps |t|
  the gap    q = (o + d t) - (p0 + v s): products, sums and the difference round at most 4 eps (|o| + |d||t| + |p0| + |v|) together, and
       the operands carry e_o + |t| e_d + |d| e_t on the ray and e_v + |v| e_s on the segment:
         e_q = 4 eps (|o| + |d||t| + |p0| + |v|) + e_o + |t| e_d + |d| e_t + e_v + |v| e_s       (a point: p for p0, no v)
         e_d2 = 2 sqrt(d2) e_q + e_q^2 + 4 eps d2                  (|q~|^2 - |q|^2 = (|q~| - |q|)(|q~| + |q|), then gamma_3 of the dot)
  radius     r = r0 (1 - s) + r1 s: e_r = 4 eps (|r0| + |r1|) + |r1 - r0| e_s, and r r: e_r2 = 2 r e_r + e_r^2 + 4 eps r r
  v          sqrt(d2) is off by e_q (the triangle inequality on q) + 4 eps sqrt(d2) (the dot's gamma_3 halves under the root, the root
       rounds once); the quotient by r as above: e_v = 2 (e_q + 4 eps sqrt(d2) + v e_r) / r + 4 eps v, infinite where r <= 2 e_r
Underflow adds absolute errors near 1e-45, far below every term here at the scales of the tests; tmax is flt_max and never rejects.

A (ray, element) pair is DECIDED where the float32 comparisons cannot come out differently: |det| > 2 e_det; |t - tmin| > e_t;
|d2 - r r| > e_d2 + e_r2.  All three decided and a hit in float64: a decided hit.  A decided miss: det decided and one of the two
rejecting comparisons decided as rejecting (whichever way the other goes, the element rejects), or p0 == p1 bit for bit (v is exactly 0
in float32, so det is).  Everything else is undecided.  `certify` states what an answer must satisfy."""
import numpy as np

EPS = 2.0 ** -24
TMIN = 1e-4            # ray3f's default, yocto_geometry.h:118-123; as the float32 it is compared with
TMIN32 = float(np.float32(TMIN))
UNDECIDED, HIT, MISS = 0, 1, 2


def _len(x):
    return np.sqrt((x * x).sum(-1))


def _dot(x, y):
    return (x * y).sum(-1)


class Elements:
    """the points or lines of one instance, float64: p0, p1 (m, 3), r0, r1 (m,) (a point: p1 = p0, r1 = r0), the instance's frame as
    (M (3, 3) with columns x, y, z, origin f), the vertex ids (m, 2)"""

    def __init__(self, instance, shape, points, arrays, frame):
        self.instance, self.shape, self.points = instance, shape, points
        ids = arrays["points"].reshape(-1, 1).repeat(2, 1) if points else arrays["lines"]
        pos, rad = arrays["positions"].astype(np.float64), arrays["radius"].astype(np.float64)
        self.ids, self.p0, self.p1, self.r0, self.r1 = ids, pos[ids[:, 0]], pos[ids[:, 1]], rad[ids[:, 0]], rad[ids[:, 1]]
        self.degenerate = np.zeros(len(ids), bool) if points else (arrays["positions"][ids[:, 0]] == arrays["positions"][ids[:, 1]]).all(-1)
        frame = np.asarray(frame, np.float32).astype(np.float64).reshape(4, 3)
        self.M, self.f = frame[:3].T.copy(), frame[3].copy()
        self.identity = bool((frame == np.eye(4, 3)).all())
        self.arrays = {k: a.astype(np.float64) for k, a in arrays.items() if k in ("normals", "texcoords", "colors", "positions")}

    def __len__(self):
        return len(self.ids)


def instance_elements(scene, instance):
    """the Elements of a scene's instance, None where its shape holds faces"""
    shape, _ = scene.instance_ids(instance)
    arrays = scene.shape_arrays(shape)
    if not len(arrays["points"]) and not len(arrays["lines"]):
        return None
    return Elements(instance, shape, len(arrays["points"]) > 0, arrays, scene.instance_frame(instance))


def curve_instances(scene, instances=None):
    every = range(scene.count("instances")) if instances is None else instances
    return [e for e in (instance_elements(scene, i) for i in every) if e is not None]


def shape_space(el, rays):
    """the rays {o, d} (n, 6) float32 in the instance's shape space, exact in float64, and the bounds of the float32 transform:
    o, d (n, 3), e_o, e_d (n,)"""
    o, d = rays[:, :3].astype(np.float64), rays[:, 3:].astype(np.float64)
    if el.identity:
        return o, d, np.zeros(len(o)), np.zeros(len(o))
    N = np.linalg.inv(el.M)
    x, y, z = _len(el.M[:, 0]), _len(el.M[:, 1]), _len(el.M[:, 2])
    det = abs(np.linalg.det(el.M))
    h, G = x * y * z / det, np.sqrt((y * z) ** 2 + (z * x) ** 2 + (x * y) ** 2) / det
    e_o = (8 * h + 8) * EPS * G * _len(o - el.f) + 4 * EPS * G * (_len(o) + _len(el.f))
    return (o - el.f) @ N.T, d @ N.T, e_o, (8 * h + 12) * EPS * G * _len(d)


def pairs(el, rays):
    """every (ray, element) pair of one instance: a dict of (n, m) arrays - t, u, v (u the clamped s; 0, 0 for points), e_t, e_u, e_v,
    state (UNDECIDED / HIT / MISS), s (unclamped), r (at the closest approach), near (d2 <= (1.3 r)^2: the ray passes within 1.3 r),
    tmin_only (a decided miss ahead of the origin that only the tmin comparison rejects: 0 < t < tmin and d2 <= r r, both decided)"""
    o, d, e_o, e_d = (a[:, None] for a in shape_space(el, rays))
    p0, r0, r1 = el.p0[None], el.r0[None], el.r1[None]
    O, D, P0 = _len(o), _len(d), _len(p0)
    a = _dot(d, d)
    with np.errstate(all="ignore"):
        if el.points:
            w = p0 - o
            W, e_w, e_a = _len(w), e_o + EPS * _len(w), 4 * EPS * D * D + 2 * D * e_d
            num, e_n = _dot(w, d), 4 * EPS * W * D + D * e_w + W * e_d
            t = num / a
            e_t = (e_n + np.abs(t) * e_a) / (a - e_a) + 4 * EPS * np.abs(t)
            det_ok = np.ones(t.shape, bool)
            s = u = e_u = np.zeros(t.shape)
            q = p0 - (o + d * t[..., None])
            e_q = 4 * EPS * (O + D * np.abs(t) + P0) + e_o + np.abs(t) * e_d + D * e_t
            r, e_r = np.broadcast_to(r0, t.shape), 0.0
        else:
            v, w = el.p1[None] - p0, o - p0
            V, W = _len(v), _len(w)
            e_v, e_w = EPS * V, EPS * W
            b, c, dd, e = _dot(d, v), _dot(v, v), _dot(d, w), _dot(v, w)
            e_a, e_b, e_c = 4 * EPS * a, 4 * EPS * D * V + D * e_v, 4 * EPS * c + 2 * V * e_v
            e_dd, e_e = 4 * EPS * D * W + D * e_w, 4 * EPS * V * W + W * e_v + V * e_w
            det = a * c - b * b
            sin = np.sqrt(np.maximum(det, 0) / (a * c))
            e_det0 = 4 * EPS * (a * c + b * b) + c * e_a + a * e_c + 2 * np.abs(b) * e_b
            e_det = e_det0 + 2 * (2 * c * D * sin * e_d + c * e_d * e_d)
            det_ok = np.abs(det) > 2 * e_det
            e_nt = 4 * EPS * (np.abs(b * e) + np.abs(c * dd)) + np.abs(e) * e_b + np.abs(b) * e_e + np.abs(dd) * e_c + c * e_dd
            e_ns = 4 * EPS * (np.abs(a * e) + np.abs(b * dd)) + np.abs(e) * e_a + a * e_e + np.abs(dd) * e_b + np.abs(b) * e_dd
            t, s = (b * e - c * dd) / det, (a * e - b * dd) / det
            e_t = (e_nt + np.abs(t) * e_det0) / (np.abs(det) - e_det0) + 4 * EPS * np.abs(t) + 2 * (e_o + 2 * np.abs(t) * e_d) / (D * sin)
            e_s = (e_ns + np.abs(s) * e_det0) / (np.abs(det) - e_det0) + 4 * EPS * np.abs(s) + 2 * (e_o + np.abs(t) * e_d) / (V * sin)
            e_u = np.where((s < -e_s) | (s > 1 + e_s), 0.0, e_s)
            u = np.clip(s, 0.0, 1.0)
            q = (o + d * t[..., None]) - (p0 + v * u[..., None])
            e_q = 4 * EPS * (O + D * np.abs(t) + P0 + V) + e_o + np.abs(t) * e_d + D * e_t + e_v + V * e_u
            r = r0 * (1 - u) + r1 * u
            e_r = 4 * EPS * (np.abs(r0) + np.abs(r1)) + np.abs(r1 - r0) * e_u
        d2 = _dot(q, q)
        dist = np.sqrt(d2)
        e_d2 = 2 * dist * e_q + e_q * e_q + 4 * EPS * d2
        e_r2 = 2 * r * e_r + e_r * e_r + 4 * EPS * r * r
        vv = np.zeros(t.shape) if el.points else dist / r
        e_vv = np.zeros(t.shape) if el.points else np.where(r > 2 * e_r, 2 * (e_q + 4 * EPS * dist + vv * e_r) / r + 4 * EPS * vv, np.inf)
        finite = det_ok & np.isfinite(t) & np.isfinite(e_t) & np.isfinite(d2) & np.isfinite(e_d2)
        t_ok, t_rej = finite & (np.abs(t - TMIN32) > e_t), t < TMIN32
        d_ok, d_rej = finite & (np.abs(d2 - r * r) > e_d2 + e_r2), d2 > r * r
    state = np.full(t.shape, UNDECIDED, np.int8)
    state[t_ok & d_ok & ~t_rej & ~d_rej] = HIT
    state[(t_ok & t_rej) | (d_ok & d_rej) | np.broadcast_to(el.degenerate[None], t.shape)] = MISS
    return {"t": t, "u": u, "v": vv, "e_t": e_t, "e_u": e_u, "e_v": e_vv, "state": state, "s": s, "r": r,
            "near": finite & (d2 <= (1.3 * r) ** 2), "tmin_only": t_ok & t_rej & d_ok & ~d_rej & (t > 0)}


class Verdict:
    """what certify found: violations, a list of (ray, text); undecided (n,) bool, the rays whose verdict rested on an undecided pair"""

    def __init__(self, n):
        self.violations, self.undecided = [], np.zeros(n, bool)

    @property
    def share(self):
        return float(self.undecided.mean())


class Reference:
    """the pairs of a ray set (n, 6) float32 against a list of Elements, in blocks of `chunk` rays; keep: hold what certify reads of
    every block, for ray sets that are certified many times (about 60 bytes per pair)"""
    KEYS = ("t", "u", "v", "e_t", "e_u", "e_v", "state", "r")

    def __init__(self, elements, rays, chunk=256, keep=False):
        self.elements, self.rays, self.chunk, self.kept = list(elements), np.ascontiguousarray(rays, np.float32), chunk, {} if keep else None

    def block(self, k, lo):
        if self.kept is None:
            return pairs(self.elements[k], self.rays[lo:lo + self.chunk])
        if (k, lo) not in self.kept:
            p = pairs(self.elements[k], self.rays[lo:lo + self.chunk])
            self.kept[k, lo] = {key: p[key] for key in self.KEYS}
        return self.kept[k, lo]


def certify(ref, ids, uvt, instances=None, face_instances=()):
    """Holds an answer per ray of ref.rays, ids (n, 2) {instance, element} ({-1, -1}: a miss) and uvt (n, 3) {u, v, t}, from anywhere,
    to the reference over the Elements the query covered: all of ref.elements, or those of `instances`.
      a hit on element k   k is not a decided miss; |t - t_k| <= e_t, |u - u_k| <= e_u, |v - v_k| <= e_v (a NaN v passes where r is 0);
                           no decided hit j has t_j + e_t_j < t_k - e_t_k
      a miss               no element is a decided hit
    Two elements with equal or overlapping t are both acceptable (the reference's own order dependence).  A hit on an instance of
    `face_instances` is not this reference's to judge; only a decided hit nearer than the reported t by more than 64 eps t (a generous
    bound of a triangle test's own distance error) counts against it.  A hit on any other instance is a violation.
    The verdict of a ray rests on an undecided pair where the reported element was undecided, an undecided element could have been
    nearer (its t + e_t lies below the reported interval, or its t is unknown), or a miss was reported while one existed."""
    n, out = len(ref.rays), Verdict(len(ref.rays))
    which = [k for k, el in enumerate(ref.elements) if instances is None or el.instance in instances]
    elements = [ref.elements[k] for k in which]
    by_instance = {el.instance: k for k, el in enumerate(elements)}
    ids, uvt = np.asarray(ids), np.asarray(uvt, np.float64)
    for lo in range(0, n, ref.chunk):
        hi = min(n, lo + ref.chunk)
        P = [ref.block(k, lo) for k in which]
        cat = {k: np.concatenate([p[k] for p in P], 1) for k in ("t", "e_t", "state")}
        first = np.cumsum([0] + [len(el) for el in elements])
        with np.errstate(invalid="ignore"):
            upper = np.where(np.isfinite(cat["t"] + cat["e_t"]), cat["t"] + cat["e_t"], -np.inf)   # an unknown t could be anywhere
        nearest_decided = np.where(cat["state"] == HIT, upper, np.inf).min(1)
        for i in range(lo, hi):
            row = i - lo
            inst, k = int(ids[i, 0]), int(ids[i, 1])
            und = cat["state"][row] == UNDECIDED
            if inst < 0:
                if nearest_decided[row] < np.inf:
                    j = int(np.argmin(np.where(cat["state"][row] == HIT, upper[row], np.inf)))
                    out.violations.append((i, f"a miss, but pair {j} is a decided hit at t = {cat['t'][row, j]:.9g}"))
                out.undecided[i] = und.any()
                continue
            if inst not in by_instance:
                t = uvt[i, 2]
                if inst not in face_instances:
                    out.violations.append((i, f"a hit on instance {inst}, which the query did not cover"))
                elif nearest_decided[row] < t - 64 * EPS * abs(t):
                    out.violations.append((i, f"a face at t = {t:.9g}, but a decided hit ends at {nearest_decided[row]:.9g}"))
                out.undecided[i] = (und & (upper[row] < t)).any()
                continue
            e, p = by_instance[inst], P[by_instance[inst]]
            if not 0 <= k < len(elements[e]):
                out.violations.append((i, f"element {k} out of range on instance {inst}"))
                continue
            g = first[e] + k
            if p["state"][row, k] == MISS:
                out.violations.append((i, f"a hit on ({inst}, {k}), a decided miss"))
                continue
            for name, got, key in (("t", uvt[i, 2], "t"), ("u", uvt[i, 0], "u"), ("v", uvt[i, 1], "v")):
                want, bound = p[key][row, k], p["e_" + key][row, k]
                if name == "v" and np.isnan(got) and p["r"][row, k] == 0:
                    continue
                if not abs(got - want) <= bound:
                    out.violations.append((i, f"({inst}, {k}): {name} = {got:.9g}, reference {want:.9g} +- {bound:.3g}"))
            lower = p["t"][row, k] - p["e_t"][row, k]
            if nearest_decided[row] < lower:
                j = int(np.argmin(np.where(cat["state"][row] == HIT, upper[row], np.inf)))
                out.violations.append((i, f"({inst}, {k}) at t = {p['t'][row, k]:.9g}, but pair {j} is a decided hit at {cat['t'][row, j]:.9g}"))
            other = und.copy()
            other[g] = False
            out.undecided[i] = und[g] or (other & (upper[row] < lower)).any()
    return out


def nearest_decided(ref, instances=None):
    """per ray the decided hit of smallest t as (instance, element), (-1, -1) where there is none: what the float64 reference alone knows"""
    out = np.full((len(ref.rays), 2), -1, np.int64)
    which = [k for k, el in enumerate(ref.elements) if instances is None or el.instance in instances]
    for lo in range(0, len(ref.rays), ref.chunk):
        best = np.full(len(ref.rays[lo:lo + ref.chunk]), np.inf)
        for k in which:
            p = ref.block(k, lo)
            t = np.where(p["state"] == HIT, p["t"], np.inf)
            j = t.argmin(1)
            rows = np.nonzero(t[np.arange(len(j)), j] < best)[0]
            best[rows] = t[rows, j[rows]]
            out[lo + rows, 0], out[lo + rows, 1] = ref.elements[k].instance, j[rows]
    return out


def coverage(elements, rays):
    """what a ray set exercises, from the float64 reference alone: {"hits": {instance: decided hits}, "clamped0", "clamped1": decided
    hits with s clamped at that end, "near_misses": decided misses within 1.3 r, "tmin_only": pairs only the tmin comparison rejects}"""
    out = {"hits": {}, "clamped0": 0, "clamped1": 0, "near_misses": 0, "tmin_only": 0}
    for el in elements:
        p = pairs(el, rays)
        hit = p["state"] == HIT
        out["hits"][el.instance] = int(hit.sum())
        out["clamped0"] += int((hit & (p["s"] < 0)).sum())
        out["clamped1"] += int((hit & (p["s"] > 1)).sum())
        out["near_misses"] += int(((p["state"] == MISS) & p["near"]).sum())
        out["tmin_only"] += int(p["tmin_only"].sum())
    return out


# ---- shading: what the reference's debug shaders return on a hit (yocto_pathtrace.cpp:893-930 over yocto_scene.cpp:305-356, 476-526)
def _unit(x):
    return x / _len(x)[..., None]


def _lerp(a, b, u):
    return a * (1 - u)[..., None] + b * u[..., None]


def shade(el, color, element, u, v, outgoing, e_outgoing=0.0):
    """What the debug shaders give for hits {element, u, v} (n,) on one instance seen from `outgoing` (n, 3); `color` is the material's
    (no textures); e_outgoing bounds what the float32 outgoing is off by.  A dict: texcoord (n, 2), color (n, 3), normal (n, 3), and
    e_texcoord, e_color, e_normal (n,), bounds of their float32 evaluation per component: a lerp rounds 1 - u, two products and a sum, at
    most 4 eps (|x0| + |x1|); the colour is then multiplied by the material's and by the (absent) texture's 1, 8 eps in all; the normal
    is derived below."""
    A, i0, i1 = el.arrays, el.ids[element, 0], el.ids[element, 1]
    uv, n_hits = np.stack([u, v], -1), len(u)
    big = lambda x: np.abs(x[i0]).max(-1) + np.abs(x[i1]).max(-1)
    texcoord = uv if not len(A["texcoords"]) else A["texcoords"][i0] if el.points else _lerp(A["texcoords"][i0], A["texcoords"][i1], u)
    e_texcoord = 4 * EPS * big(A["texcoords"]) if len(A["texcoords"]) and not el.points else np.zeros(n_hits)
    shape_color = 1.0 if not len(A["colors"]) else A["colors"][i0, :3] if el.points else _lerp(A["colors"][i0, :3], A["colors"][i1, :3], u)
    col = np.asarray(color, np.float64) * shape_color * np.ones((n_hits, 3))
    e_color = 8 * EPS * np.abs(color).max() * (big(A["colors"]) if len(A["colors"]) else np.ones(n_hits))
    out = {"texcoord": texcoord, "e_texcoord": e_texcoord, "color": col, "e_color": e_color}
    if el.points:   # the "HACK: sphere" branch at uv = {0, 0}: the frame's z axis
        return dict(out, normal=np.broadcast_to(_unit(el.M[:, 2]), (n_hits, 3)), e_normal=np.full(n_hits, 8 * EPS))
    n = _unit(_lerp(A["normals"][i0], A["normals"][i1], u)) if len(A["normals"]) else _unit(A["positions"][i1] - A["positions"][i0])
    n = _unit(n @ el.M.T)
    # the float32 n is within e_n of n: a lerp (4 eps of its operands' lengths, relative to the lerp's own length L, which two
    # opposed normals shrink), two normalisations (4 eps each: a dot, a root, a division) and the frame (4 eps times its condition
    # sqrt(3) G |M| at most); w = outgoing - n (outgoing . n) then carries 4 eps |outgoing| of its own roundings and 2 |outgoing| e_n
    # of n's and 2 e_outgoing of outgoing's (itself and through the dot), and normalising a vector of length |w| turns an absolute
    # error x into x / |w| (plus 4 eps)
    if len(A["normals"]):
        n0, n1 = A["normals"][i0], A["normals"][i1]
        L = _len(_lerp(n0, n1, u))
        e_l = 4 * EPS * (_len(n0) + _len(n1)) / L
    else:
        e_l = EPS * (_len(A["positions"][i1]) + _len(A["positions"][i0])) / _len(A["positions"][i1] - A["positions"][i0])
    cond = np.linalg.norm(el.M) * np.linalg.norm(np.linalg.inv(el.M))
    e_n = (e_l + 4 * EPS) * cond + 4 * EPS * cond + 4 * EPS
    w = outgoing - n * _dot(outgoing, n)[..., None]
    O = _len(outgoing)
    return dict(out, normal=_unit(w), e_normal=(4 * EPS * O + 2 * O * e_n + 2 * e_outgoing) / _len(w) + 4 * EPS)


def camera_rays(camera, width, height):
    """eval_camera (yocto_scene.cpp:67-102) at the pixel centres with the lens sample ignored (aperture 0), in float64: (h, w, 6).
    `camera`: the scene's vpt_camera record; perspective only."""
    assert not camera.orthographic and camera.aperture == 0
    film = (camera.film, camera.film / camera.aspect) if camera.aspect >= 1 else (camera.film * camera.aspect, camera.film)
    centre = lambda n: ((np.arange(n, dtype=np.float32) + np.float32(0.5)) / np.float32(n)).astype(np.float64)   # the shader's float32 u, v
    u, v = centre(width)[None, :], centre(height)[:, None]
    q = np.stack(np.broadcast_arrays(film[0] * (0.5 - u), film[1] * (v - 0.5), np.float64(camera.lens)), -1)
    dc = -_unit(q)
    d = _unit(dc * camera.focus / np.abs(dc[..., 2:3]))
    fr = np.array([list(camera.frame.x), list(camera.frame.y), list(camera.frame.z), list(camera.frame.o)], np.float64)
    out = np.empty((height, width, 6))
    out[..., :3], out[..., 3:] = fr[3], _unit(d @ fr[:3])
    return out
