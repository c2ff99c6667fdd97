"""Float64 references for the volgrid shader (include/vpt.h: VPT_SHADER_VOLGRID), plain numpy, no project code: what the kernel's free
flight and its paths are held to in test_volgrid_exact_host.py (the references on their own) and test_volgrid_exact_gpu.py.

  optical_depth    tau(t) along a world ray through trilinear grids: the exact integral, piece by piece between node planes
  pcg_advance, rand1f, rng_skip   PCG32 as the kernels draw it, on (n, 2) uint64 arrays, to replay draws
  ks_sqrt_n        the Kolmogorov statistic of free flights against 1 - exp(-tau(t)), escapes an atom at infinity
  reference_paths  a Monte Carlo path tracer for homogeneous boxes: analytic free flights, no delta tracking, no roulette, no MIS

A grid instance is a dict (`grid_instance`): voxels (d, h, w), res, frame (12 floats x, y, z, o: local = x p.x + y p.y + z p.z + o, an
orthonormal frame), scalef, trdepth - the float32 numbers the scene holds, everything after them float64."""
import numpy as np

F = np.float32
GL4_X, GL4_W = np.polynomial.legendre.leggauss(4)     # exact for polynomials of degree <= 7: a trilerp along a ray is a cubic
GL16_X, GL16_W = np.polynomial.legendre.leggauss(16)  # for smooth integrands that are no polynomials (sigma exp(-tau))


# ---- (a) optical depth ----------------------------------------------------------------------------------------------------------------------
def grid_instance(voxels, res, frame, scalef, trdepth):
    voxels = np.asarray(voxels)
    assert voxels.ndim == 3 and np.isfinite(voxels).all() and (voxels >= 0).all(), "only finite non-negative grids: clean() is the identity"
    return {"voxels": voxels.astype(np.float64), "res": F(res), "frame": np.asarray(frame, F).reshape(12), "scalef": F(scalef), "trdepth": F(trdepth)}


def describe(scene, count):
    """the first `count` grid instances of a scene object with volume(), volume_instance() and material() getters"""
    out = []
    for g in range(count):
        vi = scene.volume_instance(g)
        voxels, res = scene.volume(vi.volume)
        frame = [*vi.frame.x, *vi.frame.y, *vi.frame.z, *vi.frame.o]
        out.append(grid_instance(voxels, res, frame, vi.scalef, scene.material(vi.material).trdepth))
    return out


def bbox_of(inst):
    """the float32 box the record holds, (res * whd) * scalef, as float64: (3,) for x, y, z"""
    d, h, w = inst["voxels"].shape
    return np.array([F(F(inst["res"] * F(n)) * inst["scalef"]) for n in (w, h, d)], np.float64)


def to_local(inst, o, d):
    f = inst["frame"].astype(np.float64)
    R = np.stack([f[0:3], f[3:6], f[6:9]], axis=1)    # columns x, y, z
    return R @ np.asarray(o, np.float64) + f[9:12], R @ np.asarray(d, np.float64)


def to_world(inst, pl, dl=None):
    """the inverse of to_local for an orthonormal frame: a point, or (point, direction)"""
    f = inst["frame"].astype(np.float64)
    R = np.stack([f[0:3], f[3:6], f[6:9]], axis=1)
    p = R.T @ (np.asarray(pl, np.float64) - f[9:12])
    return p if dl is None else (p, R.T @ np.asarray(dl, np.float64))


def box_interval(inst, o, d):
    """the parameters at which the world ray is inside the instance's box, clipped at 0: (t0, t1), or None if it misses"""
    ol, dl = to_local(inst, o, d)
    bbox = bbox_of(inst)
    t0, t1 = 0.0, np.inf
    for k in range(3):
        if dl[k] == 0:
            if not 0 <= ol[k] <= bbox[k]:
                return None
        else:
            a, b = (0 - ol[k]) / dl[k], (bbox[k] - ol[k]) / dl[k]
            t0, t1 = max(t0, min(a, b)), min(t1, max(a, b))
    return (t0, t1) if t0 < t1 else None


def _node(inst, ol, dl, t):
    """node coordinates (.., 3) of the ray at parameters t: pl / bbox * (W - 1)"""
    d, h, w = inst["voxels"].shape
    return (ol + dl * np.asarray(t)[..., None]) / bbox_of(inst) * (np.array([w, h, d]) - 1)


def _trilerp(inst, cell, node):
    """the trilinear polynomial of the cell `cell` (.., 3 ints: x, y, z) at node coordinates `node` (.., 3), over trdepth"""
    v = inst["voxels"]
    top = np.array(v.shape[::-1]) - 1
    i = np.minimum(cell, top)
    ii = np.minimum(i + 1, top)
    f = node - i
    out = 0.0
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                x, y, z = (ii if dx else i)[..., 0], (ii if dy else i)[..., 1], (ii if dz else i)[..., 2]
                wgt = (f[..., 0] if dx else 1 - f[..., 0]) * (f[..., 1] if dy else 1 - f[..., 1]) * (f[..., 2] if dz else 1 - f[..., 2])
                out = out + v[z, y, x] * wgt
    return out / np.float64(inst["trdepth"])


class _Pieces:
    """one instance along one ray: the cuts t_0 < .. < t_m of its box interval at every integer node plane, the cell of every piece, the
    integral of sigma over every piece"""

    def __init__(self, inst, o, d, halve):
        self.inst = inst
        self.ol, self.dl = to_local(inst, o, d)
        iv = box_interval(inst, o, d)
        self.cuts = np.zeros(1)
        self.cum = np.zeros(1)
        self.cells = np.zeros((0, 3), np.int64)
        if iv is None:
            return
        t0, t1 = iv
        bbox = bbox_of(inst)
        dims = np.array(inst["voxels"].shape[::-1])
        cuts = [np.array([t0, t1])]
        for k in range(3):
            if self.dl[k] != 0 and dims[k] > 1:
                planes = np.arange(dims[k]) * bbox[k] / (dims[k] - 1)
                tk = (planes - self.ol[k]) / self.dl[k]
                cuts.append(tk[(tk > t0) & (tk < t1)])
        cuts = np.unique(np.concatenate(cuts))
        if halve:
            cuts = np.unique(np.concatenate([cuts, (cuts[:-1] + cuts[1:]) / 2]))
        self.cuts = cuts
        mid = (cuts[:-1] + cuts[1:]) / 2
        self.cells = np.clip(np.floor(_node(inst, self.ol, self.dl, mid)).astype(np.int64), 0, np.maximum(dims - 2, 0))
        self.cum = np.concatenate([[0.0], np.cumsum(self._integral(np.arange(len(mid)), cuts[:-1], cuts[1:]))])

    def sigma(self, k, t):
        """sigma at parameters t, each on piece k (the piece's own polynomial)"""
        return _trilerp(self.inst, self.cells[k][..., None, :] if np.ndim(t) > np.ndim(k) else self.cells[k], _node(self.inst, self.ol, self.dl, t))

    def _integral(self, k, a, b, x=GL4_X, w=GL4_W):
        t = a[:, None] + (b - a)[:, None] * (x + 1) / 2
        return (b - a) / 2 * (self.sigma(k, t) * w).sum(axis=1)

    def locate(self, t):
        """the piece of each t in [t_0, t_m] (ends clamped), and t clamped into it"""
        k = np.clip(np.searchsorted(self.cuts, t, "right") - 1, 0, len(self.cuts) - 2)
        return k, np.clip(t, self.cuts[k], self.cuts[k + 1])

    def tau(self, t):
        t = np.atleast_1d(np.asarray(t, np.float64))
        if len(self.cells) == 0:
            return np.zeros(t.shape)
        k, b = self.locate(t)
        return self.cum[k] + self._integral(k, self.cuts[k], b)

    def sigma_at(self, t):
        """sigma at any parameters: 0 outside the box interval"""
        t = np.atleast_1d(np.asarray(t, np.float64))
        if len(self.cells) == 0:
            return np.zeros(t.shape)
        k, b = self.locate(t)
        return np.where((t >= self.cuts[0]) & (t <= self.cuts[-1]), self.sigma(k, b), 0.0)


class OpticalDepth:
    """tau(t) of a world ray (o, d) through grid instances: callable on arrays of t, exact up to float64 rounding"""

    def __init__(self, instances, o, d, only=None, halve=False):
        picked = instances if only is None else [instances[only]]
        self.parts = [_Pieces(inst, o, d, halve) for inst in picked]
        self.total = float(sum(p.cum[-1] for p in self.parts))

    def __call__(self, t):
        return sum(p.tau(t) for p in self.parts)

    def sigma(self, t):
        return sum(p.sigma_at(t) for p in self.parts)

    def cuts(self):
        return np.unique(np.concatenate([p.cuts for p in self.parts if len(p.cells)] or [np.zeros(1)]))

    def cdf(self, t, scale=1.0):
        """the unconditional distribution of the free flight, 1 - exp(-scale tau(t))"""
        return -np.expm1(-scale * self(t))

    def invert(self, target):
        """t with tau(t) = target for 0 <= target < total, by a safeguarded Newton iteration (tau' = sigma)"""
        target = np.asarray(target, np.float64)
        cuts = self.cuts()
        at = self(cuts)
        k = np.clip(np.searchsorted(at, target, "right") - 1, 0, len(cuts) - 2)
        lo, hi = cuts[k].copy(), cuts[k + 1].copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            x = lo + (hi - lo) * np.nan_to_num((target - at[k]) / (at[k + 1] - at[k]), nan=0.5, posinf=0.5)   # tau linear over the piece
        todo = np.arange(len(x))   # the targets not met yet: only they are evaluated again
        for _ in range(80):
            f = self(x[todo]) - target[todo]
            todo, f = todo[np.abs(f) > 1e-12], f[np.abs(f) > 1e-12]
            if len(todo) == 0:
                break
            lo[todo], hi[todo] = np.where(f < 0, x[todo], lo[todo]), np.where(f >= 0, x[todo], hi[todo])
            s = self.sigma(x[todo])
            with np.errstate(divide="ignore", invalid="ignore"):
                step = x[todo] - f / s
            x[todo] = np.where((s > 0) & (step >= lo[todo]) & (step <= hi[todo]), step, (lo[todo] + hi[todo]) / 2)
        return x

    def share(self, g):
        """the probability that a flight that collides collides in part g: the integral of sigma_g exp(-tau) over t, over 1 - exp(-total)"""
        cuts = self.cuts()
        a, b = cuts[:-1], cuts[1:]
        t = a[:, None] + (b - a)[:, None] * (GL16_X + 1) / 2
        flat = t.reshape(-1)
        integrand = (self.parts[g].sigma_at(flat) * np.exp(-self(flat))).reshape(t.shape)
        return float(((b - a) / 2 * (integrand * GL16_W).sum(axis=1)).sum() / -np.expm1(-self.total))


def optical_depth(instances, o, d, only=None, halve=False):
    """(tau, tau_total) of the world ray o + t d, t >= 0, through `instances` (all of them, or instance `only`); tau is callable on arrays
    of t.  halve: every piece cut in two, the check of the routine against itself"""
    tau = OpticalDepth(instances, o, d, only, halve)
    return tau, tau.total


# ---- (b) PCG32 ------------------------------------------------------------------------------------------------------------------------------
PCG_MULT = np.uint64(6364136223846793005)


def pcg_advance(rng):
    """one step of (n, 2) uint64 streams {state, inc}: (the streams after it, the uint32 outputs)"""
    rng = np.asarray(rng, np.uint64).reshape(-1, 2)
    old = rng[:, 0]
    with np.errstate(over="ignore"):
        state = old * PCG_MULT + rng[:, 1]
    xs = (((old >> np.uint64(18)) ^ old) >> np.uint64(27)).astype(np.uint32)
    rot = (old >> np.uint64(59)).astype(np.uint32)
    out = (xs >> rot) | (xs << ((~rot + np.uint32(1)) & np.uint32(31)))
    return np.stack([state, rng[:, 1]], axis=1), out


def rand1f(rng):
    """(the streams after one draw, the float32 in [0, 1) the kernels make of it)"""
    rng, bits = pcg_advance(rng)
    return rng, ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(F) - F(1)


def rng_skip(rng, draws):
    for _ in range(draws):
        rng, _ = pcg_advance(rng)
    return rng


# ---- (c) Kolmogorov's statistic -------------------------------------------------------------------------------------------------------------
def ks_sqrt_n(t_collided, S, cdf):
    """sqrt(S) D for S flights of which len(t_collided) collided, at those parameters, against the unconditional distribution cdf(t) =
    1 - exp(-tau(t)); the flights that escaped are an atom at +infinity, so the escape fraction is part of D"""
    t = np.sort(np.asarray(t_collided, np.float64))
    k = len(t)
    assert k <= S
    d = abs(k / S - float(cdf(np.array([np.inf]))[0]))          # the step at infinity: the collided fraction against F(infinity-)
    if k:
        Fi = cdf(t)
        i = np.arange(1, k + 1)
        d = max(d, float((i / S - Fi).max()), float((Fi - (i - 1) / S).max()))
    return float(np.sqrt(S) * d)


# ---- (d) the path tracer ----------------------------------------------------------------------------------------------------------------------
def box_medium(lo, hi, sigma, albedo, g, emission=(0, 0, 0)):
    return {"lo": np.asarray(lo, np.float64), "hi": np.asarray(hi, np.float64), "sigma": float(sigma), "albedo": np.asarray(albedo, np.float64) * np.ones(3),
            "g": float(g), "emission": np.asarray(emission, np.float64) * np.ones(3)}


def _basis(z):
    """unit vectors x, y with (x, y, z) orthonormal, for unit z (n, 3)"""
    a = np.where((np.abs(z[:, 0]) < 0.6)[:, None], np.array([1.0, 0, 0]), np.array([0, 1.0, 0]))
    x = np.cross(a, z)
    x /= np.linalg.norm(x, axis=1)[:, None]
    return x, np.cross(z, x)


def hg_cosine(g, xi):
    """the cosine between the old and the new direction of travel under Henyey-Greenstein's phase function with mean cosine g, from a
    uniform xi by inversion of its distribution (xi = 1: straight on); |g| < 1e-3: isotropic"""
    g, xi = np.broadcast_arrays(np.asarray(g, np.float64), np.asarray(xi, np.float64))
    iso = np.abs(g) < 1e-3
    gs = np.where(iso, 1.0, g)
    return np.where(iso, 1 - 2 * xi, (1 + gs * gs - ((1 - gs * gs) / (1 - gs + 2 * gs * xi)) ** 2) / (2 * gs))


def reference_paths(boxes, environment, bounces, paths, seed, rect, z_start=3.0):
    """Per-path (radiance (paths, 3), hit (paths,)) of the volgrid path rule for a union of axis-aligned homogeneous boxes seen by an
    orthographic camera looking down -z: camera rays start uniformly over rect = (x0, x1, y0, y1) at z_start.  Free flights are analytic
    per box (t0 - ln(1 - u) / sigma inside its slab interval), the nearest collision over the boxes wins; a collision adds weight *
    emission, scatters by Henyey-Greenstein about the direction of travel (g > 0: forward) and multiplies the weight by the albedo;
    escape adds weight * environment (a constant radiance); a path ends after `bounces` collisions.  No delta tracking, no bricks, no
    roulette, no MIS."""
    gen = np.random.default_rng(seed)
    env = np.asarray(environment, np.float64) * np.ones(3)
    radiance, hit = np.zeros((paths, 3)), np.zeros(paths)
    x0, x1, y0, y1 = rect
    pos = np.stack([gen.uniform(x0, x1, paths), gen.uniform(y0, y1, paths), np.full(paths, float(z_start))], axis=1)
    dirs = np.tile(np.array([0.0, 0.0, -1.0]), (paths, 1))
    weight = np.ones((paths, 3))
    alive = np.arange(paths)
    for bounce in range(bounces):
        if len(alive) == 0:
            break
        n = len(alive)
        best_t, best_box = np.full(n, np.inf), np.full(n, -1)
        for b, box in enumerate(boxes):
            with np.errstate(divide="ignore", invalid="ignore"):
                ta, tb = (box["lo"] - pos) / dirs, (box["hi"] - pos) / dirs
            inside = (pos >= box["lo"]) & (pos <= box["hi"])
            par = dirs == 0
            near = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(ta, tb))
            far = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(ta, tb))
            t0, t1 = np.maximum(near.max(axis=1), 0.0), far.min(axis=1)
            t = t0 - np.log1p(-gen.uniform(0, 1, n)) / box["sigma"]
            take = (t0 < t1) & (t < t1) & (t < best_t)
            best_t, best_box = np.where(take, t, best_t), np.where(take, b, best_box)
        escaped = best_box < 0
        radiance[alive[escaped]] += weight[escaped] * env
        keep = ~escaped
        alive, pos, dirs, weight, best_t, best_box = alive[keep], pos[keep], dirs[keep], weight[keep], best_t[keep], best_box[keep]
        n = len(alive)
        if bounce == 0:
            hit[alive] = 1
        pos = pos + dirs * best_t[:, None]
        emission = np.stack([b["emission"] for b in boxes])[best_box]
        albedo = np.stack([b["albedo"] for b in boxes])[best_box]
        g = np.array([b["g"] for b in boxes])[best_box]
        radiance[alive] += weight * emission
        # Henyey-Greenstein: the cosine of the angle between the old and the new direction of travel, by inversion of its distribution
        xi, phi = gen.uniform(0, 1, n), gen.uniform(0, 2 * np.pi, n)
        cos_t = hg_cosine(g, xi)
        sin_t = np.sqrt(np.maximum(0.0, 1 - cos_t * cos_t))
        bx, by = _basis(dirs)
        dirs = bx * (sin_t * np.cos(phi))[:, None] + by * (sin_t * np.sin(phi))[:, None] + dirs * cos_t[:, None]
        dirs /= np.linalg.norm(dirs, axis=1)[:, None]
        weight = weight * albedo
        keep = weight.max(axis=1) > 0
        alive, pos, dirs, weight = alive[keep], pos[keep], dirs[keep], weight[keep]
    return radiance, hit


def mean_and_se(values):
    """(mean, standard error) per column of independent samples"""
    values = np.asarray(values, np.float64)
    return values.mean(axis=0), values.std(axis=0, ddof=1) / np.sqrt(len(values))
