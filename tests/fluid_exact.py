"""The seven stages of vpt_scene_fluid_step (include/vpt.h) restated in float64 numpy, vectorised: what tests/test_fluid_host.py holds the
host mirror to, in the role volgrid_exact.py has for the volgrid shader.  Fields are (d, h, w) arrays; open_faces bit 0..5 = -x, +x, -y,
+y, -z, +z.  Nothing here shares a line with csrc/vpt_fluid_rule.h."""
import numpy as np

AXIS = (2, 1, 0)   # the numpy axis of x, y, z


def is_open(open_faces, c, side):
    return bool(open_faces >> (2 * c + side) & 1)


def force(rho, vel, dt, lift, keep_density, keep_velocity):
    return rho * keep_density, [u * keep_velocity + (dt * l) * rho for u, l in zip(vel, lift)]


def walls(vel, open_faces):
    out = [np.array(u, np.float64) for u in vel]
    for c, u in enumerate(out):
        for side in (0, 1):
            if not is_open(open_faces, c, side):
                u[tuple(-side if a == AXIS[c] else slice(None) for a in range(3))] = 0.0
    return out


def trilerp(field, q):
    shape = field.shape
    lo = [np.minimum(q[c].astype(np.int64), shape[AXIS[c]] - 1) for c in range(3)]
    hi = [np.minimum(lo[c] + 1, shape[AXIS[c]] - 1) for c in range(3)]
    f = [q[c] - lo[c] for c in range(3)]
    out = 0.0
    for dz, wz in ((lo[2], 1 - f[2]), (hi[2], f[2])):
        for dy, wy in ((lo[1], 1 - f[1]), (hi[1], f[1])):
            for dx, wx in ((lo[0], 1 - f[0]), (hi[0], f[0])):
                out = out + field[dz, dy, dx] * wx * wy * wz
    return out


def advect(rho, vel, dt):
    """the clamped node coordinates every node came from, then the four fields there"""
    shape = rho.shape
    at = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    q = [np.clip(at[AXIS[c]] - dt * vel[c], 0, shape[AXIS[c]] - 1) for c in range(3)]
    return trilerp(rho, q), [trilerp(u, q) for u in vel]


def shifted(p, c, side, fill):
    """p at the neighbour on `side` (0: -, 1: +) along component c; beyond the volume: the edge node (fill None) or `fill`"""
    a = AXIS[c]
    width = [(1, 1) if b == a else (0, 0) for b in range(3)]
    pad = np.pad(p, width, mode="edge") if fill is None else np.pad(p, width, mode="constant", constant_values=fill)
    return np.take(pad, np.arange(p.shape[a]) + 2 * side, axis=a)


def divergence(vel):
    return 0.5 * sum(shifted(vel[c], c, 1, None) - shifted(vel[c], c, 0, None) for c in range(3))


def near(p, c, side, open_faces):
    return shifted(p, c, side, 0.0 if is_open(open_faces, c, side) else None)


def pressure(div, iterations, open_faces):
    p = np.zeros_like(div, np.float64)
    for _ in range(iterations):
        p = (sum(near(p, c, side, open_faces) for c in range(3) for side in (0, 1)) - div) / 6
    return p


def project(vel, p, open_faces):
    return walls([vel[c] - 0.5 * (near(p, c, 1, open_faces) - near(p, c, 0, open_faces)) for c in range(3)], open_faces)

