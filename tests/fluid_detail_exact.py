"""Stage 2b and the MacCormack stage 3 of vpt_scene_fluid_step_detail (include/vpt.h) restated in numpy, vectorised, in float64 - or in the
dtype asked for: the float32 run of this file against its float64 run is the yardstick tests/test_fluid_detail_host.py holds the host
mirror to.  Fields are (d, h, w) arrays as in fluid_exact.py, whose shifts and stages this file uses; nothing here shares a line with
csrc/vpt_fluid_rule.h."""
import numpy as np

import fluid_exact as ex
import fluid_mg_exact as mg


def diff(a, c):
    """a[+1] - a[-1] along component c, the indices clamped to the volume"""
    return ex.shifted(a, c, 1, None) - ex.shifted(a, c, 0, None)


def curl(vel):
    half = vel[0].dtype.type(0.5)
    return [half * (diff(vel[2], 1) - diff(vel[1], 2)), half * (diff(vel[0], 2) - diff(vel[2], 0)), half * (diff(vel[1], 0) - diff(vel[0], 1))]


def confine(vel, k, open_faces):
    """stage 2b and its walls: the velocity plus k times N x omega"""
    dtype = vel[0].dtype.type
    omega = curl(vel)
    m = np.sqrt(omega[0] ** 2 + omega[1] ** 2 + omega[2] ** 2)
    eta = [dtype(0.5) * diff(m, c) for c in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.sqrt(eta[0] ** 2 + eta[1] ** 2 + eta[2] ** 2) + dtype(1e-12)
        N = [e / length for e in eta]
        force = [N[1] * omega[2] - N[2] * omega[1], N[2] * omega[0] - N[0] * omega[2], N[0] * omega[1] - N[1] * omega[0]]
    return walls([u + dtype(k) * f for u, f in zip(vel, force)], open_faces)


def walls(vel, open_faces):
    return [u.astype(vel[0].dtype) for u in ex.walls(vel, open_faces)]   # ex.walls only writes zeros


def corners(field, q):
    """the eight corners the trilerp at q reads and their weights, as fluid_exact.trilerp takes them"""
    shape, dtype = field.shape, field.dtype.type
    lo = [np.minimum(q[c].astype(np.int64), shape[ex.AXIS[c]] - 1) for c in range(3)]
    hi = [np.minimum(lo[c] + 1, shape[ex.AXIS[c]] - 1) for c in range(3)]
    f = [q[c] - lo[c].astype(field.dtype) for c in range(3)]
    for dz, wz in ((lo[2], 1 - f[2]), (hi[2], f[2])):
        for dy, wy in ((lo[1], 1 - f[1]), (hi[1], f[1])):
            for dx, wx in ((lo[0], 1 - f[0]), (hi[0], f[0])):
                yield field[dz, dy, dx], (wx * wy * wz).astype(dtype)


def trace(shape, vel, dt, dtype):
    at = np.meshgrid(*(np.arange(n, dtype=dtype) for n in shape), indexing="ij")
    return [np.clip(at[ex.AXIS[c]] + dtype(dt) * vel[c], 0, shape[ex.AXIS[c]] - 1).astype(dtype) for c in range(3)]


def advect(fields, dt, maccormack):
    """stage 3 of the four fields [rho, u, v, w] by the velocity among them: semi-Lagrangian, or corrected and limited"""
    dtype, shape = fields[0].dtype.type, fields[0].shape
    q, r = trace(shape, fields[1:], -dt, dtype), trace(shape, fields[1:], dt, dtype)
    out = []
    for phi in fields:
        read = list(corners(phi, q))
        hat = sum(v * w for v, w in read)
        if maccormack:
            bar = sum(v * w for v, w in corners(hat, r))
            lo, hi = np.minimum.reduce([v for v, _ in read]), np.maximum.reduce([v for v, _ in read])
            hat = np.clip(hat + dtype(0.5) * (phi - bar), lo, hi)
        out.append(hat.astype(dtype))
    return out


def step(fields, dt, lift, keep_density, keep_velocity, open_faces, advection, vorticity, solver, dtype=np.float64):
    """one whole step of [rho, u, v, w] in `dtype`, the pressure by multigrid (`solver`: cycles, smooth, coarse_sweeps)"""
    f = [np.asarray(a, dtype) for a in fields]
    t = dtype
    rho, vel = f[0] * t(keep_density), [u * t(keep_velocity) + (t(dt) * t(l)) * f[0] for u, l in zip(f[1:], lift)]
    vel = walls(vel, open_faces)
    if vorticity > 0:
        vel = confine(vel, t(dt) * t(vorticity), open_faces)
    rho, *vel = advect([rho, *vel], dt, advection == 1)
    vel = walls(vel, open_faces)
    div = (t(0.5) * sum(diff(vel[c], c) for c in range(3))).astype(dtype)
    p = mg.pressure(div, open_faces, **solver, dtype=dtype)
    near = lambda c, side: ex.shifted(p, c, side, 0.0 if ex.is_open(open_faces, c, side) else None)   # noqa: E731
    vel = walls([(vel[c] - t(0.5) * (near(c, 1) - near(c, 0))).astype(dtype) for c in range(3)], open_faces)
    return [rho, *vel]
