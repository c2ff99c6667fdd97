"""The rule of vpt_scene_fluid_step on the CPU (include/vpt.h, csrc/vpt_fluid_rule.h): every stage of the host mirror and a whole step
against the float64 restatement (tests/fluid_exact.py) within bounds derived from the stages' operation counts, the exact facts of the
rule, the struct size, every refusal, and the ledger.  No GPU: the host mirror is compiled from the header the kernels compile."""
import ctypes as C

import numpy as np
import pytest

import fluid_exact as ex
from test_volgrid_host import load

F = np.float32
U = 2.0 ** -24   # unit roundoff of float32
SLACK = 1 + 1e-3   # the second-order terms of every bound below
WHD = (7, 5, 6)
PARAMS = dict(dt=0.75, lift=(0.125, float(F(0.9)), float(F(-0.3))), keep_density=float(F(0.97)), keep_velocity=float(F(0.99)))   # float32 values


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def fields(seed=3, whd=WHD, scale=1.5):
    g = np.random.default_rng(seed)
    return [g.normal(0, scale, whd[::-1]).astype(F) for _ in range(4)]


def run(vpt, f, stage=None, p=None, div=None, **kw):
    """vpth_fluid_stage (or vpth_fluid_step for stage None) on copies of the four (d, h, w) fields: (return code, message, the copies)"""
    out = [np.ascontiguousarray(a, F).copy() for a in f]
    whd = np.array(out[0].shape[::-1], np.int32)
    abi = vpt.FluidStep(0, (1, 2, 3), **{**PARAMS, **kw}).to_abi()[0]
    err = C.create_string_buffer(256)
    ptr = [a.ctypes.data for a in out]
    if stage is None:
        rc = vpt.host.vpth_fluid_step(*ptr, whd.ctypes.data, C.byref(abi), err, len(err))
    else:
        rc = vpt.host.vpth_fluid_stage(stage, *ptr, None if p is None else p.ctypes.data, None if div is None else div.ctypes.data, whd.ctypes.data, C.byref(abi), err, len(err))
    return rc, err.value.decode(), out


def f64(f):
    return [a.astype(np.float64) for a in f]


def amax(*arrays):
    return max(float(np.abs(a).max()) for a in arrays)


def slope(a):
    """the largest difference between adjacent nodes"""
    return max(float(np.abs(np.diff(a, axis=k)).max()) if a.shape[k] > 1 else 0.0 for k in range(3))


# ---- the bounds, each from the operations csrc/vpt_fluid_rule.h writes (u = 2^-24) ----------------------------------------------------------
def force_bound(u, rho, lift):
    # u kv rounds once; dt * lift and its product with rho round once each; the sum rounds once on at most the two magnitudes together
    a, b = np.abs(u * PARAMS["keep_velocity"]), np.abs(PARAMS["dt"] * lift * rho)
    return (2 * a + 3 * b) * U


def advect_bound(field, vel, dt, e_in=0.0, e_vel=0.0):
    # q = i - dt u: the product and the difference round once each, |dq| <= (|dt u| + W) u, plus dt times what the velocity is off by; the
    # trilerp is piecewise linear with slope <= D per axis (three axes), a convex combination of its nodes (so e_in passes through once),
    # and its own arithmetic costs 13 u V: 1 - f once per weight, three products a term (6 u V in all), seven sums of partial sums <= V
    dq = (abs(dt) * amax(*vel) + max(field.shape)) * U + abs(dt) * e_vel
    return 3 * dq * slope(field) + 13 * U * amax(field) + e_in


def divergence_bound(vel, e_vel=0.0):
    # three differences <= 2 M, the sums <= 4 M and 6 M, each rounded once, all halved (exact): (6 + 4 + 6) M u / 2; six inputs, halved
    return 8 * amax(*vel) * U + 3 * e_vel


def pressure_bound(n, pmax, dmax, e_div=0.0):
    # One sweep: five sums of partial sums <= 2 P .. 6 P (20 P u), s - d on <= 6 P + d (once), the product with the rounded constant 1 / 6
    # (twice), everything over 6: (38 P + 3 d) u / 6.  The sweep is an average of six values (fewer, with zeros, at an open face), so what
    # its inputs are off by comes through once, not multiplied: the error ADDS per sweep; d's own error comes in as a sixth per sweep
    return n * ((38 * pmax + 3 * dmax) * U / 6 + e_div / 6)


def project_bound(vel, pmax, e_vel=0.0, e_p=0.0):
    # hi - lo rounds once on <= 2 P, the half is exact, the difference rounds once on <= M + P; two pressures, halved
    return (2 * pmax + amax(*vel)) * U + e_vel + e_p


def pressure_max(div, n, open_faces):
    return max([amax(ex.pressure(div, k, open_faces)) for k in range(1, n + 1)], default=0.0)


# ---- stage by stage ------------------------------------------------------------------------------------------------------------------------
def test_force_and_walls_against_float64(vpt):
    f = fields()
    rc, _, got = run(vpt, f, 0)
    rho, vel = ex.force(*(lambda r, *v: (r, v))(*f64(f)), **PARAMS)
    assert rc == 0 and (np.abs(got[0] - rho) <= np.abs(rho) * U * SLACK).all()
    for c in range(3):
        assert (np.abs(got[1 + c] - vel[c]) <= force_bound(f64(f)[1 + c], f64(f)[0], PARAMS["lift"][c]) * SLACK).all()
    rc, _, walled = run(vpt, f, 1, open_faces=0b001001)   # -x and +y open
    want = ex.walls(f64(f)[1:], 0b001001)
    assert rc == 0 and all(np.array_equal(bits(walled[1 + c]), bits(want[c])) for c in range(3)) and np.array_equal(bits(walled[0]), bits(f[0]))
    assert (walled[1][:, :, -1] == 0).all() and (walled[1][:, :, 0] != 0).all() and (walled[2][:, -1] != 0).all() and (walled[3][0] == 0).all()


def test_advect_against_float64(vpt):
    f = fields()
    rc, _, got = run(vpt, f, 2)
    rho, vel = ex.advect(f64(f)[0], f64(f)[1:], PARAMS["dt"])
    assert rc == 0
    for a, want, src in zip(got, [rho, *vel], f64(f)):
        assert np.abs(a - want).max() <= advect_bound(src, f64(f)[1:], PARAMS["dt"]) * SLACK and np.abs(a - src).max() > 0.1


@pytest.mark.parametrize("iterations,open_faces", [(1, 0), (8, 0), (8, 0b001000), (40, 63)])
def test_divergence_pressure_and_project_against_float64(vpt, iterations, open_faces):
    f = fields()
    div, p = np.zeros(WHD[::-1], F), np.zeros(WHD[::-1], F)
    assert run(vpt, f, 3, p, div)[0] == 0
    assert np.abs(div - ex.divergence(f64(f)[1:])).max() <= divergence_bound(f64(f)[1:]) * SLACK and amax(div) > 0.5
    assert run(vpt, f, 4, p, div, iterations=iterations, open_faces=open_faces)[0] == 0
    d64 = div.astype(np.float64)   # each stage from the mirror's own inputs
    pmax = pressure_max(d64, iterations, open_faces)
    assert np.abs(p - ex.pressure(d64, iterations, open_faces)).max() <= pressure_bound(iterations, pmax, amax(d64)) * SLACK and amax(p) > 0.05
    rc, _, got = run(vpt, f, 5, p, div, open_faces=open_faces)
    want = ex.project(f64(f)[1:], p.astype(np.float64), open_faces)
    assert rc == 0 and max(np.abs(got[1 + c] - want[c]).max() for c in range(3)) <= project_bound(f64(f)[1:], amax(p)) * SLACK
    assert np.array_equal(bits(got[0]), bits(f[0]))


@pytest.mark.parametrize("iterations,open_faces", [(0, 0), (8, 0b001000), (20, 63)])
def test_a_whole_step_against_float64(vpt, iterations, open_faces):
    """the stage bounds chained: what a stage's inputs are off by enters the next stage's bound where the rule lets it through"""
    f = fields(scale=0.8)
    rc, _, got = run(vpt, f, iterations=iterations, open_faces=open_faces, steps=1)
    dt, lift = PARAMS["dt"], PARAMS["lift"]
    rho1, vel1 = ex.force(f64(f)[0], f64(f)[1:], **PARAMS)
    vel1 = ex.walls(vel1, open_faces)
    e_rho = amax(rho1) * U
    e_vel = max(float(force_bound(f64(f)[1 + c], f64(f)[0], lift[c]).max()) for c in range(3))
    rho2, vel2 = ex.advect(rho1, vel1, dt)
    vel2 = ex.walls(vel2, open_faces)
    e_rho = advect_bound(rho1, vel1, dt, e_rho, e_vel)
    e_vel = max(advect_bound(u, vel1, dt, e_vel, e_vel) for u in vel1)
    div = ex.divergence(vel2)
    pmax = pressure_max(div, iterations, open_faces)
    e_p = pressure_bound(iterations, pmax, amax(div), divergence_bound(vel2, e_vel))
    want = ex.project(vel2, ex.pressure(div, iterations, open_faces), open_faces)
    e_vel = project_bound(vel2, pmax, e_vel, e_p)
    assert rc == 0 and np.abs(got[0] - rho2).max() <= e_rho * SLACK and max(np.abs(got[1 + c] - want[c]).max() for c in range(3)) <= e_vel * SLACK
    assert e_vel < 1e-3 and np.abs(got[1] - f[1]).max() > 0.1   # the bound says something, and so did the step
    faces = [got[1][:, :, 0], got[1][:, :, -1], got[2][:, 0], got[2][:, -1], got[3][0], got[3][-1]]   # closed: the normal component is +0.0f
    assert all(bits(face).any() == bool(open_faces >> n & 1) for n, face in enumerate(faces))


# ---- exact facts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u,dt,shift", [(0.0, 1.0, 0), (None, 0.0, 0), (1.0, 1.0, 1)], ids=["zero velocity", "dt = 0", "one node"])
def test_advection_without_a_displacement_keeps_every_bit_and_by_one_node_shifts_the_interior(vpt, u, dt, shift):
    f = fields()
    if u is not None:
        f[1:] = [np.full_like(f[1], u), np.zeros_like(f[2]), np.zeros_like(f[3])]
    rc, _, got = run(vpt, f, 2, dt=dt)
    w = WHD[0]
    assert rc == 0 and all(np.array_equal(bits(a[:, :, shift:]), bits(b[:, :, :w - shift])) for a, b in zip(got, f))
    assert np.array_equal(bits(got[0][:, :, 0]), bits(f[0][:, :, 0]))


def test_a_divergence_free_field_keeps_its_bits_through_pressure_and_project(vpt):
    g = np.random.default_rng(5)
    d, h, w = WHD[::-1]   # u constant along x, v along y, w along z: every central difference is exactly 0
    f = [g.normal(0, 1, (d, h, w)).astype(F), np.broadcast_to(g.normal(0, 1, (d, h, 1)).astype(F), (d, h, w)),
         np.broadcast_to(g.normal(0, 1, (d, 1, w)).astype(F), (d, h, w)), np.broadcast_to(g.normal(0, 1, (1, h, w)).astype(F), (d, h, w))]
    div, p = np.ones((d, h, w), F), np.ones((d, h, w), F)
    assert run(vpt, f, 3, p, div)[0] == 0 and not div.any()
    assert run(vpt, f, 4, p, div, iterations=6, open_faces=63)[0] == 0 and not p.any()
    rc, _, got = run(vpt, f, 5, p, div, open_faces=63)
    assert rc == 0 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, f))


# ---- the interface ----------------------------------------------------------------------------------------------------------------------------
def test_struct_size_is_the_headers_and_2_to_the_30_nodes_are_refused_from_the_sizes_alone(vpt):
    assert (C.sizeof(vpt.VptFluidStep), vpt.FLUID_RECORD_BYTES, vpt.FLUID_MAX_ITERATIONS, vpt.FLUID_OPEN_ALL, vpt.FLUID_DEFAULT_BLOCK) == (52, 48, 1024, 63, 2)
    whd, err, a = np.array([1024, 1024, 1025], np.int32), C.create_string_buffer(256), np.zeros(1, F)
    step = vpt.FluidStep(0, (1, 2, 3)).to_abi()[0]
    assert vpt.host.vpth_fluid_step(*[a.ctypes.data] * 4, whd.ctypes.data, C.byref(step), err, 256) == -1 and b"2^30" in err.value


def smoke_scene(vpt, shape=None, seed=1):
    """"messy": density 0 (9 x 17 x 30 with NaN and Inf voxels, or a random grid of `shape`), random velocities 2, 3, 4 behind volume 1, volume 5 behind those"""
    host = load(vpt, "messy")
    g = np.random.default_rng(seed)
    if shape is not None:
        host.set_volume(0, g.uniform(0, 1, shape[::-1]).astype(F), res=0.05)
        host.update_volumes()
    for _ in range(3):
        host.add_volume(g.normal(0, 1.2, host.volume(0)[0].shape).astype(F), res=0.05)
    host.add_volume(fill=7.5, whd=(2, 3, 2), res=0.05)
    host.update_volume_set()
    return host


REFUSALS = {   # name -> (fields of the FluidStep, what the message names)
    "id": (dict(density=6), "density: volume id out of range"), "velocity_id": (dict(velocity=(2, -1, 4)), "velocity: volume id out of range"),
    "equal_ids": (dict(velocity=(2, 3, 2)), "two of the four volume ids are equal"), "whd": (dict(velocity=(2, 3, 5)), "whd is not the density's"),
    "dt": (dict(dt=np.inf), "dt is not finite"), "lift": (dict(lift=(0, np.nan, 0)), "lift is not finite"),
    "keep_density": (dict(keep_density=-np.inf), "keep_density is not finite"), "keep_velocity": (dict(keep_velocity=np.nan), "keep_velocity is not finite"),
    "steps": (dict(steps=-1), "steps is negative"), "iterations_low": (dict(iterations=-1), "iterations is not one of 0..1024"),
    "iterations_high": (dict(iterations=1025), "iterations is not one of 0..1024"), "mask": (dict(open_faces=64), "open_faces has bits above the six faces"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_a_refusal_names_its_field_and_writes_nothing(vpt, name):
    host = smoke_scene(vpt)
    before = [bits(host.volume(i)[0]).copy() for i in range(6)]
    changed, named = REFUSALS[name]
    with pytest.raises(vpt.VptError, match=named):
        host.fluid_step(vpt.FluidStep(**{**dict(density=0, velocity=(2, 3, 4)), **changed}))
    assert all(np.array_equal(bits(host.volume(i)[0]), before[i]) for i in range(6)) and host.update_fluid() == []


def test_the_ledger(vpt):
    host = smoke_scene(vpt)   # a step applies at once and waits for update_fluid(); the other voxel edits refuse its volumes, and the reverse
    before = host.volume(0)[0].copy()
    step = host.fluid_step(vpt.FluidStep(0, (2, 3, 4), iterations=3, **PARAMS))
    assert not np.array_equal(bits(host.volume(0)[0]), bits(before))
    for call in (lambda: host.sculpt_volume(3, []), lambda: host.set_volume(0, before), lambda: host.filter_volume(4, [vpt.FilterOp.to_density(0.5)])):
        with pytest.raises(vpt.VptError, match="fluid steps pending"):
            call()
    with pytest.raises(vpt.VptError, match="update_fluid"):
        host.remove_volumes([1])
    host.filter_volume(1, [vpt.FilterOp.to_density(0.5)])   # a volume the steps do not name is free
    assert host.update_fluid() == [step] and host.update_fluid() == []
    with pytest.raises(vpt.VptError, match="filters pending"):
        host.fluid_step(vpt.FluidStep(1, (2, 3, 4)))

