"""Stage 2b and the MacCormack advection of vpt_scene_fluid_step_detail on the CPU (include/vpt.h, csrc/vpt_fluid_rule.h): the
host mirror against the float64 restatement (tests/fluid_detail_exact.py) within four times what the same restatement loses in float32,
the exact facts of the rule, what MacCormack is for (on the float64 restatement alone), the detail that changes nothing, the refusals, the
struct size and the ledger.  No GPU: the host mirror is compiled from the header the kernels compile."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import fluid_detail_exact as dx
from test_fluid_host import PARAMS, F, bits, fields, smoke_scene
from test_fluid_mg_host import SOLVER, fields_of

DETAILS = {"maccormack": dict(advection=1, vorticity=0.0), "confine": dict(advection=0, vorticity=0.3), "both": dict(advection=1, vorticity=0.3)}
CASES = [(whd, mask, name) for whd in ((20, 9, 9), (9, 17, 30)) for mask in (0, 8, 63) for name in DETAILS]


def relative(got, exact):
    return float(np.linalg.norm(np.concatenate(got).astype(np.float64) - np.concatenate(exact)) / np.linalg.norm(np.concatenate(exact)))


@lru_cache(maxsize=None)
def case(whd, mask, name):
    """(four seeded random float32 fields; the float64 restatement's step of them; what its float32 run is off by)"""
    f = fields(seed=11, whd=whd, scale=0.8)
    run = lambda dtype: dx.step(f, **PARAMS, open_faces=mask, **DETAILS[name], solver=SOLVER, dtype=dtype)   # noqa: E731
    exact = run(np.float64)
    return f, exact, relative(run(F), exact)


def mirror(vpt, f, detail, stage=None, **step):
    """vpth_fluid_step_detail with the multigrid SOLVER (or vpth_fluid_detail_stage `stage`) on copies of four (d, h, w) fields: the copies"""
    out, err = [np.ascontiguousarray(a, F).copy() for a in f], C.create_string_buffer(256)
    whd = np.array(out[0].shape[::-1], np.int32)
    args = [*[a.ctypes.data for a in out], whd.ctypes.data, C.byref(vpt.FluidStep(0, (1, 2, 3), **step).to_abi()[0])]
    if stage is None:
        rc = vpt.host.vpth_fluid_step_detail(*args, C.byref(vpt.FluidSolver(**SOLVER).to_abi()), C.byref(detail.to_abi()), err, 256)
    else:
        rc = vpt.host.vpth_fluid_detail_stage(stage, *args, C.byref(detail.to_abi()), err, 256)
    assert rc == 0, err.value
    return out


@pytest.mark.parametrize("whd,mask,name", CASES)
def test_the_mirror_against_float64_within_four_times_float32s_own_error(vpt, whd, mask, name):
    yardstick = max(case(*c)[2] for c in CASES)
    f, exact, own = case(whd, mask, name)
    off = relative(mirror(vpt, f, vpt.FluidDetail(**DETAILS[name]), open_faces=mask, **PARAMS), exact)
    print(f"{whd} open {mask} {name}: mirror {off:.3g}, numpy float32 {own:.3g}, allowed {4 * yardstick:.3g}")
    assert 1e-8 < yardstick < 1e-5 and off <= 4 * yardstick


def test_confinement_leaves_a_rigid_rotation_alone(vpt):
    z, y, x = np.meshgrid(np.arange(7.0), np.arange(8.0), np.arange(9.0), indexing="ij")
    f = [np.ones_like(x), 3 - y, x - 4, np.zeros_like(x)]   # constant curl: m is flat two nodes from a face, eta = 0 there, N = 0 and f = +0
    got = mirror(vpt, f, vpt.FluidDetail(vorticity=0.3), 0, open_faces=63, **PARAMS)
    assert all(np.array_equal(bits(a)[2:-2, 2:-2, 2:-2], bits(b)[2:-2, 2:-2, 2:-2]) for a, b in zip(got, f))
    assert not np.array_equal(bits(got[1]), bits(f[1]))   # (near the faces the one-sided differences bend m)


def test_maccormack_equals_semi_lagrangian_on_a_linear_field(vpt):
    z, y, x = np.meshgrid(np.arange(9.0), np.arange(10.0), np.arange(12.0), indexing="ij")
    f = [2 * x + 3 * y - z, np.full_like(x, 0.25), np.full_like(x, 0.5), np.full_like(x, -0.25)]
    plain, err, whd = [a.astype(F) for a in f], C.create_string_buffer(256), np.array([12, 10, 9], np.int32)
    step = vpt.FluidStep(0, (1, 2, 3), dt=1.0).to_abi()[0]
    assert vpt.host.vpth_fluid_stage(2, *[a.ctypes.data for a in plain], None, None, whd.ctypes.data, C.byref(step), err, 256) == 0
    got = mirror(vpt, f, vpt.FluidDetail(advection=vpt.FLUID_MACCORMACK), 1, dt=1.0)
    # both traces are exact on a linear field, so the correction is a rounding residue: 4 ulp of the largest value
    assert np.abs(got[0] - plain[0])[2:-2, 2:-2, 2:-2].max() <= 4 * np.spacing(F(np.abs(f[0]).max())) and np.abs(plain[0] - f[0]).max() > 1


def test_maccormack_beats_semi_lagrangian_on_a_smooth_field():
    at = np.meshgrid(*[np.arange(32.0)] * 3, indexing="ij")
    wave = lambda shift: np.prod([np.sin(2 * np.pi * (a - s) / 16) for a, s in zip(at, shift)], axis=0)   # noqa: E731
    vel = [np.full((32,) * 3, u) for u in (0.25, 0.5, -0.25)]
    off = {}
    for maccormack in (False, True):
        phi = wave((0, 0, 0))
        for _ in range(8):
            phi = dx.advect([phi, *vel], 1.0, maccormack)[0]
        off[maccormack] = float(np.linalg.norm(phi - wave((-2.0, 4.0, 2.0))))   # eight steps of (w, v, u) along (z, y, x)
    print(f"L2 error after 8 steps: semi-Lagrangian {off[False]:.4g}, MacCormack {off[True]:.4g}, ratio {off[False] / off[True]:.3g}")
    assert off[True] < off[False]


def test_the_limiter_holds(vpt):
    f = case((9, 17, 30), 8, "maccormack")[0]
    rho = mirror(vpt, f, vpt.FluidDetail(advection=vpt.FLUID_MACCORMACK), 1, **PARAMS)[0]
    assert f[0].min() <= rho.min() and rho.max() <= f[0].max() and not np.array_equal(rho, f[0])


@pytest.mark.parametrize("detail", [None, dict()], ids=["null", "off"])
def test_a_null_or_off_detail_is_fluid_step_with_a_solver(vpt, detail):
    a, b = smoke_scene(vpt), smoke_scene(vpt)
    step = vpt.FluidStep(0, (2, 3, 4), open_faces=8, **PARAMS)
    a.fluid_step(step, vpt.FluidSolver(**SOLVER))
    noted = b.fluid_step(step, vpt.FluidSolver(**SOLVER), detail if detail is None else vpt.FluidDetail(**detail))
    assert all(np.array_equal(x, y) for x, y in zip(fields_of(a), fields_of(b))) and noted.payload_bytes() == vpt.FLUID_RECORD_BYTES


@pytest.mark.parametrize("detail,named", [(dict(advection=2), "fluid: detail: advection"), (dict(vorticity=np.nan), "fluid: detail: vorticity"),
                                          (dict(vorticity=-0.5), "fluid: detail: vorticity is not finite or is negative")], ids=["advection", "nan", "negative"])
def test_a_refusal_names_its_field_and_writes_nothing(vpt, detail, named):
    host = smoke_scene(vpt)
    before = fields_of(host)
    with pytest.raises(vpt.VptError, match=named):
        host.fluid_step(vpt.FluidStep(0, (2, 3, 4)), detail=vpt.FluidDetail(**detail))
    assert all(np.array_equal(a, b) for a, b in zip(fields_of(host), before)) and host.update_fluid() == []


def test_struct_size_and_the_ledger_carries_the_detail(vpt):
    assert (C.sizeof(vpt.VptFluidDetail), vpt.FLUID_SEMI_LAGRANGIAN, vpt.FLUID_MACCORMACK, vpt.FLUID_DETAIL_BYTES) == (8, 0, 1, 8)
    host, detail = smoke_scene(vpt), vpt.FluidDetail(vpt.FLUID_MACCORMACK, 0.3)
    plain = host.fluid_step(vpt.FluidStep(0, (2, 3, 4), iterations=3, **PARAMS))
    noted = host.fluid_step(vpt.FluidStep(0, (2, 3, 4), iterations=3, steps=2, **PARAMS), detail=detail)
    assert plain.detail is None and noted.detail == detail and host.update_fluid() == [plain, noted] and noted.payload_bytes() == 56
    assert (detail.launches(noted, (9, 17, 30)), vpt.FluidDetail(vorticity=1.0).launches(noted, (9, 17, 30)), detail.launches(noted, (9, 0, 3))) == (2 * 8, 2 * 7, noted.launches())
