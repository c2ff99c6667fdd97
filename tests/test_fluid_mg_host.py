"""The multigrid pressure of vpt_scene_fluid_step_solver on the CPU (include/vpt.h, csrc/vpt_fluid_rule.h): the host mirror
against the float64 restatement (tests/fluid_mg_exact.py) within four times what the same restatement loses in float32, the one
convergence condition (on the float64 restatement alone), the solver that changes nothing, every refusal, the struct size and the ledger.
No GPU: the host mirror is compiled from the header the kernels compile."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import fluid_exact as ex
import fluid_mg_exact as mg
from test_fluid_host import PARAMS, F, bits, smoke_scene

SOLVER = dict(cycles=3, smooth=2, coarse_sweeps=16)
CASES = [(whd, mask) for whd in ((20, 9, 9), (33, 17, 30)) for mask in (0, 8, 63)]


@lru_cache(maxsize=None)
def case(whd, mask):
    """(the float32 divergence of a seeded, blurred random velocity; the float64 restatement's p for it; what its float32 run is off by)"""
    g = np.random.default_rng(7)
    vel = [g.normal(0, 1, whd[::-1]) for _ in range(3)]
    for _ in range(4):
        for c in range(3):
            vel = [(u + ex.shifted(u, c, 0, None) + ex.shifted(u, c, 1, None)) / 3 for u in vel]
    div = ex.divergence(vel).astype(F)
    p = mg.pressure(div, mask, **SOLVER)
    return div, p, relative(mg.pressure(div, mask, **SOLVER, dtype=F), p)


def relative(p, exact):
    return float(np.linalg.norm(p.astype(np.float64) - exact) / np.linalg.norm(exact))


def mirror_pressure(vpt, div, mask, **solver):
    p, err = np.full(div.shape, 9, F), C.create_string_buffer(256)
    whd = np.array(div.shape[::-1], np.int32)
    rc = vpt.host.vpth_fluid_multigrid_pressure(div.ctypes.data, p.ctypes.data, whd.ctypes.data, mask, C.byref(vpt.FluidSolver(**solver).to_abi()), err, 256)
    assert rc == 0, err.value
    return p


@pytest.mark.parametrize("whd,mask", CASES)
def test_the_mirror_against_float64_within_four_times_float32s_own_error(vpt, whd, mask):
    yardstick = max(case(*c)[2] for c in CASES)   # DESIGN.md §36 records it: 6.5e-7, the closed 20 x 9 x 9
    div, exact, _ = case(whd, mask)
    off = relative(mirror_pressure(vpt, div, mask, **SOLVER), exact)
    print(f"{whd} open {mask}: mirror {off:.3g}, numpy float32 {case(whd, mask)[2]:.3g}, allowed {4 * yardstick:.3g}")
    assert 1e-8 < yardstick < 1e-5 and off <= 4 * yardstick


@pytest.mark.parametrize("whd,mask", CASES)
def test_three_cycles_leave_no_more_residual_than_forty_jacobi_sweeps(whd, mask):
    div, p, _ = case(whd, mask)
    after, jacobi = mg.residual_norm(p, div, mask), mg.residual_norm(ex.pressure(div.astype(np.float64), 40, mask), div, mask)
    print(f"{whd} open {mask}: multigrid {after:.4g}, 40 Jacobi sweeps {jacobi:.4g}, of {mg.residual_norm(np.zeros_like(p), div, mask):.4g}")
    assert after <= jacobi


def test_one_node_and_no_cycles(vpt):
    one = np.array([[[2.5]]], F)   # D == 0 behind closed faces: the node keeps its 0; all open: D = 6, p = -d / 6 at once
    assert bits(mirror_pressure(vpt, one, 0, **SOLVER))[0, 0, 0] == 0
    assert mirror_pressure(vpt, one, 63, **SOLVER)[0, 0, 0] == F(-2.5) / F(6)
    assert not mirror_pressure(vpt, case((20, 9, 9), 8)[0], 8, cycles=0, smooth=1, coarse_sweeps=1).any()


def fields_of(host):
    return [bits(host.volume(i)[0]).copy() for i in range(6)]


@pytest.mark.parametrize("solver", [None, dict(kind=0, cycles=-5, smooth=0, coarse_sweeps=0)], ids=["null", "jacobi"])
def test_a_null_or_jacobi_solver_is_fluid_step(vpt, solver):
    a, b = smoke_scene(vpt), smoke_scene(vpt)
    step = vpt.FluidStep(0, (2, 3, 4), iterations=5, open_faces=8, **PARAMS)
    a.fluid_step(step)
    b.fluid_step(step, solver and vpt.FluidSolver(**solver))   # kind JACOBI: the other fields are not read
    assert all(np.array_equal(x, y) for x, y in zip(fields_of(a), fields_of(b)))
    c = smoke_scene(vpt)
    c.fluid_step(step, vpt.FluidSolver(**SOLVER))
    assert not np.array_equal(fields_of(a)[2], fields_of(c)[2]) and np.array_equal(fields_of(a)[0], fields_of(c)[0])   # the pressure moves no density


REFUSALS = {"kind": (dict(kind=2), "solver: kind"), "cycles_low": (dict(cycles=-1), "solver: cycles is not one of 0..64"),
            "cycles_high": (dict(cycles=65), "solver: cycles"), "smooth_low": (dict(smooth=0), "solver: smooth is not one of 1..4"),
            "smooth_high": (dict(smooth=5), "solver: smooth"), "coarse_low": (dict(coarse_sweeps=0), "solver: coarse_sweeps is not one of 1..64"),
            "coarse_high": (dict(coarse_sweeps=65), "solver: coarse_sweeps"), "step": (dict(), "iterations is not one of 0..1024")}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_a_refusal_names_its_field_and_writes_nothing(vpt, name):
    host = smoke_scene(vpt)
    before = fields_of(host)
    changed, named = REFUSALS[name]
    with pytest.raises(vpt.VptError, match=named):   # with MULTIGRID the step's iterations is not used, and validated as before
        host.fluid_step(vpt.FluidStep(0, (2, 3, 4), iterations=1025 if name == "step" else 4), vpt.FluidSolver(**{**SOLVER, **changed}))
    assert all(np.array_equal(a, b) for a, b in zip(fields_of(host), before)) and host.update_fluid() == []


def test_struct_size_and_the_ledger_carries_the_solver(vpt):
    assert (C.sizeof(vpt.VptFluidSolver), vpt.FLUID_JACOBI, vpt.FLUID_MULTIGRID, vpt.FLUID_MAX_CYCLES) == (16, 0, 1, 64)
    host = smoke_scene(vpt)
    solver = vpt.FluidSolver(cycles=2, smooth=1, coarse_sweeps=4)
    plain = host.fluid_step(vpt.FluidStep(0, (2, 3, 4), iterations=3, **PARAMS))
    noted = host.fluid_step(vpt.FluidStep(0, (2, 3, 4), **PARAMS), solver)
    assert plain.solver is None and noted.solver == solver and host.update_fluid() == [plain, noted] and host.update_fluid() == []
    assert (solver.launches(noted, (9, 17, 30), 2), solver.launches(noted, (9, 17, 30), 4), solver.launches(noted, (8, 8, 1))) == (5 + 2 * 7, 5 + 2 * 7, 7)
    assert vpt.FluidSolver(smooth=3).launches(noted, (9, 17, 30), 4) == 5 + 3 * (2 * (2 * 2 + 1) + 1) and vpt.FluidSolver(kind=0).launches(plain, (9, 17, 30)) == plain.launches()
