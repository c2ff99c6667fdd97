"""vpt_scene_fluid_step_solver on the GPU (include/vpt.h).  The criterion is equality of bits: a resident scene after a step
whose pressure is solved by multigrid against the host mirror (HostScene.fluid_step with a solver, held to float64 by
tests/test_fluid_mg_host.py), at every number of half-sweeps a smoothing launch can block.  The scene is test_fluid_host's."""
import numpy as np
import pytest

from test_filter_gpu import same_state
from test_fluid_gpu import SHAPES, voxels_of
from test_fluid_host import PARAMS, smoke_scene

pytestmark = pytest.mark.gpu
BLOCKS = (None, "2", "4")   # VPT_FLUID_MG_BLOCK: the default and each forced H
WHD = {None: (9, 17, 30)}   # the messy grid: three levels, odd halves on two axes


def block_of(monkeypatch, block, vpt_default):
    monkeypatch.setenv("VPT_FLUID_MG_BLOCK", block or "")   # an empty value asks for nothing
    return int(block or vpt_default)


def device_voxels(dev):
    return voxels_of(dev, lambda d, i: d.get_voxels(i))


@pytest.mark.parametrize("smooth", [1, 2])
@pytest.mark.parametrize("cycles", [0, 1, 3])
@pytest.mark.parametrize("open_faces", [0, 0b001000, 63], ids=["closed", "open+y", "open"])
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_a_multigrid_step_equals_the_mirror_at_every_block(vpt, monkeypatch, shape, open_faces, cycles, smooth):
    host = smoke_scene(vpt, shape)
    devices = [vpt.DeviceScene(host, 0) for _ in BLOCKS]
    before = voxels_of(host, lambda h, i: h.volume(i)[0])
    solver = vpt.FluidSolver(cycles=cycles, smooth=smooth, coarse_sweeps=3)
    host.fluid_step(vpt.FluidStep(0, (2, 3, 4), steps=1, iterations=1, open_faces=open_faces, **PARAMS), solver)
    [step] = host.update_fluid()
    want = voxels_of(host, lambda h, i: h.volume(i)[0])
    assert np.array_equal(want[1], before[1]) and np.array_equal(want[5], before[5]) and not np.array_equal(want[0], before[0])
    for block, dev in zip(BLOCKS, devices):
        h = block_of(monkeypatch, block, vpt.FLUID_DEFAULT_MG_BLOCK)
        dev.fluid_step(step)   # the ledger's step carries the solver
        launches, sent, ms = dev.update_stats()
        print(f"{shape} open {open_faces} cycles {cycles} smooth {smooth} H = {block}: {(launches, sent, ms)} (launches, bytes, device ms)", flush=True)
        assert (launches, sent) == (solver.launches(step, WHD.get(shape, shape), h), vpt.FLUID_RECORD_BYTES)
        got = device_voxels(dev)
        for i in range(6):
            assert np.array_equal(got[i], want[i]), f"H = {block}: {np.count_nonzero(got[i] != want[i])} voxels of volume {i} differ from the host mirror's"


@pytest.mark.parametrize("block", BLOCKS)
def test_two_steps_in_one_call_equal_two_calls_and_a_fresh_scene(vpt, monkeypatch, block):
    h = block_of(monkeypatch, block, vpt.FLUID_DEFAULT_MG_BLOCK)
    host = smoke_scene(vpt, (20, 9, 9))
    A, B = vpt.DeviceScene(host, 0), vpt.DeviceScene(host, 0)
    solver = vpt.FluidSolver(cycles=2, smooth=3, coarse_sweeps=16)
    step = vpt.FluidStep(0, (2, 3, 4), steps=2, open_faces=0b010010, **PARAMS)
    A.fluid_step(step, solver)
    assert A.update_stats()[:2] == (solver.launches(step, (20, 9, 9), h), 48) == (2 * (5 + 2 * (2 * (2 * {2: 3, 4: 2}[h] + 1) + 1)), 48)
    for _ in range(2):
        B.fluid_step(vpt.FluidStep(0, (2, 3, 4), steps=1, open_faces=0b010010, **PARAMS), solver)
    host.fluid_step(step, solver)
    assert host.update_fluid() == [vpt.FluidStep(0, (2, 3, 4), steps=2, open_faces=0b010010, **PARAMS, solver=solver)]   # the descriptor follows
    want = voxels_of(host, lambda s, i: s.volume(i)[0])
    for dev in (A, B, vpt.DeviceScene(host, 0)):
        assert all(np.array_equal(a, b) for a, b in zip(device_voxels(dev), want))
    A.fluid_step(vpt.FluidStep(0, (2, 3, 4), iterations=6, open_faces=8, **PARAMS), vpt.FluidSolver(kind=vpt.FLUID_JACOBI))   # the Jacobi, launch for launch
    B.fluid_step(vpt.FluidStep(0, (2, 3, 4), iterations=6, open_faces=8, **PARAMS))
    assert A.update_stats()[:2] == B.update_stats()[:2] and all(np.array_equal(a, b) for a, b in zip(device_voxels(A), device_voxels(B)))


def test_session_edit_fluid_with_a_solver_resets_and_a_refused_solver_leaves_it(vpt):
    host = smoke_scene(vpt)
    params = vpt.PathtraceParams(camera=0, resolution=48, shader="volgrid", samples=8, bounces=4)
    s = vpt.RenderSession(vpt.DeviceScene(host, 0), params)
    s.advance(2)
    host.fluid_step(vpt.FluidStep(0, (2, 3, 4), **PARAMS), vpt.FluidSolver(cycles=2))
    s.edit_fluid(host.update_fluid()[0])
    assert s.samples == 0
    s.advance(2)
    fresh = vpt.RenderSession(vpt.DeviceScene(host, 0), params)
    fresh.advance(2)
    assert same_state(s.state(), fresh.state())
    with pytest.raises(vpt.VptError, match="solver: smooth"):
        s.edit_fluid(vpt.FluidStep(0, (2, 3, 4)), vpt.FluidSolver(smooth=0))
    assert s.samples == 2 and same_state(s.state(), fresh.state())
    s.close(), fresh.close()
