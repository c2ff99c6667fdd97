"""vpt_scene_fluid_step_detail on the GPU (include/vpt.h).  The criterion is equality of bits: a resident scene after a step
with vorticity confinement, MacCormack advection or both against the host mirror (HostScene.fluid_step with a detail, held to float64 by
tests/test_fluid_detail_host.py).  The scene is test_fluid_host's."""
import numpy as np
import pytest

from test_filter_gpu import same_state
from test_fluid_gpu import SHAPES, voxels_of
from test_fluid_host import PARAMS, smoke_scene

pytestmark = pytest.mark.gpu
DETAILS = {"maccormack": dict(advection=1, vorticity=0.0), "confine": dict(advection=0, vorticity=0.3), "both": dict(advection=1, vorticity=0.3)}
SOLVERS = {"jacobi": lambda vpt: None, "multigrid": lambda vpt: vpt.FluidSolver(cycles=1, smooth=1, coarse_sweeps=3)}
WHD = {None: (9, 17, 30)}


def device_voxels(dev):
    return voxels_of(dev, lambda d, i: d.get_voxels(i))


def host_voxels(host):
    return voxels_of(host, lambda h, i: h.volume(i)[0])


@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("open_faces", [0, 0b001000, 63], ids=["closed", "open+y", "open"])
@pytest.mark.parametrize("name", list(DETAILS))
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_a_detailed_step_equals_the_mirror(vpt, shape, name, open_faces, solver):
    host = smoke_scene(vpt, shape)
    dev, detail = vpt.DeviceScene(host, 0), vpt.FluidDetail(**DETAILS[name])
    before = host_voxels(host)
    host.fluid_step(vpt.FluidStep(0, (2, 3, 4), iterations=5, open_faces=open_faces, **PARAMS), SOLVERS[solver](vpt), detail)
    [step] = host.update_fluid()
    want = host_voxels(host)
    assert np.array_equal(want[1], before[1]) and np.array_equal(want[5], before[5]) and not np.array_equal(want[0], before[0])
    dev.fluid_step(step)   # the ledger's step carries the solver and the detail
    launches, sent, ms = dev.update_stats()
    print(f"{shape} {name} open {open_faces} {solver}: {(launches, sent, ms)} (launches, bytes, device ms)", flush=True)
    assert (launches, sent) == (detail.launches(step, WHD.get(shape, shape)), vpt.FLUID_RECORD_BYTES + vpt.FLUID_DETAIL_BYTES) and sent == step.payload_bytes()
    for i, got in enumerate(device_voxels(dev)):
        assert np.array_equal(got, want[i]), f"{np.count_nonzero(got != want[i])} voxels of volume {i} differ from the host mirror's"


@pytest.mark.parametrize("detail", [None, dict()], ids=["null", "off"])
def test_a_null_or_off_detail_is_the_step_launch_for_launch(vpt, detail):
    host = smoke_scene(vpt)
    A, B = vpt.DeviceScene(host, 0), vpt.DeviceScene(host, 0)
    step, solver = vpt.FluidStep(0, (2, 3, 4), steps=2, open_faces=8, **PARAMS), vpt.FluidSolver(cycles=1)
    A.fluid_step(step, solver)
    B.fluid_step(step, solver, detail if detail is None else vpt.FluidDetail(**detail))
    assert A.update_stats()[:2] == B.update_stats()[:2] == (solver.launches(step, (9, 17, 30)), 48)
    assert all(np.array_equal(a, b) for a, b in zip(device_voxels(A), device_voxels(B)))


@pytest.mark.parametrize("name", list(DETAILS))
def test_two_steps_in_one_call_equal_two_calls_and_a_fresh_scene(vpt, name):
    host = smoke_scene(vpt, (20, 9, 9))
    A, B = vpt.DeviceScene(host, 0), vpt.DeviceScene(host, 0)
    solver, detail = vpt.FluidSolver(cycles=1), vpt.FluidDetail(**DETAILS[name])
    step = vpt.FluidStep(0, (2, 3, 4), steps=2, open_faces=0b010010, **PARAMS)
    A.fluid_step(step, solver, detail)
    assert A.update_stats()[:2] == (detail.launches(step, (20, 9, 9), solver), 56)
    for _ in range(2):
        B.fluid_step(vpt.FluidStep(0, (2, 3, 4), steps=1, open_faces=0b010010, **PARAMS), solver, detail)
    host.fluid_step(step, solver, detail)
    assert host.update_fluid() == [vpt.FluidStep(0, (2, 3, 4), steps=2, open_faces=0b010010, **PARAMS, solver=solver, detail=detail)]
    want = host_voxels(host)
    for dev in (A, B, vpt.DeviceScene(host, 0)):
        assert all(np.array_equal(a, b) for a, b in zip(device_voxels(dev), want))


def test_session_edit_fluid_with_a_detail_resets_and_a_refused_detail_leaves_it(vpt):
    host = smoke_scene(vpt)
    params = vpt.PathtraceParams(camera=0, resolution=48, shader="volgrid", samples=8, bounces=4)
    s = vpt.RenderSession(vpt.DeviceScene(host, 0), params)
    s.advance(2)
    host.fluid_step(vpt.FluidStep(0, (2, 3, 4), **PARAMS), vpt.FluidSolver(cycles=2), vpt.FluidDetail(vpt.FLUID_MACCORMACK, 0.3))
    s.edit_fluid(host.update_fluid()[0])
    assert s.samples == 0
    s.advance(2)
    fresh = vpt.RenderSession(vpt.DeviceScene(host, 0), params)
    fresh.advance(2)
    assert same_state(s.state(), fresh.state())
    with pytest.raises(vpt.VptError, match="detail: advection"):
        s.edit_fluid(vpt.FluidStep(0, (2, 3, 4)), detail=vpt.FluidDetail(advection=-1))
    assert s.samples == 2 and same_state(s.state(), fresh.state())
    s.close(), fresh.close()
