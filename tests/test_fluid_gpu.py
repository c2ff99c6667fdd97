"""vpt_scene_fluid_step on the GPU (include/vpt.h).  The criterion is equality of bits, no tolerance anywhere: a resident
scene after fluid_step(step) against the host mirror (HostScene.fluid_step, held to float64 by tests/test_fluid_host.py) and against a fresh
DeviceScene made from the stepped host scene, at every number of sweeps a Jacobi launch can block.  The scene is test_fluid_host's: the
density is volume 0 of 10_volgrid_synth's "messy", the velocity volumes 2, 3, 4; volumes 1 and 5 lie behind them in the pool."""
import numpy as np
import pytest

from test_filter_gpu import render, same_state
from test_fluid_host import PARAMS, REFUSALS, bits, smoke_scene

pytestmark = pytest.mark.gpu
BLOCKS = (None, "1", "2", "4")   # VPT_FLUID_BLOCK: the default and each forced K
SHAPES = [(1, 1, 1), (3, 5, 2), None, (20, 9, 9)]   # None: the messy 9 x 17 x 30 grid with its NaN and Inf voxels


def block_of(monkeypatch, block, vpt_default):
    """VPT_FLUID_BLOCK set or unset; the sweeps per launch it asks for"""
    monkeypatch.setenv("VPT_FLUID_BLOCK", block or "")   # an empty value asks for nothing
    return int(block or vpt_default)


def voxels_of(scene, get):
    return [bits(get(scene, i)) for i in range(6)]


@pytest.mark.parametrize("open_faces", [0, 0b001000, 63], ids=["closed", "open+y", "open"])
@pytest.mark.parametrize("iterations", [0, 1, 5, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_a_step_equals_the_mirror_at_every_block_and_a_fresh_scene(vpt, monkeypatch, shape, iterations, open_faces):
    host = smoke_scene(vpt, shape)
    devices = [vpt.DeviceScene(host, 0) for _ in BLOCKS]
    before = voxels_of(host, lambda h, i: h.volume(i)[0])
    host.fluid_step(vpt.FluidStep(0, (2, 3, 4), steps=1, iterations=iterations, open_faces=open_faces, **PARAMS))
    [step] = host.update_fluid()
    want = voxels_of(host, lambda h, i: h.volume(i)[0])
    assert np.array_equal(want[1], before[1]) and np.array_equal(want[5], before[5]) and not np.array_equal(want[0], before[0])
    for block, dev in zip(BLOCKS, devices):
        k = block_of(monkeypatch, block, vpt.FLUID_DEFAULT_BLOCK)
        dev.fluid_step(step)
        launches, sent, ms = dev.update_stats()
        print(f"{shape} N = {iterations} open {open_faces} K = {block}: {(launches, sent, ms)} (launches, bytes, device ms)", flush=True)
        assert (launches, sent) == (step.launches(k), vpt.FLUID_RECORD_BYTES) and sent == step.payload_bytes()
        got = voxels_of(dev, lambda d, i: d.get_voxels(i))
        for i in range(6):
            assert np.array_equal(got[i], want[i]), f"K = {block}: {np.count_nonzero(got[i] != want[i])} voxels of volume {i} differ from the host mirror's"
    assert all(np.array_equal(a, b) for a, b in zip(voxels_of(vpt.DeviceScene(host, 0), lambda d, i: d.get_voxels(i)), want))


@pytest.mark.parametrize("block", BLOCKS)
def test_three_steps_in_one_call_equal_three_calls_and_no_steps_launch_nothing(vpt, monkeypatch, block):
    k = block_of(monkeypatch, block, vpt.FLUID_DEFAULT_BLOCK)
    host = smoke_scene(vpt, (20, 9, 9))
    A, B = vpt.DeviceScene(host, 0), vpt.DeviceScene(host, 0)
    step = vpt.FluidStep(0, (2, 3, 4), steps=3, iterations=7, open_faces=0b010010, **PARAMS)
    A.fluid_step(step)
    assert A.update_stats()[:2] == (step.launches(k), 48) == (3 * (5 + {1: 7, 2: 4, 4: 3}[k]), 48)
    for _ in range(3):
        B.fluid_step(vpt.FluidStep(0, (2, 3, 4), steps=1, iterations=7, open_faces=0b010010, **PARAMS))
    host.fluid_step(step)
    want = voxels_of(host, lambda h, i: h.volume(i)[0])
    for dev in (A, B):
        assert all(np.array_equal(a, b) for a, b in zip(voxels_of(dev, lambda d, i: d.get_voxels(i)), want))
    idle = vpt.FluidStep(0, (2, 3, 4), steps=0, iterations=7)
    B.fluid_step(idle)
    assert B.update_stats()[:2] == (0, 0) == (idle.launches(k), idle.payload_bytes())


def test_volgrid_majorants_and_renders_follow_a_step(vpt):
    host = smoke_scene(vpt)
    A = vpt.DeviceScene(host, 0)
    first = render(vpt, host, A)   # the brick tables exist before the step: they have to be made anew
    builds = A.volgrid_stats()["table_builds"]
    host.fluid_step(vpt.FluidStep(0, (2, 3, 4), steps=2, iterations=6, open_faces=0b001000, **PARAMS))
    for step in host.update_fluid():
        A.fluid_step(step)
    assert np.array_equal(bits(A.volgrid_majorants(0)), bits(host.volgrid_majorants(0))) and A.volgrid_stats()["table_builds"] == builds + 1
    after = render(vpt, host, A)
    assert same_state(after, render(vpt, host, vpt.DeviceScene(host, 0))) and not same_state(after, first)


def test_session_edit_fluid_resets_and_a_refused_edit_leaves_it(vpt):
    host = smoke_scene(vpt)
    params = vpt.PathtraceParams(camera=0, resolution=48, shader="volgrid", samples=8, bounces=4)
    s = vpt.RenderSession(vpt.DeviceScene(host, 0), params)
    s.advance(2)
    host.fluid_step(vpt.FluidStep(0, (2, 3, 4), iterations=4, **PARAMS))
    s.edit_fluid(host.update_fluid()[0])
    assert s.samples == 0
    s.advance(2)
    fresh = vpt.RenderSession(vpt.DeviceScene(host, 0), params)
    fresh.advance(2)
    assert same_state(s.state(), fresh.state())
    for changed, named in REFUSALS.values():
        with pytest.raises(vpt.VptError, match=named):
            s.edit_fluid(vpt.FluidStep(**{**dict(density=0, velocity=(2, 3, 4)), **changed}))
        assert s.samples == 2
    assert same_state(s.state(), fresh.state())
    s.close(), fresh.close()
