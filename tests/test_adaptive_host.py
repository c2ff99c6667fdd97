"""Adaptive sampling without a GPU: ypathtrace's extension options (--adaptive, --adaptivemin, --adaptivestep) and their errors,
the C-ABI's refusal of bad vpt_adaptive values before any device call, the exported symbols, and get_render_hits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENE_03

BIN = os.path.join(ROOT, "volumetric-path-tracer_amd", "ypathtrace")


def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=600)


def test_help_lists_the_adaptive_options():
    r = run("--help")
    assert r.returncode == 0
    for line in ("--adaptive <float>", "--adaptivemin <integer>", "--adaptivestep <integer>"):
        assert line in r.stdout
    assert r.stdout.count("(extension)") >= 8


@pytest.mark.parametrize("args,message", [
    (["--adaptive", "-1"], "bad value for adaptive"),
    (["--adaptive", "nan"], "bad value for adaptive"),
    (["--adaptive", "inf"], "bad value for adaptive"),
    (["--adaptive", "0.1x"], "bad value for adaptive"),
    (["--adaptive"], "missing value for adaptive"),
    (["--adaptivestep", "0"], "bad value for adaptivestep"),
    (["--adaptivemin", "0"], "bad value for adaptivemin"),
    (["--adaptivemin", "64", "--samples", "32"], "bad value for adaptivemin"),
])
def test_bad_adaptive_values_exit_with_the_references_messages(args, message):
    r = run(*args)
    assert r.returncode == 1
    assert r.stderr.startswith("error: " + message), r.stderr[:200]


def test_adaptive_is_refused_on_several_gpus():
    r = run("--scene", SCENE_03, "--adaptive", "0.05", "--gpus", "2", "--output", os.devnull)
    assert r.returncode == 1
    assert "--adaptive" in r.stderr and "one GPU" in r.stderr, r.stderr[:200]


def test_symbols_are_exported(vpt):
    for name in ("vpt_render_adaptive", "vpt_render_device_adaptive", "vpt_resolve_hits_device"):
        getattr(vpt.hip, name)
    for name in ("get_render_hits", "resolve_hits_device"):
        assert callable(getattr(vpt, name))
    assert callable(vpt.DeviceScene.pathtrace_adaptive) and callable(vpt.DeviceScene.render_device_adaptive)


@pytest.mark.parametrize("threshold,min_samples,step,message", [
    (-1.0, 8, 4, "threshold"), (float("nan"), 8, 4, "threshold"), (float("inf"), 8, 4, "threshold"),
    (0.1, 0, 4, "min_samples"), (0.1, 65, 4, "min_samples"), (0.1, 8, 0, "step"), (0.1, 8, -3, "step"),
    (0.1, 8, 4, "null scene"),
])
def test_the_c_abi_refuses_bad_arguments_without_a_device(vpt, threshold, min_samples, step, message):
    params = vpt.PathtraceParams(resolution=16, samples=64, shader="volpathtrace").to_abi()
    ad = vpt.VptAdaptive(threshold, min_samples, step)
    image = np.zeros((8, 8, 4), np.float32)
    hits = np.zeros((8, 8), np.int32)
    rngs = np.zeros((8, 8, 2), np.uint64)
    samples, rendered, rounds = C.c_int(0), C.c_int64(0), C.c_int(0)
    rc = vpt.hip.vpt_render_adaptive(None, C.byref(params), C.byref(ad), 8, 8, image.ctypes.data, hits.ctypes.data, rngs.ctypes.data,
                                     C.byref(samples), C.byref(rendered))
    assert rc == -1 and message in vpt.hip.vpt_last_error().decode()
    layout = vpt.VptLayout(8, 8, 8, 8, 0, 1)
    rc = vpt.hip.vpt_render_device_adaptive(None, C.byref(params), C.byref(ad), C.byref(layout), None, None, None, None,
                                            C.byref(rounds), C.byref(rendered))
    assert rc == -1 and message in vpt.hip.vpt_last_error().decode()
    assert vpt.hip.vpt_resolve_hits_device(None, None, None, None, None) == -1


def test_get_render_hits_divides_each_pixel_by_its_own_count(vpt):
    rng = np.random.default_rng(3)
    st = vpt.PathtraceState(5, 3, 12, rng.random((3, 5, 4), dtype=np.float32) * 40, rng.integers(0, 40, (3, 5)).astype(np.int32),
                            np.zeros((3, 5, 2), np.uint64))
    st.hits[0, 0] = 0
    out = vpt.get_render_hits(st)
    assert out.dtype == np.float32 and out.shape == (3, 5, 4)
    for j in range(3):
        for i in range(5):
            h = st.hits[j, i]
            want = st.image[j, i] * (np.float32(1) / np.float32(h)) if h else np.zeros(4, np.float32)
            assert np.array_equal(out[j, i].view(np.uint32), want.astype(np.float32).view(np.uint32))
    # uniform hits: get_render's bits
    st.hits[:] = 12
    assert np.array_equal(vpt.get_render_hits(st).view(np.uint32), vpt.get_render(st).view(np.uint32))
