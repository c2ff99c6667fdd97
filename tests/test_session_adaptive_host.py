"""Adaptive sampling in a render session (include/vpt.h: vpt_adaptive_run, vpt_session_set_adaptive), the part that
needs no GPU: the names the Python layer exposes, the sizes of the structures the C-ABI pins, the refusal of null arguments before a
device is looked for, and the command line's usage errors for --converge."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENE_03

BIN = os.path.join(ROOT, "volumetric-path-tracer_amd", "ypathtrace")


def test_the_python_layer_exposes_the_new_names(vpt):
    for name in ("set_adaptive", "progress", "converged", "hits", "noise", "adaptive_stats"):
        assert callable(getattr(vpt.RenderSession, name)), name
    for name in ("rounds", "progress", "noise_device", "stats_device", "close"):
        assert callable(getattr(vpt.AdaptiveRun, name)), name
    assert callable(vpt.DeviceScene.adaptive_run) and callable(vpt.box3_device)
    for name in ("vpt_adaptive_run_create", "vpt_adaptive_run_rounds", "vpt_adaptive_run_progress", "vpt_adaptive_run_noise_device",
                 "vpt_adaptive_run_stats_device", "vpt_adaptive_run_destroy", "vpt_box3_device", "vpt_session_set_adaptive",
                 "vpt_session_progress", "vpt_session_get_hits", "vpt_session_get_noise", "vpt_session_get_adaptive_stats"):
        assert getattr(vpt.hip, name).argtypes is not None, name


def test_the_pinned_structures_keep_their_sizes(vpt):
    assert C.sizeof(vpt.VptSessionParams) == 72 and C.sizeof(vpt.VptAdaptive) == 12


def test_every_new_entry_point_refuses_null_arguments_without_a_device(vpt):
    hip = vpt.hip
    a = np.zeros((6, 8), np.float32)
    b = np.zeros((6, 8), np.float32)
    p = a.ctypes.data
    params, ad, layout = vpt.PathtraceParams(resolution=8, samples=8).to_abi(), vpt.VptAdaptive(0.1, 4, 4), vpt.VptLayout(8, 6, 8, 8, 0, 1)
    out = C.c_void_p()
    assert hip.vpt_adaptive_run_create(None, C.byref(params), C.byref(ad), C.byref(layout), p, p, p, None, C.byref(out)) == -1
    assert hip.vpt_adaptive_run_create(None, C.byref(params), C.byref(ad), C.byref(layout), p, p, p, None, None) == -1
    assert out.value is None
    n, taken, active = C.c_int(7), C.c_int64(7), C.c_int(7)
    assert hip.vpt_adaptive_run_rounds(None, 1, C.byref(n), C.byref(taken), C.byref(active)) == -1
    assert (n.value, taken.value, active.value) == (0, 0, 0)
    assert hip.vpt_adaptive_run_progress(None, None, None, None, None) == -1
    assert hip.vpt_adaptive_run_noise_device(None, p, None, None) == -1
    assert hip.vpt_adaptive_run_stats_device(None, p, p, None) == -1
    hip.vpt_adaptive_run_destroy(None)   # like the other destroy calls: nothing to do
    assert hip.vpt_box3_device(8, 6, None, p, None) == -1 and "in" in hip.vpt_last_error().decode()
    assert hip.vpt_box3_device(8, 6, p, None, None) == -1 and "out" in hip.vpt_last_error().decode()
    assert hip.vpt_box3_device(8, 6, p, p, None) == -1 and "aliases" in hip.vpt_last_error().decode()
    assert hip.vpt_box3_device(0, 6, p, b.ctypes.data, None) == -1
    assert hip.vpt_session_set_adaptive(None, C.byref(ad)) == -1 and hip.vpt_session_set_adaptive(None, None) == -1
    assert hip.vpt_session_progress(None, None, None, None) == -1
    assert hip.vpt_session_get_hits(None, p) == -1
    assert hip.vpt_session_get_noise(None, p, p) == -1
    assert hip.vpt_session_get_adaptive_stats(None, p, p) == -1


def run(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("args,name", [
    (["--converge", "0.1"], "converge"), (["--progressive", "4", "--converge", "-1"], "converge"),
    (["--progressive", "4", "--converge", "nan"], "converge"), (["--progressive", "4", "--adaptive", "0.1"], "progressive"),
])
def test_cli_usage_errors_name_the_option(args, name):
    r = run("--scene", SCENE_03, *args)
    assert r.returncode == 1
    first = r.stderr.splitlines()[0]
    assert first.startswith("error: ") and name in first, r.stderr[:200]
    assert "usage: ypathtrace" in r.stderr   # a usage error, not a failure of the run


def test_cli_help_lists_converge():
    r = run("--help")
    assert r.returncode == 0 and "--converge" in r.stdout
