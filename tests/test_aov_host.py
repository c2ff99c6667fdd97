"""What the first-hit pass checks before it looks for a device (include/vpt.h: vpt_render_aov and its neighbours): every refusal is
VPT_ERR_INVALID_ARG with a message that names the argument, the scene handle is looked at last, and nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest

W, H = 16, 8


@pytest.fixture()
def call(vpt):
    """vpt_render_aov with good arguments but for the ones overridden; returns (code, message)"""
    planes = {n: np.zeros((H, W, 2 if n == "ids" else 3 if n == "uvt" else 4), np.int32 if n == "ids" else np.float32) for n in vpt.AOV_PLANES}
    hits, rng = np.zeros((H, W), np.int32), np.zeros((H, W, 2), np.uint64)

    def run(**over):
        given = over.pop("planes", tuple(vpt.AOV_PLANES))
        pl = None if given is None else C.byref(vpt.VptAovPlanes(**{n: planes[n].ctypes.data for n in given}))
        a = dict(scene=None, nsamples=1, width=W, height=H, hits=hits.ctypes.data, rng=rng.ctypes.data, samples_io=C.byref(C.c_int(0)),
                 params=C.byref(vpt.PathtraceParams(resolution=W, samples=4, shader="normal").to_abi()))
        a.update(over)
        rc = vpt.hip.vpt_render_aov(a["scene"], a["params"], a["nsamples"], a["width"], a["height"], pl, a["hits"], a["rng"], a["samples_io"])
        return rc, vpt.hip.vpt_last_error().decode()
    return run


def test_the_abi_structs_have_the_headers_layout(vpt):
    assert C.sizeof(vpt.VptAovPlanes) == 6 * C.sizeof(C.c_void_p) and [f[0] for f in vpt.VptAovPlanes._fields_] == list(vpt.AOV_PLANES)
    assert C.sizeof(vpt.VptPick) == 32
    assert vpt.AOV_PLANES == ("normal", "albedo", "texcoord", "depth", "ids", "uvt")


@pytest.mark.parametrize("over,word", [
    (dict(planes=None), "planes"),
    (dict(planes=()), "every plane is null"),
    (dict(planes=("uvt",)), "uvt is given without ids"),
    (dict(planes=("normal", "uvt")), "uvt is given without ids"),
    (dict(width=0), "width"),
    (dict(height=-3), "height"),
    (dict(width=40000), "width"),
    (dict(hits=None), "hits"),
    (dict(rng=None), "rng"),
    (dict(samples_io=None), "samples_io"),
    (dict(params=None), "params"),
    (dict(nsamples=-1), "nsamples"),
    (dict(), "scene"),   # everything else is in order: the null scene is what is left to refuse
])
def test_render_aov_checks_its_arguments_before_looking_for_a_device(call, over, word):
    rc, message = call(**over)
    assert rc == -1 and word in message, (rc, message)


def test_a_single_plane_and_ids_alone_pass_the_plane_checks(call):
    for planes in (("depth",), ("ids",), ("ids", "uvt")):
        rc, message = call(planes=planes)
        assert rc == -1 and "scene" in message, (planes, message)


def test_two_planes_in_one_buffer_are_refused(vpt):
    buf = np.zeros((H, W, 4), np.float32)
    hits, rng = np.zeros((H, W), np.int32), np.zeros((H, W, 2), np.uint64)
    pl = vpt.VptAovPlanes(normal=buf.ctypes.data, depth=buf.ctypes.data)
    abi = vpt.PathtraceParams(resolution=W, samples=4).to_abi()
    rc = vpt.hip.vpt_render_aov(None, C.byref(abi), 1, W, H, C.byref(pl), hits.ctypes.data, rng.ctypes.data, C.byref(C.c_int(0)))
    assert rc == -1 and "normal and depth share a buffer" in vpt.hip.vpt_last_error().decode()


def test_the_device_entry_points_refuse_null_arguments(vpt):
    lay = vpt.VptLayout(W, H, 8, 8, 0, 1)
    abi = vpt.PathtraceParams(resolution=W).to_abi()
    assert vpt.hip.vpt_render_aov_device(None, C.byref(abi), C.byref(lay), 1, None, None, None, None) == -1
    assert "planes" in vpt.hip.vpt_last_error().decode()
    empty = vpt.VptAovPlanes()
    assert vpt.hip.vpt_render_aov_device(None, C.byref(abi), C.byref(lay), 1, C.byref(empty), None, None, None) == -1
    assert "every plane is null" in vpt.hip.vpt_last_error().decode()
    assert vpt.hip.vpt_resolve_ids_device(None, None, None, None, None, None) == -1
    assert vpt.hip.vpt_session_pick(None, 0, 0, None) == -1
    assert vpt.hip.vpt_session_get_ids(None, None, None) == -1
    assert vpt.hip.vpt_session_get_guides(None, None, None) == -1


def test_the_python_wrappers_name_an_unknown_plane(vpt):
    st = vpt.PathtraceState(W, H, 0, np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.int32), np.zeros((H, W, 2), np.uint64))
    with pytest.raises(vpt.VptError, match="unknown AOV plane 'colour'"):
        vpt.DeviceScene.render_aovs(None, st, vpt.PathtraceParams(resolution=W), 1, planes=("normal", "colour"))
