"""What the sphere-traced first-hit pass checks before it looks for a device (include/vpt.h: vpt_render_sdf_aov and its neighbours): every
refusal is VPT_ERR_INVALID_ARG with a message that names the argument, the scene handle is looked at last, and nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest

W, H = 16, 8


def _arrays(vpt):
    planes = {n: np.zeros((H, W, 2 if n == "ids" else 4), np.int32 if n == "ids" else np.float32) for n in vpt.SDF_AOV_PLANES}
    return planes, np.zeros((H, W), np.int32), np.zeros((H, W, 2), np.uint64)


@pytest.fixture()
def call(vpt):
    """vpt_render_sdf_aov with good arguments but for the ones overridden; returns (code, message)"""
    planes, hits, rng = _arrays(vpt)

    def run(**over):
        given = over.pop("planes", tuple(vpt.SDF_AOV_PLANES))
        pl = None if given is None else C.byref(vpt.VptSdfAovPlanes(**{n: planes[n].ctypes.data for n in given}))
        params = vpt.PathtraceParams(resolution=W, samples=4, shader="implicit_normal", spheretrace_maxiter=over.pop("maxiter", 450))
        a = dict(scene=None, nsamples=1, width=W, height=H, hits=hits.ctypes.data, rng=rng.ctypes.data, samples_io=C.byref(C.c_int(0)),
                 params=C.byref(params.to_abi()))
        a.update(over)
        rc = vpt.hip.vpt_render_sdf_aov(a["scene"], a["params"], a["nsamples"], a["width"], a["height"], pl, a["hits"], a["rng"], a["samples_io"])
        return rc, vpt.hip.vpt_last_error().decode()
    return run


@pytest.fixture()
def device_call(vpt):
    """vpt_render_sdf_aov_device in the same way (the pointers are never followed: the null scene is refused last)"""
    planes, hits, rng = _arrays(vpt)

    def run(**over):
        given = over.pop("planes", tuple(vpt.SDF_AOV_PLANES))
        pl = None if given is None else C.byref(vpt.VptSdfAovPlanes(**{n: planes[n].ctypes.data for n in given}))
        params = vpt.PathtraceParams(resolution=W, samples=4, shader="implicit_normal", spheretrace_maxiter=over.pop("maxiter", 450))
        a = dict(scene=None, nsamples=1, layout=C.byref(vpt.VptLayout(W, H, 8, 8, 0, 1)), hits=hits.ctypes.data, rng=rng.ctypes.data,
                 params=C.byref(params.to_abi()))
        a.update(over)
        rc = vpt.hip.vpt_render_sdf_aov_device(a["scene"], a["params"], a["layout"], a["nsamples"], pl, a["hits"], a["rng"], None)
        return rc, vpt.hip.vpt_last_error().decode()
    return run


def test_the_abi_structs_have_the_headers_layout(vpt):
    assert C.sizeof(vpt.VptSdfAovPlanes) == 5 * C.sizeof(C.c_void_p)
    assert [f[0] for f in vpt.VptSdfAovPlanes._fields_] == list(vpt.SDF_AOV_PLANES)
    assert C.sizeof(vpt.VptSdfPick) == 48
    assert [f[0] for f in vpt.VptSdfPick._fields_] == ["hit", "vol_instance", "sdf", "volume", "material", "distance", "position", "normal"]
    assert vpt.SDF_AOV_PLANES == ("normal", "albedo", "depth", "ids", "hit")
    # the mesh pass's structs are other structs and stay as they are
    assert C.sizeof(vpt.VptAovPlanes) == 6 * C.sizeof(C.c_void_p) and C.sizeof(vpt.VptPick) == 32


REFUSALS = [
    (dict(planes=None), "planes"),
    (dict(planes=()), "every plane is null"),
    (dict(planes=("hit",)), "hit is given without ids"),
    (dict(planes=("normal", "hit")), "hit is given without ids"),
    (dict(hits=None), "hits"),
    (dict(rng=None), "rng"),
    (dict(params=None), "params"),
    (dict(nsamples=-1), "nsamples"),
    (dict(maxiter=-1), "spheretrace_maxiter"),
    (dict(maxiter=(1 << 20) + 1), "spheretrace_maxiter"),
    (dict(), "scene"),   # everything else is in order: the null scene is what is left to refuse
    (dict(maxiter=0), "scene"),   # both ends of the range are inside it
    (dict(maxiter=1 << 20), "scene"),
]


@pytest.mark.parametrize("over,word", REFUSALS + [
    (dict(width=0), "width"),
    (dict(height=-3), "height"),
    (dict(width=40000), "width"),
    (dict(samples_io=None), "samples_io"),
])
def test_render_sdf_aov_checks_its_arguments_before_looking_for_a_device(call, over, word):
    rc, message = call(**over)
    assert rc == -1 and word in message, (rc, message)


@pytest.mark.parametrize("over,word", REFUSALS + [(dict(layout=None), "layout")])
def test_render_sdf_aov_device_checks_its_arguments_and_the_scene_last(device_call, over, word):
    rc, message = device_call(**over)
    assert rc == -1 and word in message, (rc, message)


def test_a_single_plane_and_ids_alone_pass_the_plane_checks(call, device_call):
    for planes in (("depth",), ("albedo",), ("ids",), ("ids", "hit")):
        for run in (call, device_call):
            rc, message = run(planes=planes)
            assert rc == -1 and "scene" in message, (planes, message)


@pytest.mark.parametrize("a,b", [("normal", "depth"), ("albedo", "hit"), ("normal", "albedo")])
def test_two_planes_in_one_buffer_are_refused(vpt, a, b):
    buf = np.zeros((H, W, 4), np.float32)
    ids = np.zeros((H, W, 2), np.int32)
    hits, rng = np.zeros((H, W), np.int32), np.zeros((H, W, 2), np.uint64)
    pl = vpt.VptSdfAovPlanes(**{a: buf.ctypes.data, b: buf.ctypes.data, "ids": ids.ctypes.data})
    abi = vpt.PathtraceParams(resolution=W, samples=4).to_abi()
    lay = vpt.VptLayout(W, H, 8, 8, 0, 1)
    rc = vpt.hip.vpt_render_sdf_aov(None, C.byref(abi), 1, W, H, C.byref(pl), hits.ctypes.data, rng.ctypes.data, C.byref(C.c_int(0)))
    assert rc == -1 and f"{a} and {b} share a buffer" in vpt.hip.vpt_last_error().decode()
    rc = vpt.hip.vpt_render_sdf_aov_device(None, C.byref(abi), C.byref(lay), 1, C.byref(pl), hits.ctypes.data, rng.ctypes.data, None)
    assert rc == -1 and f"{a} and {b} share a buffer" in vpt.hip.vpt_last_error().decode()


def test_the_resolve_and_the_session_entry_points_refuse_null_arguments(vpt):
    lay = vpt.VptLayout(W, H, 8, 8, 0, 1)
    ids = np.zeros((H, W, 2), np.int32)
    assert vpt.hip.vpt_resolve_sdf_ids_device(None, None, None, None, None, None) == -1
    assert vpt.hip.vpt_resolve_sdf_ids_device(C.byref(lay), ids.ctypes.data, ids.ctypes.data, ids.ctypes.data, None, None) == -1
    assert "null together" in vpt.hip.vpt_last_error().decode()
    out = vpt.VptSdfPick()
    assert vpt.hip.vpt_session_pick_sdf(None, 0, 0, C.byref(out)) == -1
    assert vpt.hip.vpt_session_pick_sdf(None, 0, 0, None) == -1
    assert vpt.hip.vpt_session_get_sdf_ids(None, ids.ctypes.data, None) == -1 and "session" in vpt.hip.vpt_last_error().decode()


def test_the_python_wrappers_name_an_unknown_plane(vpt):
    st = vpt.PathtraceState(W, H, 0, np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.int32), np.zeros((H, W, 2), np.uint64))
    with pytest.raises(vpt.VptError, match="unknown SDF AOV plane 'texcoord'"):
        vpt.DeviceScene.render_sdf_aovs(None, st, vpt.PathtraceParams(resolution=W), 1, planes=("normal", "texcoord"))
    with pytest.raises(vpt.VptError, match="unknown SDF AOV plane 'uvt'"):
        vpt.DeviceScene.render_sdf_aov_device(None, vpt.PathtraceParams(resolution=W), vpt.VptLayout(W, H, 8, 8, 0, 1), 1, {"uvt": 1}, 0, 0)
