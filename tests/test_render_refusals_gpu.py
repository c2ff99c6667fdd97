"""The single-fault refusals of the render-side entry points (include/vpt.h, include/vpt_kat.h): vpt_render_device, vpt_render, the
adaptive entry points, the two read-backs of a launch, vpt_intersect, vpt_kat and the light-CDF self-test.  Every call below has exactly
one thing wrong; the (code, message) pairs are written out as the library's source states them.  Raw calls on one tiny resident scene
(synth_scenes.chain_scene: two instances, one camera, the environment as its only light, no texture, volume or SDF), a 16 x 8 frame,
device buffers from torch.  Nothing is rendered except where a refusal can only come after a launch (the device's own look at hits[]).
The refusals of the first-hit passes are pinned by test_aov_host.py, test_aov_gpu.py and test_sdf_aov_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import synth_scenes

pytestmark = pytest.mark.gpu

W, H = 16, 8
INVALID, UNKNOWN_SHADER = -1, -4   # VPT_ERR_INVALID_ARG, VPT_ERR_UNKNOWN_SHADER
KAT = dict(LOBES=0, TEXTURE=2, CAMERA=3, INTERSECT=4, SURFACE=5, SDF_NORMAL=11, SPHERETRACE=12, VOLUME=13, SDF_FUNCTION=14, OP_COUNT=15)
KAT_IN = {0: 19, 2: 4, 3: 5, 4: 7, 5: 7, 11: 6, 12: 7, 13: 4, 14: 4}   # floats per input record (include/vpt_kat.h)


@pytest.fixture(scope="module")
def host(vpt, tmp_path_factory):
    path, facts = synth_scenes.chain_scene(tmp_path_factory.mktemp("refusals"), depth=6)
    assert facts["instances"] == 2
    return vpt.HostScene(path)


@pytest.fixture(scope="module")
def dev(vpt, host):
    if vpt.device_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible (the HIP path has no CPU fallback)")
    return vpt.DeviceScene(host, 0)


class Frame:
    """a 16 x 8 state on the device (one rank, 8 x 8 tiles: 128 slots) and the same on the host"""

    def __init__(self, vpt):
        import torch
        self.layout = vpt.VptLayout(W, H, 8, 8, 0, 1)
        slots = vpt.layout_slots(self.layout)
        self.image = torch.zeros((slots, 4), dtype=torch.float32, device="cuda")
        self.hits = torch.zeros((slots,), dtype=torch.int32, device="cuda")
        self.rng = torch.zeros((slots, 2), dtype=torch.int64, device="cuda")
        vpt.state_init_device(self.layout, self.image.data_ptr(), self.hits.data_ptr(), self.rng.data_ptr())
        torch.cuda.synchronize()
        self.h_image, self.h_hits = np.full((H, W, 4), 0.25, np.float32), np.zeros((H, W), np.int32)
        self.h_rng = np.arange(H * W * 2, dtype=np.uint64).reshape(H, W, 2)

    def device_bytes(self):
        import torch
        torch.cuda.synchronize()
        return [t.cpu().numpy().tobytes() for t in (self.image, self.hits, self.rng)]

    def host_bytes(self):
        return [a.tobytes() for a in (self.h_image, self.h_hits, self.h_rng)]


@pytest.fixture()
def frame(vpt):
    return Frame(vpt)


def params_abi(vpt, **over):
    p = vpt.PathtraceParams(resolution=W, samples=4, shader="eyelight", bounces=2).to_abi()
    for k, v in over.items():
        setattr(p, k, v)
    return p


def outcome(vpt, rc):
    return rc, vpt.hip.vpt_last_error().decode()


# ---- vpt_render_device -----------------------------------------------------------------------------------------------------------
def render_device(vpt, dev, frame, nsamples=1, **over):
    a = dict(scene=dev.handle, params=C.byref(params_abi(vpt, **over.pop("p", {}))), layout=C.byref(frame.layout), image=frame.image.data_ptr(),
             hits=frame.hits.data_ptr(), rng=frame.rng.data_ptr())
    a.update(over)
    return outcome(vpt, vpt.hip.vpt_render_device(a["scene"], a["params"], a["layout"], nsamples, a["image"], a["hits"], a["rng"], None))


@pytest.mark.parametrize("over,nsamples,expected", [
    (dict(scene=None), 1, (INVALID, "null argument")),
    (dict(params=None), 1, (INVALID, "null argument")),
    (dict(layout=None), 1, (INVALID, "null argument")),
    (dict(image=None), 1, (INVALID, "null argument")),
    (dict(hits=None), 1, (INVALID, "null argument")),
    (dict(rng=None), 1, (INVALID, "null argument")),
    (dict(p=dict(shader=-1)), 1, (UNKNOWN_SHADER, "sampler unknown")),
    (dict(p=dict(shader=9)), 1, (UNKNOWN_SHADER, "sampler unknown")),   # one past VPT_SHADER_IMPLICIT_NORMAL
    (dict(p=dict(camera=-1)), 1, (INVALID, "camera -1 out of range")),
    (dict(p=dict(camera=1)), 1, (INVALID, "camera 1 out of range")),   # num_cameras
    (dict(), -1, (INVALID, "negative sample/bounce count")),
    (dict(p=dict(bounces=-1)), 1, (INVALID, "negative sample/bounce count")),
])
def test_render_device_refusals(vpt, dev, frame, over, nsamples, expected):
    before = frame.device_bytes()
    assert render_device(vpt, dev, frame, nsamples, **over) == expected
    assert frame.device_bytes() == before


def test_render_device_of_no_samples_is_a_no_op(vpt, dev, frame):
    before = frame.device_bytes()
    assert render_device(vpt, dev, frame, 0)[0] == 0
    assert frame.device_bytes() == before


# ---- vpt_render ------------------------------------------------------------------------------------------------------------------
def render(vpt, dev, frame, reached=0, **over):
    io = C.c_int(reached)
    a = dict(scene=dev.handle, params=C.byref(params_abi(vpt, **over.pop("p", {}))), width=W, height=H, image=frame.h_image.ctypes.data,
             hits=frame.h_hits.ctypes.data, rng=frame.h_rng.ctypes.data, samples_io=C.byref(io))
    a.update(over)
    rc = vpt.hip.vpt_render(a["scene"], a["params"], 1, a["width"], a["height"], a["image"], a["hits"], a["rng"], a["samples_io"])
    return outcome(vpt, rc), io.value


@pytest.mark.parametrize("over,expected", [
    (dict(scene=None), (INVALID, "null argument")),
    (dict(params=None), (INVALID, "null argument")),
    (dict(image=None), (INVALID, "null argument")),
    (dict(hits=None), (INVALID, "null argument")),
    (dict(rng=None), (INVALID, "null argument")),
    (dict(samples_io=None), (INVALID, "null argument")),
    (dict(width=0), (INVALID, "bad image size")),
    (dict(height=0), (INVALID, "bad image size")),
    (dict(p=dict(shader=-1)), (UNKNOWN_SHADER, "sampler unknown")),
    (dict(p=dict(shader=9)), (UNKNOWN_SHADER, "sampler unknown")),
])
def test_render_refusals(vpt, dev, frame, over, expected):
    before = frame.host_bytes()
    got, io = render(vpt, dev, frame, **over)
    assert got == expected and io == 0
    assert frame.host_bytes() == before


def test_render_is_a_no_op_once_the_samples_are_reached(vpt, dev, frame):
    before = frame.host_bytes()
    got, io = render(vpt, dev, frame, reached=4)   # params->samples
    assert got[0] == 0 and io == 4
    assert frame.host_bytes() == before


# ---- vpt_render_adaptive, vpt_adaptive_run_create ----------------------------------------------------------------------------------
def adaptive_abi(vpt, **over):
    a = vpt.VptAdaptive(0.05, 2, 1)   # threshold, min_samples, step
    for k, v in over.items():
        setattr(a, k, v)
    return a


def run_create(vpt, dev, frame, **over):
    out = C.c_void_p()
    a = dict(scene=dev.handle, params=C.byref(params_abi(vpt, **over.pop("p", {}))), adaptive=C.byref(adaptive_abi(vpt, **over.pop("a", {}))),
             layout=C.byref(frame.layout), image=frame.image.data_ptr(), hits=frame.hits.data_ptr(), rng=frame.rng.data_ptr(), out=C.byref(out))
    a.update(over)
    rc = vpt.hip.vpt_adaptive_run_create(a["scene"], a["params"], a["adaptive"], a["layout"], a["image"], a["hits"], a["rng"], None, a["out"])
    got = outcome(vpt, rc)
    if out.value:
        vpt.hip.vpt_adaptive_run_destroy(out)
    return got, bool(out.value)


def render_adaptive(vpt, dev, frame, **over):
    io, rendered = C.c_int(-7), C.c_int64(-7)
    a = dict(scene=dev.handle, params=C.byref(params_abi(vpt, **over.pop("p", {}))), adaptive=C.byref(adaptive_abi(vpt, **over.pop("a", {}))),
             width=W, height=H, image=frame.h_image.ctypes.data, hits=frame.h_hits.ctypes.data, rng=frame.h_rng.ctypes.data,
             samples_io=C.byref(io))
    a.update(over)
    rc = vpt.hip.vpt_render_adaptive(a["scene"], a["params"], a["adaptive"], a["width"], a["height"], a["image"], a["hits"], a["rng"],
                                     a["samples_io"], C.byref(rendered))
    return outcome(vpt, rc), rendered.value


ADAPTIVE_BOTH = [   # what check_adaptive refuses, in its order: the same for both entry points
    (dict(params=None), (INVALID, "null argument")),
    (dict(adaptive=None), (INVALID, "null argument")),
    (dict(a=dict(threshold=float("nan"))), (INVALID, "adaptive threshold must be finite and >= 0")),
    (dict(a=dict(threshold=-0.5)), (INVALID, "adaptive threshold must be finite and >= 0")),
    (dict(a=dict(step=0)), (INVALID, "adaptive step must be >= 1")),
    (dict(p=dict(samples=0)), (INVALID, "params->samples (the per-pixel cap) must be >= 1")),
    (dict(a=dict(min_samples=0)), (INVALID, "adaptive min_samples must be in 1 .. params->samples (4)")),
    (dict(a=dict(min_samples=5)), (INVALID, "adaptive min_samples must be in 1 .. params->samples (4)")),   # samples + 1
    (dict(p=dict(bounces=-1)), (INVALID, "negative bounce count")),
    (dict(scene=None), (INVALID, "null scene")),
    (dict(p=dict(shader=-1)), (UNKNOWN_SHADER, "sampler unknown")),
    (dict(p=dict(shader=9)), (UNKNOWN_SHADER, "sampler unknown")),
    (dict(p=dict(camera=-1)), (INVALID, "camera -1 out of range")),
    (dict(p=dict(camera=1)), (INVALID, "camera 1 out of range")),
]


@pytest.mark.parametrize("over,expected", ADAPTIVE_BOTH + [
    (dict(out=None), (INVALID, "null argument")),
    (dict(layout=None), (INVALID, "null argument")),
    (dict(image=None), (INVALID, "null argument")),
    (dict(hits=None), (INVALID, "null argument")),
    (dict(rng=None), (INVALID, "null argument")),
    (dict(layout="w0"), (INVALID, "bad layout")),
    (dict(layout="h0"), (INVALID, "bad layout")),
])
def test_adaptive_run_create_refusals(vpt, dev, frame, over, expected):
    over = {k: (dict(v) if isinstance(v, dict) else v) for k, v in over.items()}
    if isinstance(over.get("layout"), str):
        over["layout"] = C.byref(vpt.VptLayout(0, H, 8, 8, 0, 1) if over["layout"] == "w0" else vpt.VptLayout(W, 0, 8, 8, 0, 1))
    before = frame.device_bytes()
    got, made = run_create(vpt, dev, frame, **over)
    assert got == expected and not made
    assert frame.device_bytes() == before


@pytest.mark.parametrize("over,expected", ADAPTIVE_BOTH + [
    (dict(image=None), (INVALID, "null argument")),
    (dict(hits=None), (INVALID, "null argument")),
    (dict(rng=None), (INVALID, "null argument")),
    (dict(samples_io=None), (INVALID, "null argument")),
    (dict(width=0), (INVALID, "bad image size")),
    (dict(height=0), (INVALID, "bad image size")),
])
def test_render_adaptive_refusals(vpt, dev, frame, over, expected):
    over = {k: (dict(v) if isinstance(v, dict) else v) for k, v in over.items()}
    before = frame.host_bytes()
    got, rendered = render_adaptive(vpt, dev, frame, **over)
    assert got == expected and rendered == 0
    assert frame.host_bytes() == before


def test_unequal_hits_are_refused_by_the_host_with_the_pixel_and_by_the_device_with_the_range(vpt, dev, frame):
    frame.h_hits[0, 5] = 1
    got, rendered = render_adaptive(vpt, dev, frame)
    assert got == (INVALID, "hits[] must be equal on entry (pixel 5 has 1, pixel 0 0)") and rendered == 0
    frame.hits[5] = 1   # a slot that owns a pixel: 16 x 8 in 8 x 8 tiles has no padding
    got, made = run_create(vpt, dev, frame)
    assert got == (INVALID, "hits[] must be equal on entry (found 0 .. 1)") and not made


def test_adaptive_run_rounds_refusals(vpt, dev, frame):
    done, rendered, active = C.c_int(-7), C.c_int64(-7), C.c_int(-7)
    rc = vpt.hip.vpt_adaptive_run_rounds(None, 1, C.byref(done), C.byref(rendered), C.byref(active))
    assert outcome(vpt, rc) == (INVALID, "null run") and (done.value, rendered.value, active.value) == (0, 0, 0)
    out = C.c_void_p()
    p, a = params_abi(vpt), adaptive_abi(vpt)
    assert vpt.hip.vpt_adaptive_run_create(dev.handle, C.byref(p), C.byref(a), C.byref(frame.layout), frame.image.data_ptr(), frame.hits.data_ptr(),
                                           frame.rng.data_ptr(), None, C.byref(out)) == 0
    try:
        before = frame.device_bytes()
        done, rendered, active = C.c_int(-7), C.c_int64(-7), C.c_int(-7)
        rc = vpt.hip.vpt_adaptive_run_rounds(out, -1, C.byref(done), C.byref(rendered), C.byref(active))
        assert outcome(vpt, rc) == (INVALID, "negative round count") and (done.value, rendered.value, active.value) == (0, 0, 0)
        assert frame.device_bytes() == before
    finally:
        vpt.hip.vpt_adaptive_run_destroy(out)


# ---- the read-backs of a launch --------------------------------------------------------------------------------------------------
def test_a_fresh_handle_has_no_launch_to_report(vpt, host):
    fresh = vpt.DeviceScene(host, 0)
    ms, count = C.c_float(-1), C.c_int(-1)
    assert outcome(vpt, vpt.hip.vpt_last_kernel_ms(fresh.handle, C.byref(ms))) == (INVALID, "no launch recorded")
    assert outcome(vpt, vpt.hip.vpt_last_wave_costs(fresh.handle, None, 0, C.byref(count))) == (INVALID, "no launch recorded")
    assert outcome(vpt, vpt.hip.vpt_last_kernel_ms(None, C.byref(ms))) == (INVALID, "null argument")
    assert outcome(vpt, vpt.hip.vpt_last_kernel_ms(fresh.handle, None)) == (INVALID, "null argument")
    assert outcome(vpt, vpt.hip.vpt_last_wave_costs(None, None, 0, C.byref(count))) == (INVALID, "bad argument")
    assert outcome(vpt, vpt.hip.vpt_last_wave_costs(fresh.handle, None, 0, None)) == (INVALID, "bad argument")
    assert outcome(vpt, vpt.hip.vpt_last_wave_costs(fresh.handle, None, -1, C.byref(count))) == (INVALID, "bad argument")
    assert outcome(vpt, vpt.hip.vpt_last_wave_costs(fresh.handle, None, 4, C.byref(count))) == (INVALID, "bad argument")
    fresh.close()


# ---- vpt_intersect -----------------------------------------------------------------------------------------------------------------
def test_intersect_refusals(vpt, dev):
    rays = np.array([[0, 0, 5, 0, 0, -1]], np.float32)
    ids, uvt = np.full((1, 2), -7, np.int32), np.full((1, 3), -7, np.float32)
    r, i, u = rays.ctypes.data, ids.ctypes.data, uvt.ctypes.data
    call = lambda *a: outcome(vpt, vpt.hip.vpt_intersect(*a))   # noqa: E731
    assert call(None, 1, r, -1, i, u) == (INVALID, "bad argument")
    assert call(dev.handle, 1, None, -1, i, u) == (INVALID, "bad argument")
    assert call(dev.handle, 1, r, -1, None, u) == (INVALID, "bad argument")
    assert call(dev.handle, 1, r, -1, i, None) == (INVALID, "bad argument")
    assert call(dev.handle, -1, r, -1, i, u) == (INVALID, "bad argument")
    assert call(dev.handle, 1, r, 2, i, u) == (INVALID, "instance 2 out of range")   # num_instances
    assert call(dev.handle, 1, r, -2, i, u) == (INVALID, "instance -2 out of range")
    assert call(dev.handle, 0, r, -1, i, u)[0] == 0
    assert np.all(ids == -7) and np.all(uvt == -7)


# ---- vpt_kat, vpt_kat_strides --------------------------------------------------------------------------------------------------------
def kat(vpt, dev, op, records, iparam=0):
    records = np.ascontiguousarray(records, np.float32)
    out = np.full((max(len(records), 1), 32), -7, np.float32)
    rc = vpt.hip.vpt_kat(dev.handle, op, iparam, len(records), records.ctypes.data, out.ctypes.data)
    return outcome(vpt, rc), out


def test_kat_strides_refusals(vpt):
    a, b = C.c_int(-7), C.c_int(-7)
    assert outcome(vpt, vpt.hip.vpt_kat_strides(KAT["OP_COUNT"], C.byref(a), C.byref(b))) == (INVALID, "unknown KAT op 15")
    assert outcome(vpt, vpt.hip.vpt_kat_strides(-1, C.byref(a), C.byref(b))) == (INVALID, "unknown KAT op -1")
    assert outcome(vpt, vpt.hip.vpt_kat_strides(0, None, C.byref(b))) == (INVALID, "unknown KAT op 0")
    assert outcome(vpt, vpt.hip.vpt_kat_strides(0, C.byref(a), None)) == (INVALID, "unknown KAT op 0")
    assert (a.value, b.value) == (-7, -7)
    for op, si in KAT_IN.items():
        assert vpt.hip.vpt_kat_strides(op, C.byref(a), C.byref(b)) == 0 and a.value == si


def test_kat_refusals(vpt, dev):
    one = np.zeros((1, 19), np.float32)
    o = np.full((1, 32), -7, np.float32)
    call = lambda *a: outcome(vpt, vpt.hip.vpt_kat(*a))   # noqa: E731
    assert call(None, 0, 0, 1, one.ctypes.data, o.ctypes.data) == (INVALID, "bad argument")
    assert call(dev.handle, 0, 0, -1, one.ctypes.data, o.ctypes.data) == (INVALID, "bad argument")
    assert call(dev.handle, 0, 0, 1, None, o.ctypes.data) == (INVALID, "bad argument")
    assert call(dev.handle, 0, 0, 1, one.ctypes.data, None) == (INVALID, "bad argument")
    assert call(dev.handle, KAT["OP_COUNT"], 0, 1, one.ctypes.data, o.ctypes.data) == (INVALID, "unknown KAT op 15")
    assert call(dev.handle, -1, 0, 1, one.ctypes.data, o.ctypes.data) == (INVALID, "unknown KAT op -1")
    assert call(dev.handle, 0, 0, 0, None, None)[0] == 0
    assert np.all(o == -7)


@pytest.mark.parametrize("op,column,bad,record", [
    # a record of zeros is valid for the first four families (material type 0, camera 0, instance 0, element 0): record 1 carries the fault
    ("LOBES", 0, 8.0, 1),        # one past VPT_MAT_GLTFPBR
    ("LOBES", 0, 0.5, 1),        # not an integer
    ("CAMERA", 0, 1.0, 1),       # num_cameras
    ("INTERSECT", 6, 2.0, 1),    # num_instances
    ("INTERSECT", 6, -2.0, 1),
    ("SURFACE", 0, 2.0, 1),      # num_instances
    ("SURFACE", 1, 1e6, 1),      # past the elements of instance 0's shape
    # the scene has none of these tables: id 0 is out of range already
    ("TEXTURE", 0, 0.0, 0),
    ("SDF_NORMAL", 1, 0.0, 0),   # kind 0: a volume instance
    ("SDF_NORMAL", 0, 2.0, 0),   # no such kind
    ("SPHERETRACE", 6, 0.0, 0),
    ("VOLUME", 0, 0.0, 0),
    ("SDF_FUNCTION", 0, 0.0, 0),
])
def test_kat_refuses_a_record_whose_id_is_out_of_range(vpt, dev, op, column, bad, record):
    records = np.zeros((record + 1, KAT_IN[KAT[op]]), np.float32)
    if op == "INTERSECT":
        records[:, 3:6] = (0, 0, -1)
    records[record, column] = bad
    got, out = kat(vpt, dev, KAT[op], records)
    assert got == (INVALID, f"KAT op {KAT[op]} record {record}: id out of range")
    assert np.all(out == -7)


@pytest.mark.parametrize("iparam", [-1, (1 << 20) + 1])
def test_kat_refuses_an_iteration_limit_out_of_range(vpt, dev, iparam):
    record = np.array([[0, 0, 5, 0, 0, -1, -1]], np.float32)   # sdf -1: the whole scene
    got, out = kat(vpt, dev, KAT["SPHERETRACE"], record, iparam)
    assert got == (INVALID, f"KAT op 12: iteration limit {iparam} out of range")
    assert np.all(out == -7)


# ---- vpt_selftest_light_cdf ------------------------------------------------------------------------------------------------------------
def test_selftest_light_cdf_refusals(vpt, dev):
    bad, indexed = C.c_ulonglong(7), C.c_int(-7)
    call = lambda *a: outcome(vpt, vpt.hip.vpt_selftest_light_cdf(*a))   # noqa: E731
    assert len(dev.get_lights()[0]) == 1
    assert call(dev.handle, 1, 64, C.byref(bad), C.byref(indexed)) == (INVALID, "light 1 out of range")   # num_lights
    assert call(dev.handle, -1, 64, C.byref(bad), C.byref(indexed)) == (INVALID, "light -1 out of range")
    assert call(dev.handle, 0, 0, C.byref(bad), C.byref(indexed)) == (INVALID, "bad argument")
    assert call(None, 0, 64, C.byref(bad), C.byref(indexed)) == (INVALID, "bad argument")
    assert call(dev.handle, 0, 64, None, C.byref(indexed)) == (INVALID, "bad argument")
    assert call(dev.handle, 0, 64, C.byref(bad), None) == (INVALID, "bad argument")
    assert (bad.value, indexed.value) == (7, -7)
