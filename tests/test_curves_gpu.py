"""Shapes of points and lines on the MI355X against the reference's own renders (tests/golden/curves_states.npz,
written by ref_driver: tests/golden/make_curves_scene.py): all seven mesh shaders on 09_curves_synth/curves.json, volpathtrace on the
20k-segment dense.json; the same bits with the group forms off and with spilled stacks; the device BVH build; vpt_intersect against
the path tracer's traversal and a float64 brute force; one device through vpt_multi_*; ypathtrace's JPEG."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

SCENES = os.path.join(GOLDEN, "scenes", "09_curves_synth")
CURVES, DENSE = os.path.join(SCENES, "curves.json"), os.path.join(SCENES, "dense.json")
RESOLUTION, BOUNCES = 96, 8
CASES = (("volpathtrace", 4), ("pathtrace", 4), ("naive", 4), ("eyelight", 4), ("normal", 2), ("texcoord", 2), ("color", 2))
REF = np.load(os.path.join(GOLDEN, "curves_states.npz"))


def _render(vpt, path, shader, resolution, spp, multi=False):
    scene = vpt.HostScene(path)
    params = vpt.PathtraceParams(resolution=resolution, samples=spp, shader=shader, bounces=BOUNCES)
    state = scene.make_state(params)
    dev = vpt.MultiDeviceScene(scene, [0]) if multi else vpt.DeviceScene(scene, 0)
    dev.pathtrace_samples(state, params, spp)
    return state


# shaders whose radiance holds no device libm result on these scenes: bit for bit.  The three that sample BSDF lobes and light
# directions pass ocml's sinf / cosf / powf / expf (<= 2 ulp from glibc's) into the radiance of pixels whose streams
# stay the reference's: those are held to identical streams and the 2e-3 radiance bar of tests/test_gpu_parity.py, on every pixel
EXACT = ("eyelight", "normal", "texcoord", "color")


def _same_bits(state, key, spp, shader):
    ref_img, ref_rng = REF[f"{key}_image"], REF[f"{key}_rngs"]
    assert state.samples == spp and (state.hits == REF[f"{key}_hits"]).all()
    assert np.array_equal(state.rngs, ref_rng), f"{key}: {np.mean(np.any(state.rngs != ref_rng, -1)):.4f} of the streams differ"
    if shader in EXACT:
        assert np.array_equal(state.image.view(np.uint32), ref_img.view(np.uint32)), \
            f"{key}: {np.mean(np.any(state.image != ref_img, -1)):.4f} of the pixels differ"
    else:
        close = np.isclose(state.image, ref_img, rtol=2e-3, atol=2e-3 * spp)
        rel = np.max(np.abs(state.image - ref_img) / (np.abs(ref_img) + 1e-6))
        print(f"{key}: bit-identical pixels {np.mean(np.all(state.image == ref_img, -1)):.4f}, max relative difference {rel:.2e}")
        assert close.all(), f"{key}: {np.mean(~np.all(close, -1)):.4f} of the pixels off by more than 2e-3"


SWITCHES = {"default": {}, "own_forms": {"VPT_NO_GROUP_FORMS": "1"}, "spilled": {"VPT_STACK_LDS": "4"},
            "own_forms_spilled": {"VPT_NO_GROUP_FORMS": "1", "VPT_STACK_LDS": "4"}}


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("shader,spp", CASES)
def test_curves_replay_the_references_paths(vpt, monkeypatch, shader, spp, switch):
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    _same_bits(_render(vpt, CURVES, shader, RESOLUTION, spp), shader, spp, shader)


@pytest.mark.parametrize("switch", ["default", "own_forms_spilled"])
def test_dense_strands_replay_the_references_paths(vpt, monkeypatch, switch):
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    _same_bits(_render(vpt, DENSE, "volpathtrace", 64, 2), "dense", 2, "volpathtrace")


def test_one_device_of_vpt_multi_equals_the_single_gpu_bits(vpt):
    one, multi = _render(vpt, CURVES, "volpathtrace", RESOLUTION, 4), _render(vpt, CURVES, "volpathtrace", RESOLUTION, 4, multi=True)
    assert np.array_equal(multi.rngs, one.rngs) and np.array_equal(multi.hits, one.hits)
    assert np.array_equal(multi.image.view(np.uint32), one.image.view(np.uint32))


def test_device_bvh_build_equals_the_host_build(vpt):
    for path in (CURVES, DENSE):
        assert vpt.HostScene(path, bvh_device=0).stats() == vpt.HostScene(path).stats()


def _segments(path):
    """the dense shape's segments as float64 (p0, p1, r0, r1) from its PLY (shapes/dense.ply: x y z radius, line lists)"""
    raw = open(os.path.join(SCENES, "shapes", "dense.ply"), "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode().split("\n")
    nv = int([h for h in head if h.startswith("element vertex")][0].split()[-1])
    nl = int([h for h in head if h.startswith("element line")][0].split()[-1])
    v = np.frombuffer(raw, "<f4", nv * 4, end).reshape(nv, 4)
    off, segs = end + nv * 16, []
    for _ in range(nl):
        n = raw[off]
        idx = np.frombuffer(raw, "<i4", n, off + 1)
        segs += [(a, b) for a, b in zip(idx[:-1], idx[1:])]
        off += 1 + 4 * n
    segs = np.asarray(segs)
    return v[segs[:, 0], :3].astype(np.float64), v[segs[:, 1], :3].astype(np.float64), v[segs[:, 0], 3].astype(np.float64), \
        v[segs[:, 1], 3].astype(np.float64)


def _brute_force(rays, p0, p1, r0, r1):
    """intersect_line of yocto_geometry.h:705-746 in float64 over every segment: the nearest distance per ray (inf: a miss)"""
    best = np.full(len(rays), np.inf)
    for i, (o, d) in enumerate(zip(rays[:, :3].astype(np.float64), rays[:, 3:].astype(np.float64))):
        v, w = p1 - p0, o - p0
        a, b, c = d @ d, v @ d, np.einsum("ij,ij->i", v, v)
        dd, e = w @ d, np.einsum("ij,ij->i", v, w)
        det = a * c - b * b
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (b * e - c * dd) / det
            s = np.clip((a * e - b * dd) / det, 0, 1)
        pr = o + d * t[:, None]
        pl = p0 + v * s[:, None]
        d2 = np.einsum("ij,ij->i", pr - pl, pr - pl)
        r = r0 * (1 - s) + r1 * s
        ok = (det != 0) & (t >= 1e-4) & (d2 <= r * r)
        if ok.any():
            best[i] = t[ok].min()
    return best


def test_intersect_on_dense_strands(vpt):
    scene = vpt.HostScene(DENSE)
    dev = vpt.DeviceScene(scene, 0)
    g = np.random.default_rng(5)
    n = 512
    o = np.stack([g.uniform(-0.5, 0.5, n), np.full(n, 0.15), np.full(n, 1.0)], 1)
    tgt = np.stack([g.uniform(-0.45, 0.45, n), g.uniform(0.0, 0.2, n), g.uniform(-0.45, 0.45, n)], 1)
    rays = np.concatenate([o, tgt - o], 1).astype(np.float32)
    ids, uvt = dev.intersect(rays)
    ids1, uvt1 = dev.intersect(rays, instance=2)
    hit_strand = ids[:, 0] == 2
    assert hit_strand.sum() > n // 8, "the rays should meet the strands"
    # the single-instance query gives the whole-scene bits wherever the strands are the nearest hit
    assert np.array_equal(ids1[hit_strand], ids[hit_strand]) and np.array_equal(uvt1[hit_strand].view(np.uint32), uvt[hit_strand].view(np.uint32))
    # the same traversal as the path tracers' (the own form with spilled stacks gives the same bits)
    os.environ["VPT_NO_GROUP_FORMS"], os.environ["VPT_STACK_LDS"] = "1", "4"
    try:
        dev2 = vpt.DeviceScene(vpt.HostScene(DENSE), 0)
        ids2, uvt2 = dev2.intersect(rays)
    finally:
        del os.environ["VPT_NO_GROUP_FORMS"], os.environ["VPT_STACK_LDS"]
    assert np.array_equal(ids2, ids) and np.array_equal(uvt2.view(np.uint32), uvt.view(np.uint32))
    # distances against a float64 brute force over the 20k segments, except at near-ties of two candidates
    p0, p1, r0, r1 = _segments(DENSE)
    best = _brute_force(rays[:, :], p0, p1, r0, r1)
    strand_t = np.where(ids1[:, 0] == 2, uvt1[:, 2], np.inf)
    agree = np.isclose(strand_t, best, rtol=1e-4, atol=1e-6) | (np.isinf(strand_t) & np.isinf(best))
    assert agree.mean() > 0.98, f"{agree.mean():.4f}"


def test_ypathtrace_jpeg_equals_the_references(tmp_path):
    out = tmp_path / "curves.jpg"
    r = subprocess.run([os.path.join(ROOT, "volumetric-path-tracer_amd", "ypathtrace"), "--scene", CURVES, "--shader", "volpathtrace",
                        "--samples", "2", "--resolution", "48", "--bounces", str(BOUNCES), "--output", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == open(os.path.join(GOLDEN, "curves_volpath.jpg"), "rb").read()
