"""Point and line hits on the MI355X held to the float64 reference of tests/curve_exact.py, ray by ray: vpt_intersect through the
certificate on every ray set of tests/curve_cases.py (whole-scene and single-instance queries, both traversal settings, dense and
sparse waves) and on dense.json; {u, v, t} bit for bit against the float32 restatement on the element the device reported; the AOV
planes against the shading reference; and vpt_kat's refusal of the two ops that cannot walk such a scene."""
import json
import os
import shutil

import numpy as np
import pytest

import curve_cases
import curve_exact
import curve_restated
import kat_lib
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SCENES = os.path.join(GOLDEN, "scenes", "09_curves_synth")
CURVES, DENSE = os.path.join(SCENES, "curves.json"), os.path.join(SCENES, "dense.json")
SETTINGS = {"default": {}, "own_forms_spilled": {"VPT_NO_GROUP_FORMS": "1", "VPT_STACK_LDS": "4"}}
PIXELS = 96
LINE_PIXELS, POINT_PIXELS = 30, 15     # tests/test_curve_exact_host.py shows the pixel-centre rays reach these


def _device(vpt, path, env):
    """a handle created under `env` (the switches are read at handle creation)"""
    assert vpt.device_count() >= 1, "GPU test selected but no HIP device is visible"
    os.environ.update(env)
    try:
        return vpt.DeviceScene(vpt.HostScene(path), 0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def case(vpt, tmp_path_factory):
    c = curve_cases.Case(vpt, tmp_path_factory.mktemp("curve_exact"))
    c.devs = {name: _device(vpt, c.path, env) for name, env in SETTINGS.items()}
    return c


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _report(verdict):
    return f"{len(verdict.violations)} violations, the first: {verdict.violations[:3]}"


@pytest.mark.parametrize("name", ["lines", "points", "edge", "tmin", "inside"])
def test_intersect_passes_the_certificate(case, name):
    line, point = curve_cases.instance_of("lines_all", "rigid"), curve_cases.instance_of("points_colors", "scaled")
    rays = case.sets[name]
    batches = {"dense": (rays, case.refs[name]), "3 per wave": (curve_cases.sparse(rays), None)}
    for batch, (r, ref) in batches.items():
        ref = ref or curve_exact.Reference(case.elements, r, keep=True)
        for query in (-1, line, point):
            got = {setting: dev.intersect(r, query) for setting, dev in case.devs.items()}
            assert _same(got["default"], got["own_forms_spilled"]), (name, batch, query)
            ids, uvt = got["default"]
            verdict = curve_exact.certify(ref, ids, uvt, instances=None if query < 0 else [query], face_instances=[curve_cases.PYRAMID])
            print(f"{name}, {batch}, query {query}: {(ids[:, 0] >= 0).sum()} hits, {verdict.undecided.sum()} of {len(r)} rays undecided")
            assert not verdict.violations, f"{name}, {batch}, query {query}: {_report(verdict)}"


def test_dense_strands_pass_the_certificate(vpt):
    scene = vpt.HostScene(DENSE)
    elements = curve_exact.curve_instances(scene, [2])
    rays = curve_cases.dense_rays()
    ids, uvt = vpt.DeviceScene(scene, 0).intersect(rays, instance=2)
    verdict = curve_exact.certify(curve_exact.Reference(elements, rays, chunk=32), ids, uvt)
    print(f"dense: {(ids[:, 0] == 2).sum()} hits, {verdict.undecided.sum()} of {len(rays)} rays undecided")
    assert not verdict.violations, _report(verdict)
    assert (ids[:, 0] == 2).sum() > len(rays) // 8 and verdict.undecided.sum() <= 0.15 * len(rays)


def test_uvt_bits_on_the_reported_element(case):
    """given the element, the function depends on no traversal order: under the identity frame (the ray's transform is then exact) the
    device's {u, v, t} are the float32 restatement's on that element, bit for bit (NaN equals NaN)"""
    checked = 0
    for name, rays in case.sets.items():
        ids, uvt = case.devs["default"].intersect(rays)
        for el in case.elements:
            rows = np.nonzero(ids[:, 0] == el.instance)[0]
            if not el.identity or not len(rows):
                continue
            ok, want = curve_restated.on_elements(el, rays[rows], ids[rows, 1])
            assert ok.all(), (name, el.instance, rows[~ok][:8].tolist())
            same = (uvt[rows].view(np.uint32) == want.view(np.uint32)) | (np.isnan(uvt[rows]) & np.isnan(want))
            bad = rows[~same.all(1)]
            assert not len(bad), (name, el.instance, len(bad), bad[:4].tolist(), uvt[bad[:4]].tolist(), want[~same.all(1)][:4].tolist())
            checked += len(rows)
    print(f"{checked} hits on identity-frame instances, equal bits")
    assert checked >= 8 * 100


def test_aov_planes_lie_within_the_shading_reference(vpt, case):
    params = vpt.PathtraceParams(resolution=PIXELS, samples=1, shader="eyelight", bounces=4)
    state = case.scene.make_state(params)
    assert (state.width, state.height) == (PIXELS, PIXELS)
    planes = case.devs["default"].render_aovs(state, params, 1)
    ids, uvt = planes["ids"].reshape(-1, 2), planes["uvt"].reshape(-1, 3)
    flat = {k: planes[k].reshape(-1, 4).astype(np.float64) for k in ("normal", "albedo", "texcoord", "depth")}
    outgoing = -curve_exact.camera_rays(case.scene.camera(0), PIXELS, PIXELS).reshape(-1, 6)[:, 3:]
    # the float32 eval_camera behind the device's outgoing: q (2 roundings), its normalisation (4), the focus point (2), its normalisation
    # (4), the frame's vector transform (3 of 4) and normalisation (4)
    e_outgoing = 20 * curve_exact.EPS
    counts = dict.fromkeys(curve_cases.VARIANTS, 0)
    for el in case.elements:
        rows = np.nonzero((ids[:, 0] == el.instance) & np.isfinite(uvt).all(1))[0]
        if not len(rows):
            continue
        assert (planes["depth"].reshape(-1, 4)[rows, 0].view(np.uint32) == uvt[rows, 2].view(np.uint32)).all()
        assert (flat["depth"][rows, 1:] == [0, 0, 1]).all() and all((flat[k][rows, 3] == 1).all() for k in ("normal", "albedo", "texcoord"))
        want = curve_exact.shade(el, case.material_color(el.instance), ids[rows, 1], uvt[rows, 0].astype(np.float64),
                                 uvt[rows, 1].astype(np.float64), outgoing[rows], e_outgoing)
        for plane, key, width in (("texcoord", "texcoord", 2), ("albedo", "color", 3), ("normal", "normal", 3)):
            off = np.abs(flat[plane][rows, :width] - want[key]).max(1)
            worst = int(np.argmax(off / np.maximum(want["e_" + key], 1e-300)))
            assert (off <= want["e_" + key]).all(), (plane, el.instance, int(rows[worst]), float(off[worst]), float(want["e_" + key][worst]))
        assert (flat["texcoord"][rows, 2] == 0).all()
        counts[case.variant_of(el.instance)] += len(rows)
    print(counts)
    for variant, n in counts.items():
        assert n >= (LINE_PIXELS if variant in curve_cases.LINE_VARIANTS else POINT_PIXELS), counts


def test_kat_refuses_intersect_and_surface_on_a_scene_with_curves(vpt, tmp_path):
    dev = vpt.DeviceScene(vpt.HostScene(CURVES), 0)
    ray, hit = np.float32([[0, 0.1, 1, 0, 0, -1, -1]] * 4), np.float32([[2, 0, 0.5, 0.5, 0, 0, 1]] * 4)   # valid records, were they run
    for op, rec in (("intersect", ray), ("surface", hit)):
        with pytest.raises(vpt.VptError, match=r"\(-5\).*points or lines.*vpt_intersect.*AOV pass"):
            dev.kat(kat_lib.OPS[op][0], rec)
    # the other ops answer as before: the lights of the scene are shapes of faces, and their single-instance walks enter no point or
    # line leaf - the same bits as on a copy of the scene that keeps only its instances of faces (floor, light, pyramid)
    scene = json.load(open(CURVES))
    names = ("floor", "arealight1", "pyramid")
    shapes = [sh for sh in scene["shapes"] if sh["name"] in names]
    keep = [dict(i, shape=[sh["name"] for sh in shapes].index(scene["shapes"][i["shape"]]["name"])) for i in scene["instances"] if i["name"] in names]
    os.makedirs(tmp_path / "shapes")
    for sh in shapes:
        shutil.copy(os.path.join(SCENES, sh["uri"]), tmp_path / "shapes")
    with open(tmp_path / "faces.json", "w") as f:
        json.dump(dict(scene, shapes=shapes, instances=keep), f)
    faces = vpt.DeviceScene(vpt.HostScene(str(tmp_path / "faces.json")), 0)
    g = np.random.default_rng(11)
    lo, hi = np.array([-0.6, 0.0, -0.4]), np.array([0.6, 0.4, 0.4])
    records = {"camera": kat_lib.gen_camera(g, {"cameras": 1}, 256), "environment": kat_lib.gen_dirs(g, 256),
               "sample_lights": kat_lib.gen_sample_lights(g, lo, hi, 512)}
    for name, rec in records.items():
        a, b = dev.kat(kat_lib.OPS[name][0], rec), faces.kat(kat_lib.OPS[name][0], rec)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
        if name == "sample_lights":
            pdf = np.concatenate([rec[:, :3], a], 1)
            for op in ("lights_pdf", "lights_pdf_k2"):
                a2, b2 = dev.kat(kat_lib.OPS[op][0], pdf, 450), faces.kat(kat_lib.OPS[op][0], pdf, 450)
                assert np.array_equal(a2.view(np.uint32), b2.view(np.uint32)) and (a2 > 0).any(), op
    # and the handle renders as usual afterwards: the reference's own eyelight render of the scene
    ref = np.load(os.path.join(GOLDEN, "curves_states.npz"))
    host = vpt.HostScene(CURVES)
    params = vpt.PathtraceParams(resolution=96, samples=4, shader="eyelight", bounces=8)
    state = host.make_state(params)
    dev.pathtrace_samples(state, params, 4)
    assert np.array_equal(state.image.view(np.uint32), ref["eyelight_image"].view(np.uint32))
