"""vpt_scene_update_lights on the GPU (include/vpt.h).  The criterion is equality of bits, no tolerance anywhere:
A = DeviceScene(original); A.update_lights(edit) against B = a DeviceScene made from the host scene after the same edit and
update_lights().  The light list and CDF pool A holds must be the host mirror's byte for byte, the six hashes of its light tables
B's, its BVHs the mirror's, and every render (image as uint32, rngs, hits) B's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import light_edits as L
import scene_edits as E
from conftest import GOLDEN, ROOT
from test_scene_update_gpu import assert_same_bvh, render, same_state

pytestmark = pytest.mark.gpu

MESH_SHADERS = ("volpathtrace", "pathtrace", "naive", "eyelight")
K2_SHADERS = ("implicit", "implicit_normal")


def path(scene_file):
    return os.path.join(GOLDEN, "scenes", scene_file)


def shaders_of(scene_file):
    return K2_SHADERS if scene_file in (L.GRID, L.SDFN) else MESH_SHADERS


def updated_pair(vpt, scene_file, edit):
    """(A, B, edited host scene, the SceneEdit)"""
    A = vpt.DeviceScene(vpt.HostScene(path(scene_file)), 0)
    host = vpt.HostScene(path(scene_file))
    edit(host)
    what = host.update_lights()
    assert not what.empty()
    A.update_lights(what)
    return A, vpt.DeviceScene(host, 0), host, what


def assert_same_lights(A, B, host, what):
    lights, cdf = A.get_lights()
    want_lights, want_cdf = host.lights()
    assert lights.tobytes() == want_lights.tobytes(), f"{what}: light list {lights} differs from the host mirror's {want_lights}"
    assert cdf.tobytes() == want_cdf.tobytes(), f"{what}: {int((cdf.view(np.uint32) != want_cdf.view(np.uint32)).sum())} of {len(cdf)} cdf entries differ from the host mirror's"
    names = ("lights", "light_cdf", "light_rec", "light_prims", "light_index + pool", "light_guide")
    a, b = A.light_tables_hash(), B.light_tables_hash()
    assert a == b, f"{what}: tables that differ from the fresh scene's: {[n for n, x, y in zip(names, a, b) if x != y]}"


def assert_same_everything(vpt, A, B, host, scene_file, what):
    assert_same_lights(A, B, host, what)
    assert_same_bvh(A, host, what)
    lights, _ = A.get_lights()
    for l in range(len(lights)):
        bad, indexed = A.selftest_light_cdf(l, 1 << 16)
        assert bad == 0 and indexed == B.selftest_light_cdf(l, 1 << 16)[1], (what, l, bad, indexed)
    for shader in shaders_of(scene_file):
        a, b = render(vpt, A, host, scene_file, shader), render(vpt, B, host, scene_file, shader)
        assert same_state(a, b), f"{what}: {shader} differs from the fresh scene's render"


@pytest.mark.parametrize("name", list(L.CASES))
def test_update_lights_equals_a_fresh_scene(vpt, name):
    scene_file, edit = L.CASES[name]
    A, B, host, what = updated_pair(vpt, scene_file, edit)
    print(f"{name}: {A.update_stats()} (launches, bytes, device ms of the refit); lights {A.get_lights()[0].tolist()}", flush=True)
    assert_same_everything(vpt, A, B, host, scene_file, name)
    if name != "curves_hair_on":   # the edit is not a no-op: the light tables or some shader see it
        original = vpt.HostScene(path(scene_file))
        C = vpt.DeviceScene(original, 0)
        assert A.light_tables_hash() != C.light_tables_hash(), name
        assert any(not same_state(render(vpt, A, host, scene_file, s), render(vpt, C, original, scene_file, s)) for s in shaders_of(scene_file)), name


def test_new_large_lights_are_indexed(vpt):
    """jade (6 144 quads) and the head (144 046 triangles) get the 16-ary levels and the guide table (2), and the searches through
    them equal the plain binary search"""
    for name, elements in (("vol_jade_on", 6144), ("head_on", 144046)):
        A, _, host, _ = updated_pair(vpt, *L.CASES[name])
        lights, _ = A.get_lights()
        assert lights[0]["cdf_len"] == elements
        assert A.selftest_light_cdf(0, 1 << 20) == (0, 2), name


def test_head_leaves_the_compact_record_instance(vpt):
    """an all-triangle scene whose lights were environments renders through the compact records; with a 144 046-triangle emitter its
    path tracers need the mesh-light walk - the render equals the fresh scene's (test above) and differs from the original's"""
    A, B, host, _ = updated_pair(vpt, *L.CASES["head_on"])
    assert A.record_bytes() == (48, 64)   # the records are still there: the choice is the launch's
    original = vpt.HostScene(path(L.HEAD))
    C = vpt.DeviceScene(original, 0)
    assert not same_state(render(vpt, A, host, L.HEAD, "pathtrace"), render(vpt, C, original, L.HEAD, "pathtrace"))


@pytest.mark.parametrize("variable,name", [("VPT_LIGHTS_PLAIN", "vol_jade_on"), ("VPT_LIGHTS_PLAIN", "lobes_glow_nudge"), ("VPT_LIGHTS_PLAIN", "head_on"),
                                           ("VPT_NO_LEAN", "vol_on_off_move"), ("VPT_NO_LEAN", "head_on"), ("VPT_NO_LEAN", "grid_sdf_on"),
                                           ("VPT_NO_LEAN", "sdfn_sdf_off")])
def test_switches_keep_the_equality(variable, name):
    """the plain one-lane running sum gives the wave form's bits (both equal the host mirror's), and the instances with every light
    feature render what the lean ones do; in a child process, as the existing tests of such switches do"""
    env = dict(os.environ, **{variable: "1"})
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", f"{__file__}::test_update_lights_equals_a_fresh_scene[{name}]"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_on_then_off_returns_the_original(vpt):
    original = vpt.HostScene(path(L.S03))
    A = vpt.DeviceScene(vpt.HostScene(path(L.S03)), 0)
    before_hash = A.light_tables_hash()
    before = [render(vpt, A, original, L.S03, s) for s in MESH_SHADERS]
    host = vpt.HostScene(path(L.S03))
    L.CASES["vol_jade_on"][1](host)
    A.update_lights(host.update_lights())
    assert A.light_tables_hash() != before_hash
    L.switch_off(L.S03, "jade")(host)
    A.update_lights(host.update_lights())
    assert A.light_tables_hash() == before_hash
    assert host.stats() == original.stats()
    for s, st in zip(MESH_SHADERS, before):
        assert same_state(st, render(vpt, A, original, L.S03, s)), s


def test_a_plain_update_after_update_lights(vpt):
    """update_lights, then vpt_scene_update moving the new light's instance: the light mirrors of the handle followed the rebuild"""
    A, _, host, _ = updated_pair(vpt, *L.CASES["vol_jade_on"])
    jade = L.index_of(L.S03, "instances", "jade")
    E.translate(host, jade, dx=0.15, dy=0.05)
    E.rotate_instance(host, jade, 0.3)
    A.update(host.update_bvh())
    B = vpt.DeviceScene(host, 0)
    assert_same_everything(vpt, A, B, host, L.S03, "moved after the rebuild")
    # and what vpt_scene_update refuses follows the new list: jade's sphere is a light's shape now
    sphere = L.index_of(L.S03, "shapes", "sphere")
    with pytest.raises(vpt.VptError) as err:
        A.update(vpt.SceneEdit(shapes={sphere: (host.shape_positions(sphere), None)}))
    assert "(-5)" in str(err.value) and "light" in str(err.value)


@pytest.mark.parametrize("name,edit", [
    ("instance", lambda h: E.translate(h, 1, dx=0.2)),
    ("vertices", lambda h: E.move_vertices(h, E.nudge)),
    ("camera and material", lambda h: [E.edit_camera(h), E.edit_material(h, E.first_plain_material(h))]),
    ("emissive stays emissive", lambda h: L.emit(h, L.index_of(L.S03, "materials", "arealight1"), (5.0, 4.0, 3.0))),
])
def test_an_edit_without_consequence_does_what_update_does(vpt, name, edit):
    host = vpt.HostScene(path(L.S03))
    edit(host)
    what = host.update_lights()
    A, U = vpt.DeviceScene(vpt.HostScene(path(L.S03)), 0), vpt.DeviceScene(vpt.HostScene(path(L.S03)), 0)
    A.update_lights(what)
    U.update(what)
    assert A.update_stats()[:2] == U.update_stats()[:2], name
    B = vpt.DeviceScene(host, 0)
    assert A.light_tables_hash() == U.light_tables_hash() == B.light_tables_hash()
    assert same_state(render(vpt, A, host, L.S03, "volpathtrace"), render(vpt, B, host, L.S03, "volpathtrace"))


def test_bytes_of_the_head_case(vpt):
    """nothing proportional to the element count crosses PCIe: the material (its payload) plus a few words per light, in either
    direction - list entry (6 words), index header (14), record tag (1), job descriptor (6), {sorted, last entry} back (2): 29,
    bounded here by 32 words a light.  The CDF alone is 144 046 words."""
    A, _, host, what = updated_pair(vpt, *L.CASES["head_on"])
    launches, sent, _ = A.update_stats()
    import ctypes as C
    payload = len(what.materials) * C.sizeof(vpt.VptMaterial)
    lights = len(A.get_lights()[0])
    print(f"head_on: {launches} launches, {sent} bytes for a payload of {payload} and {lights} lights", flush=True)
    assert payload <= sent <= payload + 32 * 4 * lights


def test_refused_edits_leave_the_lights_untouched(vpt):
    host = vpt.HostScene(path(L.S03))
    A = vpt.DeviceScene(host, 0)
    before_hash, before = A.light_tables_hash(), render(vpt, A, host, L.S03, "pathtrace")
    jade = L.index_of(L.S03, "materials", "jade")
    glow = host.material(jade)
    glow.emission[0] = 1.0
    bad_type = host.material(jade)
    bad_type.emission[0], bad_type.type = 1.0, 99
    nan = host.material(jade)
    nan.emission[1] = float("nan")
    frame = host.instance_frame(0)
    frame[4] = np.inf
    light_shape = L.index_of(L.S03, "shapes", "arealight1")
    refused = [
        (vpt.SceneEdit(materials={jade: bad_type}), "bad type"),
        (vpt.SceneEdit(materials={jade: nan}), "material entry 0"),
        (vpt.SceneEdit(materials={host.count("materials"): glow}), "out of range"),
        (vpt.SceneEdit(materials={jade: glow}, instances={0: frame}), "instance entry 0"),
        (vpt.SceneEdit(materials={jade: glow}, shapes={light_shape: (np.full_like(host.shape_positions(light_shape), np.nan), None)}), "shape entry 0"),
    ]
    for edit, text in refused:
        with pytest.raises(vpt.VptError) as err:
            A.update_lights(edit)
        assert "(-1)" in str(err.value) and text in str(err.value), (str(err.value), text)
        assert A.light_tables_hash() == before_hash, text
        assert same_state(before, render(vpt, A, host, L.S03, "pathtrace")), text
    # vpt_scene_update itself still refuses both edits that vpt_scene_update_lights takes
    off = host.material(L.index_of(L.S03, "materials", "arealight1"))
    off.emission[0] = off.emission[1] = off.emission[2] = 0.0
    for edit, text in ((vpt.SceneEdit(materials={jade: glow}), "emission"), (vpt.SceneEdit(materials={L.index_of(L.S03, "materials", "arealight1"): off}), "emission"),
                       (vpt.SceneEdit(shapes={light_shape: (host.shape_positions(light_shape) * 2, None)}), "light")):
        with pytest.raises(vpt.VptError) as err:
            A.update(edit)
        assert "(-5)" in str(err.value) and text in str(err.value)
        assert A.light_tables_hash() == before_hash, text
    assert same_state(before, render(vpt, A, host, L.S03, "pathtrace"))


def test_session_edit_lights(vpt):
    """RenderSession.edit_lights equals a session on a fresh scene: the preview, then 3 + 5 samples"""
    host = vpt.HostScene(path(L.S03))
    p = vpt.PathtraceParams(resolution=96, samples=64, shader="pathtrace", bounces=4)
    s1 = vpt.RenderSession(vpt.DeviceScene(vpt.HostScene(path(L.S03)), 0), p)
    s1.advance(2)
    L.CASES["vol_on_off_move"][1](host)
    s1.edit_lights(host.update_lights())
    s2 = vpt.RenderSession(vpt.DeviceScene(host, 0), p)
    assert s1.samples == s2.samples == 0
    assert np.array_equal(s1.display(), s2.display())   # the preview both show after a reset
    for step in (3, 5):
        s1.advance(step), s2.advance(step)
        assert s1.samples == s2.samples
        assert same_state(s1.state(), s2.state()), step
        assert np.array_equal(s1.display(), s2.display()), step
    with pytest.raises(vpt.VptError):   # a refused edit leaves the session as it was
        bad = host.material(0)
        bad.type = 99
        s1.edit_lights(vpt.SceneEdit(materials={0: bad}))
    assert s1.samples == 8 and same_state(s1.state(), s2.state())


def test_multi_update_lights_on_one_device(vpt):
    host = vpt.HostScene(path(L.S03))
    M = vpt.MultiDeviceScene(vpt.HostScene(path(L.S03)), [0])
    L.CASES["vol_on_off_move"][1](host)
    M.update_lights(host.update_lights())
    B = vpt.DeviceScene(host, 0)
    p = vpt.PathtraceParams(resolution=64, samples=8, shader="volpathtrace", bounces=8)
    want = host.make_state(p)
    B.pathtrace_samples(want, p, 8)
    got = host.make_state(p)
    M.pathtrace_samples(got, p, 8)
    assert same_state(got, want)


# ---- end to end against the reference: its own render of the edited scene (tests/golden/light_edit_states.npz) ---------------------
def _state_cases():
    f = os.path.join(GOLDEN, "light_edit_stats.json")
    return {k: v["state"] for k, v in (json.load(open(f)) if os.path.exists(f) else {}).items() if "state" in v}


def test_reference_state_fixtures_are_there():
    assert len(_state_cases()) >= L.STATE_WANTED and set(_state_cases()) <= set(L.STATE_CANDIDATES)


@pytest.mark.parametrize("name", sorted(_state_cases()))
def test_update_lights_matches_the_references_render(vpt, oracle, name):
    """the strict check of test_gpu_parity on a handle whose lights were REBUILT to the edited scene, against the reference's state of
    that scene; floors: 0.998 on identical streams and matching pixels as for the unedited cases, and on the stable share 0.02 under
    what the fixture script measured on the reference's arithmetic"""
    from test_gpu_parity import _check_against_reference
    case = _state_cases()[name]
    A, _, host, _ = updated_pair(vpt, *L.CASES[name])
    gold = np.load(os.path.join(GOLDEN, "light_edit_states.npz"))
    p = vpt.PathtraceParams(resolution=case["resolution"], samples=case["samples"], shader=case["shader"], bounces=case["bounces"])
    g = host.make_state(p)
    A.pathtrace_samples(g, p, case["samples"])
    print(f"{name}: rendering done, checking against the reference", flush=True)
    assert case["stable_share"] >= 0.8
    _check_against_reference(oracle, host, p, case["samples"], g, gold[name + "_image"], gold[name + "_rngs"], name, 0.998, 0.998, case["stable_share"] - 0.02)
