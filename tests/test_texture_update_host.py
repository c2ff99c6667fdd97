"""The host side of vpt_scene_update_textures: HostScene.set_environment / set_texture / update_textures(), the
mirror's make_lights over a scene whose environment or textures were edited through the setters, against the same scene loaded
afresh from an edited scene file, against the reference's own make_lights (tests/golden/texture_edit_stats.json, written by
tests/golden/make_texture_edit_fixtures.py), and against a numpy replay of the rule of include/vpt.h.  No device."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import texture_edits as T
from conftest import GOLDEN, ROOT

F = np.float32


def path(scene_file):
    return os.path.join(GOLDEN, "scenes", scene_file)


def edited(vpt, name, work):
    scene_file = T.cases(vpt)[name][0]
    h = vpt.HostScene(path(scene_file))
    return scene_file, h, T.apply(vpt, name, h, work)


@pytest.mark.parametrize("name", T.NAMES)
def test_update_textures_hands_out_the_edit_and_remakes_the_lights(vpt, tmp_path, name):
    """every step yields a TextureEdit, a second call none; the list is make_lights' (environments between meshes and SDFs, cdf_len =
    width * height of the texture); the lights change unless the case is built not to change them"""
    scene_file, h, edits = edited(vpt, name, tmp_path)
    assert all(not e.empty() for e in edits) and h.update_textures().empty()
    lights, cdf = h.lights()
    env = [l for l in lights if l["environment"] >= 0]
    e = h.environment(0)
    lit = any(float(c) != 0.0 for c in e.emission)
    assert len(env) == (1 if lit else 0)
    if lit:
        t = h.texture(e.emission_tex)[0] if e.emission_tex >= 0 else np.zeros((0, 0, 4), F)
        assert int(env[0]["cdf_len"]) == t.shape[0] * t.shape[1]
    assert list(lights["cdf_offset"]) == list(np.cumsum([0] + list(lights["cdf_len"]))[:-1]) and len(cdf) == int(lights["cdf_len"].sum())
    original = vpt.HostScene(path(scene_file))
    same = T.lights_of(h.stats()) == T.lights_of(original.stats())
    assert same == (name in T.NO_OPS + ("sky_dim", "floor_repaint")), name


@pytest.mark.parametrize("name", list(T.AS_SCENE_FILE))
def test_update_textures_equals_the_edited_scene_loaded_afresh(vpt, tmp_path, name):
    scene_file, h, _ = edited(vpt, name, tmp_path)
    fresh = vpt.HostScene(T.write_edited_scene(name, tmp_path))
    assert h.stats() == fresh.stats()
    (lights, cdf), (want_lights, want_cdf) = h.lights(), fresh.lights()
    assert lights.tobytes() == want_lights.tobytes() and cdf.tobytes() == want_cdf.tobytes()


def _reference():
    f = os.path.join(GOLDEN, "texture_edit_stats.json")
    return json.load(open(f)) if os.path.exists(f) else {}


def test_reference_fixtures_are_there():
    assert set(_reference()) == set(T.AS_SCENE_FILE)
    states = [k for k, v in _reference().items() if "state" in v]
    assert len(states) == T.STATE_WANTED and set(states) <= set(T.STATE_CANDIDATES)
    gold = np.load(os.path.join(GOLDEN, "texture_edit_states.npz"))
    assert set(gold.files) == {k + s for k in states for s in ("_image", "_rngs")}


@pytest.mark.parametrize("name", list(T.AS_SCENE_FILE))
def test_update_textures_equals_the_references_make_lights(vpt, tmp_path, name):
    """lights, textures and BVH hashes of the mirror against the reference's own load of the edited scene"""
    _, h, _ = edited(vpt, name, tmp_path)
    mine, ref = json.loads(h.stats()), _reference()[name]["stats"]
    assert mine["lights"] == ref["lights"]
    assert mine["textures"] == ref["textures"]
    assert mine["scene_bvh"] == ref["scene_bvh"]
    assert [{k: s[k] for k in ("bvh_nodes", "bvh_nodes_fnv", "bvh_prims_fnv")} for s in mine["shapes"]] == ref["shapes"]


def sinf(x):
    """the C library's float sine, the one make_lights calls"""
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    libm.sinf.restype, libm.sinf.argtypes = ctypes.c_float, [ctypes.c_float]
    return F(libm.sinf(float(x)))


def replay(texels):
    """w[idx] = max4(texel) * sin((j + 0.5f) * pif / height) and its running sum, every operation in float32 (include/vpt.h); max is
    the select (a > b) ? a : b; a byte texel is b / 255.0f per channel; numpy's add.accumulate is the serial chain"""
    h = texels.shape[0]
    v = texels if texels.dtype == np.float32 else (texels.astype(F) / F(255)).astype(F)
    m = v[..., 0]
    with np.errstate(invalid="ignore"):
        for c in (1, 2, 3):
            m = np.where(m > v[..., c], m, v[..., c])
        rows = np.array([sinf(((F(j) + F(0.5)) * F(3.14159265358979323846)) / F(h)) for j in range(h)], F)
        return np.add.accumulate((m * rows[:, None]).astype(F).reshape(-1), dtype=F)


@pytest.mark.parametrize("name,texture", [("sky_1x1", 1), ("sky_5x3", 1), ("sky_13x5", 1), ("sky_16x4", 1), ("sky_67x33", 1), ("sky_bytes_9x7", 1),
                                          ("sky_negative_texel", 1), ("sky_nan_texel", 1), ("sky_to_floor", 0), ("grid_sky_13x5", 0)])
def test_numpy_replay_of_an_environment_cdf(vpt, tmp_path, name, texture):
    """bit for bit; sky_to_floor is floor.png as the sky: the plain division, not the sRGB table the floor's colour goes through"""
    _, h, _ = edited(vpt, name, tmp_path)
    lights, cdf = h.lights()
    env = [l for l in lights if l["environment"] >= 0][0]
    texels = h.texture(texture)[0]
    assert (texels.dtype == np.uint8) == (name in ("sky_bytes_9x7", "sky_to_floor"))
    got, want = cdf[int(env["cdf_offset"]):][:int(env["cdf_len"])], replay(texels)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes()
    if name == "sky_negative_texel":
        assert (np.diff(got) < 0).any()   # not monotonic: no index, as at creation
    if name == "sky_nan_texel":
        assert not nan[:28 * 67 + 40].any() and nan[28 * 67 + 40:].all()
        before = got[20 * 67 + 4]   # the texel with x = 3.9 and y = NaN weighs max(z, w) = 1, not 3.9
        assert F(got[20 * 67 + 5] - before) < F(1.01)


OK_TEXELS = np.zeros((2, 2, 4), F)
REFUSALS = {   # one per rule of include/vpt.h that the host setters can meet
    "environment id out of range": lambda h: h.set_environment(1, emission=(1, 1, 1)),
    "environment id negative": lambda h: h.set_environment(-1, emission=(1, 1, 1)),
    "emission NaN": lambda h: h.set_environment(0, emission=(1, float("nan"), 1)),
    "emission infinite": lambda h: h.set_environment(0, emission=(float("inf"), 1, 1)),
    "emission_tex past the textures": lambda h: h.set_environment(0, emission_tex=2),
    "emission_tex below -1": lambda h: h.set_environment(0, emission_tex=-2),
    "texture id out of range": lambda h: h.set_texture(2, OK_TEXELS),
    "texture id negative": lambda h: h.set_texture(-1, OK_TEXELS),
    "three channels": lambda h: h.set_texture(1, np.zeros((2, 2, 3), F)),
    "float64 texels": lambda h: h.set_texture(1, np.zeros((2, 2, 4), np.float64)),
    "a float texture without texels": lambda h: h.set_texture(1, np.zeros((0, 0, 4), F)),
}


@pytest.fixture(scope="module")
def untouched(vpt):
    h = vpt.HostScene(path(T.S03))
    return h, (h.lights()[0].tobytes(), h.lights()[1].tobytes(), h.stats())


@pytest.mark.parametrize("what", list(REFUSALS))
def test_setters_refuse_what_the_device_would(vpt, untouched, what):
    """after a refusal, lights(), stats() and the pending edit are unchanged"""
    h, before = untouched
    with pytest.raises(vpt.VptError):
        REFUSALS[what](h)
    assert h.update_textures().empty()
    assert (h.lights()[0].tobytes(), h.lights()[1].tobytes(), h.stats()) == before


def test_an_emitters_texture_keeps_its_texels(vpt):
    """what the device refuses ("has no texels") the setters refuse first, from either side, so host and device stay in step"""
    h = vpt.HostScene(path(T.S03))
    before = h.stats()
    with pytest.raises(vpt.VptError):
        h.set_texture(T.SKY, np.zeros((0, 0, 4), np.uint8))   # the sky's slot, emptied
    h.set_texture(T.FLOOR, np.zeros((0, 0, 4), np.uint8))     # no environment names the floor: allowed
    with pytest.raises(vpt.VptError):
        h.set_environment(0, emission_tex=T.FLOOR)            # an emissive environment pointed at it
    h.set_environment(0, emission=(0.0, 0.0, 0.0), emission_tex=T.FLOOR)   # a dark one may
    with pytest.raises(vpt.VptError):
        h.set_environment(0, emission=(1.0, 1.0, 1.0))
    h.set_texture(T.FLOOR, vpt.HostScene(path(T.S03)).texture(T.FLOOR)[0])
    h.set_environment(0, emission=(0.5, 0.5, 0.5), emission_tex=T.SKY)
    assert not h.update_textures().empty() and h.stats() == before


def test_the_edit_carries_the_frame_at_hand_out(vpt):
    """set_environment, then set_environment_frame: the entry update_textures() hands out holds the later frame"""
    import scene_edits as E
    h = vpt.HostScene(path(T.S03))
    h.set_environment(0, emission=(0.25, 0.25, 0.25))
    E.rotate_environment(h, 0, 0.4)
    entry = h.update_textures().environments[0]
    frame = np.array(list(entry.frame.x) + list(entry.frame.y) + list(entry.frame.z) + list(entry.frame.o), F)
    assert frame.tobytes() == h.environment_frame(0).tobytes() and frame[0] != F(1)
    assert list(entry.emission) == [0.25, 0.25, 0.25]


def test_getters_return_copies(vpt):
    h = vpt.HostScene(path(T.S03))
    t, linear = h.texture(1)
    assert t.shape == (1024, 2048, 4) and t.dtype == np.float32 and linear
    t[:] = 0
    assert h.texture(1)[0].any()
    e = h.environment(0)
    assert list(e.emission) == [0.5, 0.5, 0.5] and e.emission_tex == 1
    e.emission_tex = 0
    assert h.environment(0).emission_tex == 1
    b, linear = h.texture(0)
    assert b.shape == (1024, 1024, 4) and b.dtype == np.uint8 and not linear


def test_texture_edit_abi(vpt):
    """two float textures and a byte one in one edit: offsets count texels inside the edit's own pools"""
    a, b, c = T.synthetic(5, 3, 1), T.synthetic(4, 2, 2), T.synthetic(9, 7, 3, np.uint8)
    edit = vpt.TextureEdit(textures={1: (a, True), 0: (c, False), 2: (b, False)})
    abi, keep = edit.to_abi()
    entries = (vpt.VptTexture * 3).from_address(abi.textures)
    assert [(t.width, t.height, t.linear, t.is_float, t.offset) for t in entries] == [(5, 3, 1, 1, 0), (9, 7, 0, 0, 0), (4, 2, 0, 1, 15)]
    assert (abi.num_textures, abi.num_texels_f, abi.num_texels_b, abi.num_environments) == (3, 23, 63, 0)
    assert edit.payload_bytes() == 23 * 16 + 63 * 4 + 3 * 24
    assert vpt.TextureEdit().empty() and not edit.empty()


NEW_SYMBOLS = ("vpt_scene_update_textures", "vpt_multi_update_textures", "vpt_session_edit_textures")


def test_symbols_and_declarations(vpt):
    header = open(os.path.join(ROOT, "include", "vpt.h")).read()
    for name in NEW_SYMBOLS:
        assert getattr(vpt.hip, name) is not None
        assert re.search(r"^int\s+%s\(" % name, header, re.M), name
    for name in ("vpth_scene_set_environment", "vpth_scene_set_texture", "vpth_scene_update_textures"):
        assert getattr(vpt.host, name) is not None
    # the struct older binaries fill in keeps its layout beside the new one
    assert "const float* const* shape_normals;     /* per entry: num_vertices float3 or NULL (keep); the array itself may be NULL    */\n} vpt_scene_edit;" in header
    assert "int vpt_scene_update_lights(vpt_scene* scene, const vpt_scene_edit* edit);" in header
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "volumetric-path-tracer_amd", "libvpt_hip.so")], capture_output=True, text=True)
    if nm.returncode == 0:
        exported = {line.split()[-1] for line in nm.stdout.splitlines() if line.strip()}
        assert set(NEW_SYMBOLS) <= exported


def test_null_arguments_need_no_device(vpt):
    """the argument checks that come before any device call"""
    assert vpt.hip.vpt_scene_update_textures(None, None) == -1
    assert vpt.hip.vpt_multi_update_textures(None, None) == -1
    assert vpt.hip.vpt_session_edit_textures(None, None) == -1
