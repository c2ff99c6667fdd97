"""vpt_scene_update_textures on the GPU (include/vpt.h).  The criterion is equality of bits, no tolerance anywhere:
A = DeviceScene(original) after A.update_textures(edit) of every step of a case (tests/texture_edits.py) against B = a DeviceScene
made from the host scene after the same steps and update_textures().  The light list and CDF pool A holds must be the host mirror's
byte for byte, the six hashes of its light tables B's, the CDF searches B's, and every render (image as uint32, rngs, hits) B's."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import light_edits as L
import scene_edits as E
import texture_edits as T
from conftest import GOLDEN, ROOT
from test_light_update_gpu import assert_same_everything, shaders_of
from test_scene_update_gpu import render, same_state

pytestmark = pytest.mark.gpu


def path(scene_file):
    return os.path.join(GOLDEN, "scenes", scene_file)


@pytest.fixture(scope="module")
def originals(vpt):
    """scene file -> (host scene, its six hashes, its render per shader) of the unedited scenes, made once and never edited"""
    out = {}
    for scene_file in (T.S03, T.GRID):
        host = vpt.HostScene(path(scene_file))
        dev = vpt.DeviceScene(host, 0)
        out[scene_file] = (host, dev.light_tables_hash(), {s: render(vpt, dev, host, scene_file, s) for s in shaders_of(scene_file)})
    return out


def updated_pair(vpt, name, work):
    """(A, B, edited host scene, the TextureEdits)"""
    scene_file = T.cases(vpt)[name][0]
    A = vpt.DeviceScene(vpt.HostScene(path(scene_file)), 0)
    host = vpt.HostScene(path(scene_file))
    edits = T.apply(vpt, name, host, work, after_step=A.update_textures)
    assert all(not e.empty() for e in edits) and host.update_textures().empty()
    return A, vpt.DeviceScene(host, 0), host, edits


def lights_bytes(lights):
    """what a rebuild sends per light beside the edit (include/vpt.h): list entry 24, index header 56, record tag 4; 128 per
    environment light (its record); 4 per SDF light (its one CDF entry)"""
    return sum(84 + (128 if l["environment"] >= 0 else 0) + (4 if l["sdf"] >= 0 else 0) for l in lights)


@pytest.mark.parametrize("name", T.NAMES)
def test_update_textures_equals_a_fresh_scene(vpt, originals, tmp_path, name):
    A, B, host, edits = updated_pair(vpt, name, tmp_path)
    scene_file = T.cases(vpt)[name][0]
    print(f"{name}: {A.update_stats()} (launches, bytes, device ms); lights {A.get_lights()[0].tolist()}", flush=True)
    assert_same_everything(vpt, A, B, host, scene_file, name)
    _, hashes, renders = originals[scene_file]
    differs = A.light_tables_hash() != hashes or any(not same_state(render(vpt, A, host, scene_file, s), renders[s]) for s in shaders_of(scene_file))
    assert differs == (name not in T.NO_OPS), name


def test_dimming_the_sky_leaves_the_light_tables(vpt, originals, tmp_path):
    """0.5 -> 0.25: the list, the CDF and the record (frames, size, total) stay; the entry of the environment is all that is sent,
    nothing is launched, and the picture changes"""
    A, _, host, edits = updated_pair(vpt, "sky_dim", tmp_path)
    _, hashes, renders = originals[T.S03]
    assert A.light_tables_hash() == hashes
    launches, sent, _ = A.update_stats()
    assert launches == 0 and sent == edits[0].payload_bytes() == 112
    assert not same_state(render(vpt, A, host, T.S03, "pathtrace"), renders["pathtrace"])


def test_switching_the_sky_off_keeps_the_mesh_lights(vpt, originals, tmp_path):
    A, _, host, _ = updated_pair(vpt, "sky_off", tmp_path)
    lights, cdf = A.get_lights()
    assert [(int(l["instance"]), int(l["environment"])) for l in lights] == [(6, -1), (7, -1)] and len(cdf) == 2
    assert A.light_tables_hash() != originals[T.S03][1]


def test_off_then_on_returns_the_original(vpt, originals, tmp_path):
    A, _, host, _ = updated_pair(vpt, "sky_off_on", tmp_path)
    original, hashes, renders = originals[T.S03]
    assert A.light_tables_hash() == hashes and host.stats() == original.stats()
    for s, st in renders.items():
        assert same_state(st, render(vpt, A, original, T.S03, s)), s


@pytest.mark.parametrize("name,kind,cdf_len", [("sky_untextured", "const", 0), ("sky_to_floor", "tex", 1024 * 1024), ("sky_swap_hdri", "tex", 500000)])
def test_the_environments_entry_follows_its_texture(vpt, tmp_path, name, kind, cdf_len):
    A, B, host, _ = updated_pair(vpt, name, tmp_path)
    lights, _ = A.get_lights()
    assert int(lights[2]["environment"]) == 0 and int(lights[2]["cdf_len"]) == cdf_len
    assert A.selftest_light_cdf(2, 1 << 16) == (0, 0 if kind == "const" else 2)


def test_a_texture_no_light_reads_launches_nothing(vpt, originals, tmp_path):
    A, _, host, edits = updated_pair(vpt, "floor_repaint", tmp_path)
    launches, sent, _ = A.update_stats()
    assert launches == 0 and sent == edits[0].payload_bytes() == 1024 * 1024 * 4 + 24
    assert A.light_tables_hash() == originals[T.S03][1]


def test_bytes_of_the_repaint(vpt, tmp_path):
    """the edit's texels and entry, one float per row of the sky, and the words per light of a rebuild (lights_bytes) with one
    recomputed CDF (job 24 + result 8): exactly, nothing else is sent"""
    A, _, host, edits = updated_pair(vpt, "sky_repaint", tmp_path)
    launches, sent, ms = A.update_stats()
    lights, _ = A.get_lights()
    print(f"sky_repaint: {launches} launches, {sent} bytes, {ms:.3f} ms on the device", flush=True)
    assert edits[0].payload_bytes() == 2048 * 1024 * 16 + 24
    assert sent == edits[0].payload_bytes() + 1024 * 4 + lights_bytes(lights) + 32
    assert launches == 5   # weights, running sum, index levels, guide table, records


@pytest.mark.parametrize("name,indexed", [("sky_1x1", 0), ("sky_5x3", 0), ("sky_16x4", 0), ("sky_13x5", 2), ("sky_67x33", 2), ("sky_bytes_9x7", 0),
                                          ("sky_negative_texel", 0), ("sky_nan_texel", 0)])
def test_search_structures_at_the_edges(vpt, tmp_path, name, indexed):
    """no index up to 64 entries and for a CDF that is not non-decreasing (a negative or a NaN texel), as at creation"""
    A, B, host, _ = updated_pair(vpt, name, tmp_path)
    assert A.selftest_light_cdf(2, 1 << 16) == B.selftest_light_cdf(2, 1 << 16) == (0, indexed)


@pytest.mark.parametrize("name", ["sky_swap_hdri", "sky_13x5"])
def test_the_plain_running_sum_gives_the_same_bits(name):
    """VPT_LIGHTS_PLAIN=1 in a child process, as the existing tests of such switches do"""
    env = dict(os.environ, VPT_LIGHTS_PLAIN="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", f"{__file__}::test_update_textures_equals_a_fresh_scene[{name}]"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("textures_first", [True, False])
def test_other_updates_on_the_same_handle(vpt, tmp_path, textures_first):
    """update_textures, then update_lights (jade switched on) and update (an instance moved) - and the reverse order"""
    A = vpt.DeviceScene(vpt.HostScene(path(T.S03)), 0)
    host = vpt.HostScene(path(T.S03))

    def textures():
        T.apply(vpt, "sky_67x33", host, tmp_path, after_step=A.update_textures)

    def others():
        L.CASES["vol_jade_on"][1](host)
        A.update_lights(host.update_lights())
        E.translate(host, 1, dx=0.2)
        E.rotate_environment(host, 0, 0.4)
        A.update(host.update_bvh())

    for step in ((textures, others) if textures_first else (others, textures)):
        step()
    T.apply(vpt, "sky_dim", host, tmp_path, after_step=A.update_textures)   # an edit that rebuilds nothing sees the handle's state too
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, T.S03, f"textures {'first' if textures_first else 'last'}")


def test_an_entry_carries_the_frame_the_scene_holds_when_the_edit_is_handed_out(vpt):
    """environment set, frame set, update, then update_textures: the entry of the TextureEdit replaces the frame too, and must not
    bring back the one the scene held when set_environment was called"""
    A = vpt.DeviceScene(vpt.HostScene(path(T.S03)), 0)
    host = vpt.HostScene(path(T.S03))
    host.set_environment(0, emission=(0.25, 0.25, 0.25))
    E.rotate_environment(host, 0, 0.4)
    A.update(host.update_bvh())
    A.update_textures(host.update_textures())
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, T.S03, "frame set after the environment")


def test_a_turned_frame_in_the_texture_edit_alone(vpt, originals):
    """the frame reaches the device through the TextureEdit only, emission unchanged: no rebuild, the entry with its inverse frame
    (112 bytes) and the two frames of the textured environment's record (96)"""
    A = vpt.DeviceScene(vpt.HostScene(path(T.S03)), 0)
    host = vpt.HostScene(path(T.S03))
    E.rotate_environment(host, 0, 0.4)
    host.set_environment(0)
    edit = host.update_textures()
    assert list(edit.environments) == [0] and not edit.textures
    A.update_textures(edit)
    assert A.update_stats()[:2] == (0, 112 + 96)
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, T.S03, "frame through the texture edit")
    _, hashes, renders = originals[T.S03]
    assert A.light_tables_hash() != hashes and A.light_tables_hash()[:2] == hashes[:2]   # the record, not the list or the CDF
    assert not same_state(render(vpt, A, host, T.S03, "pathtrace"), renders["pathtrace"])


def raw_edit(vpt, environments=(), textures=(), texels_f=None, texels_b=None):
    """a VptTextureEdit from lists of (id, struct), for what TextureEdit cannot express (repeated ids, offsets)"""
    keep, abi = [], vpt.VptTextureEdit()
    for ids, T_, count, idp, ptr in ((environments, vpt.VptEnvironment, "num_environments", "environment_ids", "environments"),
                                    (textures, vpt.VptTexture, "num_textures", "texture_ids", "textures")):
        a = np.array([i for i, _ in ids], np.int32)
        s = (T_ * max(1, len(ids)))(*[v for _, v in ids])
        keep += [a, s]
        setattr(abi, count, len(ids)), setattr(abi, idp, a.ctypes.data), setattr(abi, ptr, C.cast(s, C.c_void_p).value)
    for pool, count, ptr in ((texels_f, "num_texels_f", "texels_f"), (texels_b, "num_texels_b", "texels_b")):
        if pool is not None:
            keep.append(pool)
            setattr(abi, count, len(pool)), setattr(abi, ptr, pool.ctypes.data)
    return abi, keep


def test_refused_edits_leave_the_scene_untouched(vpt, originals):
    host, hashes, renders = originals[T.S03]
    A = vpt.DeviceScene(vpt.HostScene(path(T.S03)), 0)

    def environment(emission=None, emission_tex=None, frame_x0=None):
        e = host.environment(0)
        if emission is not None:
            e.emission[0], e.emission[1], e.emission[2] = emission
        if emission_tex is not None:
            e.emission_tex = emission_tex
        if frame_x0 is not None:
            e.frame.x[0] = frame_x0
        return e
    f8, b4 = np.zeros((8, 4), np.float32), np.zeros((4, 4), np.uint8)
    tex = vpt.VptTexture
    refused = [
        (raw_edit(vpt, environments=[(1, environment())]), "environment entry 0: id 1 out of range"),
        (raw_edit(vpt, environments=[(0, environment()), (0, environment())]), "environment entry 1: id 0 repeated"),
        (raw_edit(vpt, environments=[(0, environment(emission=(1.0, float("nan"), 1.0)))]), "environment entry 0: a value is not finite"),
        (raw_edit(vpt, environments=[(0, environment(frame_x0=float("inf")))]), "environment entry 0: a value is not finite"),
        (raw_edit(vpt, environments=[(0, environment(emission_tex=2))]), "environment entry 0: emission_tex 2"),
        (raw_edit(vpt, environments=[(0, environment(emission_tex=-2))]), "environment entry 0: emission_tex -2"),
        (raw_edit(vpt, textures=[(2, tex(2, 2, 1, 1, 0))], texels_f=f8), "texture entry 0: id 2 out of range"),
        (raw_edit(vpt, textures=[(1, tex(2, 2, 1, 1, 0)), (1, tex(2, 2, 1, 1, 4))], texels_f=f8), "texture entry 1: id 1 repeated"),
        (raw_edit(vpt, textures=[(1, tex(-2, 2, 1, 1, 0))], texels_f=f8), "texture entry 0: negative width or height"),
        (raw_edit(vpt, textures=[(1, tex(3, 3, 1, 1, 0))], texels_f=f8), "texture entry 0: texels out of range"),
        (raw_edit(vpt, textures=[(1, tex(2, 2, 1, 1, 5))], texels_f=f8), "texture entry 0: texels out of range"),
        (raw_edit(vpt, textures=[(0, tex(2, 2, 0, 0, 1))], texels_b=b4), "texture entry 0: texels out of range"),
        (raw_edit(vpt, textures=[(1, tex(0, 0, 1, 1, 0))], texels_f=f8), "environment 0: its emission texture 1 has no texels"),
    ]
    for (abi, keep), text in refused:
        assert vpt.hip.vpt_scene_update_textures(A.handle, C.byref(abi)) == -1, text
        assert text in vpt.hip.vpt_last_error().decode(), (vpt.hip.vpt_last_error().decode(), text)
        assert A.light_tables_hash() == hashes, text
    for s, st in renders.items():
        assert same_state(st, render(vpt, A, host, T.S03, s)), s
    # a texture a material uses may be edited, and an empty edit is no error
    assert vpt.hip.vpt_scene_update_textures(A.handle, C.byref(raw_edit(vpt)[0])) == 0
    assert A.light_tables_hash() == hashes


def test_session_edit_textures(vpt, tmp_path):
    """RenderSession.edit_textures equals a session on a fresh scene: the preview, then 3 + 5 samples; a refused edit leaves it"""
    host = vpt.HostScene(path(T.S03))
    p = vpt.PathtraceParams(resolution=96, samples=64, shader="pathtrace", bounces=4)
    s1 = vpt.RenderSession(vpt.DeviceScene(vpt.HostScene(path(T.S03)), 0), p)
    s1.advance(2)
    T.apply(vpt, "sky_67x33", host, tmp_path, after_step=s1.edit_textures)
    s2 = vpt.RenderSession(vpt.DeviceScene(host, 0), p)
    assert s1.samples == s2.samples == 0
    assert np.array_equal(s1.display(), s2.display())   # the preview both show after a reset
    for step in (3, 5):
        s1.advance(step), s2.advance(step)
        assert s1.samples == s2.samples
        assert same_state(s1.state(), s2.state()), step
        assert np.array_equal(s1.display(), s2.display()), step
    bad = host.environment(0)
    bad.emission_tex = 7
    with pytest.raises(vpt.VptError):
        s1.edit_textures(vpt.TextureEdit(environments={0: bad}))
    assert s1.samples == 8 and same_state(s1.state(), s2.state())


def test_multi_update_textures_on_one_device(vpt, tmp_path):
    host = vpt.HostScene(path(T.S03))
    M = vpt.MultiDeviceScene(vpt.HostScene(path(T.S03)), [0])
    T.apply(vpt, "sky_to_floor", host, tmp_path, after_step=M.update_textures)
    B = vpt.DeviceScene(host, 0)
    p = vpt.PathtraceParams(resolution=64, samples=8, shader="volpathtrace", bounces=8)
    want = host.make_state(p)
    B.pathtrace_samples(want, p, 8)
    got = host.make_state(p)
    M.pathtrace_samples(got, p, 8)
    assert same_state(got, want)


# ---- end to end against the reference: its own render of the edited scene (tests/golden/texture_edit_states.npz) ---------------------
def _state_cases():
    f = os.path.join(GOLDEN, "texture_edit_stats.json")
    return {k: v["state"] for k, v in (json.load(open(f)) if os.path.exists(f) else {}).items() if "state" in v}


def test_reference_state_fixtures_are_there():
    assert len(_state_cases()) >= T.STATE_WANTED and set(_state_cases()) <= set(T.STATE_CANDIDATES)


@pytest.mark.parametrize("name", sorted(_state_cases()))
def test_update_textures_matches_the_references_render(vpt, oracle, tmp_path, name):
    """the check of test_light_update_gpu on a handle whose environment was REBUILT to the edited scene, against the reference's state
    of that scene: floors 0.998 on identical streams and matching pixels, and on the stable share 0.02 under what the fixture script
    measured on the reference's arithmetic"""
    from test_gpu_parity import _check_against_reference
    case = _state_cases()[name]
    A, _, host, _ = updated_pair(vpt, name, tmp_path)
    gold = np.load(os.path.join(GOLDEN, "texture_edit_states.npz"))
    p = vpt.PathtraceParams(resolution=case["resolution"], samples=case["samples"], shader=case["shader"], bounces=case["bounces"])
    g = host.make_state(p)
    A.pathtrace_samples(g, p, case["samples"])
    assert case["stable_share"] >= 0.8
    _check_against_reference(oracle, host, p, case["samples"], g, gold[name + "_image"], gold[name + "_rngs"], name, 0.998, 0.998, case["stable_share"] - 0.02)
