"""Edits of environments and textures, shared by the texture-update tests (tests/test_texture_update_host.py,
tests/test_texture_update_gpu.py), the fixture script (tests/golden/make_texture_edit_fixtures.py) and the measurements
(profiles/tools/texture_update_measure.py).  A case is (scene file, [step, ...]): every step takes a HostScene and a work directory
(a pathlib.Path, for the steps that read an image file) and changes the scene through set_environment / set_texture; the caller
runs update_textures() after each step.  Synthetic texels come from a seeded generator; texels of a file come through the
project's own loader, from a one-texture scene written to the work directory.

03_volume: texture 0 = floor.png (1024 x 1024 bytes, the floor's colour), texture 1 = sky.hdr (2048 x 1024 floats, the sky's
emission).  06_gridsdf_synth (K2): texture 0 = the same sky, on its one environment."""
import json
import os
import re

import numpy as np

import scene_edits as E

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = os.path.join(HERE, "golden", "scenes")
S03 = "03_volume/volume.json"
GRID = "06_gridsdf_synth/gridsdf_synth.json"
F = np.float32
FLOOR, SKY = 0, 1   # textures of 03_volume


def file_texels(vpt, work, uri):
    """(texels, linear) of the image file tests/golden/scenes/<uri> as the scene loader reads it"""
    folder = work / ("texture_" + os.path.basename(uri).replace(".", "_"))
    folder.mkdir(exist_ok=True)
    link = folder / os.path.basename(uri)
    if not link.exists():
        os.symlink(os.path.join(SCENES, uri), link)
    scene = {"asset": {"version": "4.2"}, "cameras": [{"name": "default", "aspect": 1.0}], "textures": [{"name": "t", "uri": os.path.basename(uri)}]}
    (folder / "scene.json").write_text(json.dumps(scene))
    return vpt.HostScene(str(folder / "scene.json")).texture(0)


def synthetic(width, height, seed, dtype=F):
    """(height, width, 4) texels: floats in [0, 4) with alpha 1 (an HDR sky's range), or bytes"""
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (height, width, 4), dtype=np.uint8)
    t = (rng.random((height, width, 4), dtype=F) * F(4)).astype(F)
    t[..., 3] = F(1)
    return t


def emission(rgb, environment=0):
    return lambda h, work: h.set_environment(environment, emission=rgb)


def emission_tex(texture, environment=0):
    return lambda h, work: h.set_environment(environment, emission_tex=texture)


def texels(texture, make):
    """texture := make() (its linear flag stays)"""
    return lambda h, work: h.set_texture(texture, make())


def swap_hdri(vpt_module):
    def step(h, work):
        t, _ = file_texels(vpt_module, work, "shared_textures/texture2.hdr")
        h.set_texture(SKY, t)
    return step


def repaint_sky(h, work):
    """a rectangle of the sky times 4, a float32 product per channel: the same size, so the overwrite is in place"""
    t, _ = h.texture(SKY)
    t[200:420, 300:900, :3] = (t[200:420, 300:900, :3] * F(4)).astype(F)
    h.set_texture(SKY, t)


def repaint_floor(h, work):
    t, _ = h.texture(FLOOR)
    h.set_texture(FLOOR, synthetic(t.shape[1], t.shape[0], 5, np.uint8))


def with_texel(width, height, seed, *changes):
    """the synthetic texture with t[at] = value for every (at, value)"""
    def make():
        t = synthetic(width, height, seed)
        for at, value in changes:
            t[at] = value
        return t
    return make


# (width, height) of the synthetic skies around the edges of the running sum's blocks and of the index: 15 entries are below one
# block of 64; 64 are exactly one block and get no index (more than 64 are needed); 65 cross the first block boundary and are the
# first indexed length, with 65 / 4 = 16 buckets, the smallest guide table there is; 2211 have odd rows and several index levels.
SIZES = {"sky_1x1": (1, 1), "sky_5x3": (5, 3), "sky_13x5": (13, 5), "sky_16x4": (16, 4), "sky_67x33": (67, 33)}


def cases(vpt):
    """name -> (scene file, [step, ...])"""
    out = {
        "sky_dim": (S03, [emission((0.25, 0.25, 0.25))]),
        "sky_off": (S03, [emission((0.0, 0.0, 0.0))]),
        "sky_off_on": (S03, [emission((0.0, 0.0, 0.0)), emission((0.5, 0.5, 0.5))]),
        "sky_untextured": (S03, [emission_tex(-1)]),
        "sky_to_floor": (S03, [emission_tex(FLOOR)]),
        "sky_swap_hdri": (S03, [swap_hdri(vpt)]),
        "sky_repaint": (S03, [repaint_sky]),
        "floor_repaint": (S03, [repaint_floor]),
        "sky_bytes_9x7": (S03, [texels(SKY, lambda: synthetic(9, 7, 97, np.uint8))]),
        "sky_negative_texel": (S03, [texels(SKY, with_texel(67, 33, 6733, ((11, 23), (-1.0, -1.0, -1.0, -1.0))))]),
        # a NaN in y under the largest x: the select form drops both (max(x, NaN) = NaN, max(NaN, z) = z), fmaxf would keep x;
        # a NaN in alpha, the last operand, stays: the CDF is NaN from that texel on
        "sky_nan_texel": (S03, [texels(SKY, with_texel(67, 33, 6733, ((20, 5), (3.9, np.nan, 0.5, 1.0)), ((28, 40, 3), np.nan)))]),
        "grid_sky_13x5": (GRID, [texels(0, lambda: synthetic(13, 5, 135))]),   # the K2 scene has a texture slot: its sky is replaced
    }
    for name, (w, h) in SIZES.items():
        out[name] = (S03, [texels(SKY, lambda w=w, h=h: synthetic(w, h, 100 * w + h))])
    return out


NAMES = ["sky_dim", "sky_off", "sky_off_on", "sky_untextured", "sky_to_floor", "sky_swap_hdri", "sky_repaint", "floor_repaint", "sky_bytes_9x7",
         "sky_negative_texel", "sky_nan_texel", "grid_sky_13x5"] + list(SIZES)
NO_OPS = ("sky_off_on",)            # constructed to return to the original
LARGE = ("sky_repaint", "sky_swap_hdri")   # the only cases whose recomputed CDF is large


def apply(vpt, name, h, work, after_step=None):
    """every step of a case on HostScene h, update_textures() after each; after_step(edit) sees each TextureEdit.  Returns the edits."""
    edits = []
    for step in cases(vpt)[name][1]:
        step(h, work)
        edits.append(h.update_textures())
        if after_step:
            after_step(edits[-1])
    return edits


# ---- the cases a scene file can express: the edited scene written out, for a fresh load and for the reference ------------------
def _environment(**values):
    def change(d):
        for k, v in values.items():
            if v is None:
                d["environments"][0].pop(k, None)
            else:
                d["environments"][0][k] = v
    return change


def _sky_uri(d):
    d["textures"][SKY]["uri"] = "../shared_textures/texture2.hdr"


AS_SCENE_FILE = {
    "sky_dim": _environment(emission=[0.25, 0.25, 0.25]),
    "sky_off": _environment(emission=[0.0, 0.0, 0.0]),
    "sky_untextured": _environment(emission_tex=None),
    "sky_to_floor": _environment(emission_tex=FLOOR),
    "sky_swap_hdri": _sky_uri,
}

# Cases the reference also renders (tests/golden/make_texture_edit_fixtures.py -> texture_edit_states.npz): name -> (shader,
# resolution, samples, bounces), the size of tests/cases.py's path_64_4.  The script keeps light_edits' rule: the share of pixels
# stable under 1-ulp nudges of libm must reach 0.8, and it takes the first STATE_WANTED candidates that do.
STATE_CANDIDATES = {"sky_to_floor": ("pathtrace", 64, 4, 4), "sky_swap_hdri": ("pathtrace", 64, 4, 4), "sky_dim": ("pathtrace", 64, 4, 4),
                    "sky_untextured": ("pathtrace", 64, 4, 4)}
STATE_WANTED = 2


def write_edited_scene(name, out):
    """the scene file of an AS_SCENE_FILE case under directory `out` (a pathlib.Path); returns its path"""
    return E.write_scene_variant(out, os.path.join(SCENES, S03), AS_SCENE_FILE[name])


def lights_of(stats):
    """the `lights` section of a stats() text or dictionary (a CDF that ends in NaN prints as C does: nan)"""
    return (json.loads(re.sub(r"-?nan\b", "NaN", stats)) if isinstance(stats, str) else stats)["lights"]
