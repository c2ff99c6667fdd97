"""Edits that change the lights, shared by the light-update tests (tests/test_light_update_host.py, tests/test_light_update_gpu.py),
the fixture script (tests/golden/make_light_edit_fixtures.py) and the measurements (profiles/tools/light_update_measure.py): each
takes a HostScene and changes it through its setters, like the cases of scene_edits.py that they build on.  Materials are named
as the scene files name them."""
import json
import os
import sys

import numpy as np

import scene_edits as E

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = os.path.join(HERE, "golden", "scenes")

S03 = "03_volume/volume.json"
LOBES = "03_volume_lobes/volume_lobes.json"
HEAD = "05_head1ss_sub/head1ss_sub.json"
CURVES = "09_curves_synth/curves.json"
GRID = "06_gridsdf_synth/gridsdf_synth.json"
SDFN = "07_sdfunction_synth/sdfunction_synth.json"

WARM = (3.0, 2.5, 2.0)   # the emission of 03_volume_lobes' glow


def index_of(scene_file, kind, name):
    """position of the item called `name` in the scene file's list `kind` (materials, shapes, instances)"""
    items = json.load(open(os.path.join(SCENES, scene_file)))[kind]
    return next(i for i, item in enumerate(items) if item.get("name") == name)


def emit(h, material, rgb):
    """emission of one material := rgb ((0, 0, 0): off)"""
    m = h.material(material)
    m.emission[0], m.emission[1], m.emission[2] = rgb
    h.set_material(material, m)


def switch_on(scene_file, name, rgb=WARM):
    return lambda h: emit(h, index_of(scene_file, "materials", name), rgb)


def switch_off(scene_file, *names):
    return lambda h: [emit(h, index_of(scene_file, "materials", n), (0.0, 0.0, 0.0)) for n in names]


def stretch(p):
    """x times 1.25 (a float32 product) on an (n, 3) float32 array: areas change with it"""
    p = np.array(p, E.F).copy()
    p[:, 0] = (p[:, 0] * E.F(1.25)).astype(E.F)
    return p


def nudge_shape(scene_file, name, formula=E.nudge):
    """formula (scene_edits.nudge) over the vertices of one shape; its normals stay"""
    def edit(h):
        s = index_of(scene_file, "shapes", name)
        h.set_shape_positions(s, formula(h.shape_positions(s)))
    return edit


def several(*edits):
    return lambda h: [e(h) for e in edits]


# name -> (scene file, edit(host scene)).  What each is there for:
#  vol_jade_on           6 144 quads become a LARGE_MESH light with index levels and a guide table; the feature bits change
#  vol_arealight1_off    a light leaves the list, the later ones move up
#  vol_on_off_move       both of the above and an instance moved, in one edit
#  vol_arealight1_nudge  the four vertices of a SMALL_MESH light stretched and nudged: its area, its record and light_prims
#  vol_meshes_off        every emissive material off: the environment alone remains, its CDF untouched
#  lobes_glow_nudge      the sphere all of 03_volume_lobes' meshes share, glow's among them: a large light whose shape moves
#  lobes_glow_off        a large light leaves, the feature bits change back
#  head_on               144 046 triangles on an all-triangle scene: the compact-record instance has to go
#  curves_hair_on        the material of a shape of lines: emissive when hit, never a light - the list stays
#  grid_sdf_on / _off, sdfn_sdf_on / _off   SDF lights come and go (K2)
CASES = {
    "vol_jade_on": (S03, switch_on(S03, "jade")),
    "vol_arealight1_off": (S03, switch_off(S03, "arealight1")),
    "vol_on_off_move": (S03, several(switch_on(S03, "jade"), switch_off(S03, "arealight1"), lambda h: E.translate(h, 1, dx=0.2))),
    "vol_arealight1_nudge": (S03, nudge_shape(S03, "arealight1", lambda p: E.nudge(stretch(p)))),
    "vol_meshes_off": (S03, switch_off(S03, "arealight1", "arealight2")),
    "lobes_glow_nudge": (LOBES, nudge_shape(LOBES, "sphere")),
    "lobes_glow_off": (LOBES, switch_off(LOBES, "glow")),
    "head_on": (HEAD, switch_on(HEAD, "material1")),
    "curves_hair_on": (CURVES, switch_on(CURVES, "hair_glossy")),
    "grid_sdf_on": (GRID, switch_on(GRID, "floor")),
    "grid_sdf_off": (GRID, switch_off(GRID, "arealight1")),
    "sdfn_sdf_on": (SDFN, switch_on(SDFN, "pbr")),
    "sdfn_sdf_off": (SDFN, switch_off(SDFN, "arealight1")),
}

# Cases the reference also renders (tests/golden/make_light_edit_fixtures.py -> light_edit_states.npz): name -> (shader, resolution,
# samples, bounces), the non-volumetric path tracer at the size of tests/cases.py's path_64_4.  The script measures on the
# reference's arithmetic the share of pixels stable under 1-ulp nudges of libm and refuses a case under 0.8; the first two are the
# candidates, the lobes cases the alternates.
STATE_CANDIDATES = {
    "vol_jade_on": ("pathtrace", 64, 4, 4), "vol_arealight1_off": ("pathtrace", 64, 4, 4),
    "lobes_glow_nudge": ("pathtrace", 64, 4, 4), "lobes_glow_off": ("pathtrace", 64, 4, 4),
}
STATE_WANTED = 2


def write_edited_scene(vpt, scene_file, edited, out):
    """the scene of `scene_file` as the HostScene `edited` holds it now - frames, moved vertices (make_update_fixtures) and the
    materials' emission - as a scene file under directory `out`; returns its path"""
    def emission(d):
        for i, m in enumerate(d["materials"]):
            rgb = [float(np.float32(c)) for c in edited.material(i).emission]
            if any(rgb) or "emission" in m:
                m["emission"] = rgb

    if "instances" not in json.load(open(os.path.join(SCENES, scene_file))):   # a scene of SDFs: nothing but materials to edit
        import pathlib
        return E.write_scene_variant(pathlib.Path(str(out)), os.path.join(SCENES, scene_file), emission)
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_update_fixtures
    path = make_update_fixtures.write_edited_scene(vpt, scene_file, edited, str(out))
    d = json.load(open(path))
    emission(d)
    json.dump(d, open(path, "w"))
    return path


def lights_of(stats):
    """the `lights` section of a stats() / --stats text or dictionary"""
    return (json.loads(stats) if isinstance(stats, str) else stats)["lights"]
