"""Cases shared by the instance-edit tests (tests/test_instance_update_host.py, tests/test_instance_update_gpu.py) and their fixture
script (tests/golden/make_instance_edit_fixtures.py): name -> Case(scene, steps).  A step changes a HostScene through add_instance /
remove_instances / set_instance; the caller hands the pending changes out with update_instances() after every step.
Every frame of a case is made of dyadic values - multiples of 1/64, quarter turns, mirrors, non-uniform scales such as 0.5 / 1.25 / 2 -
so a scene file written as text reads back bit for bit whatever a loader does between text and float.
Every case but round_trip changes the scene BVH's integer fields or node count: the host test asserts it."""
import json
import os

import numpy as np

import synth_scenes

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = os.path.join(HERE, "golden", "scenes")
S03 = "03_volume/volume.json"
CURVES = "09_curves_synth/curves.json"
# crowd_scene: its shapes and materials in the order synth_scenes writes them
TRI_LEAF, QUAD_LEAF, BLOB, GRID_QUADS, GRID_TRIS, LAMP_SMALL, LAMP_LARGE = range(7)
GREY, RED, MAT_LAMP_SMALL, MAT_LAMP_LARGE = range(4)
PLAIN = (TRI_LEAF, QUAD_LEAF, BLOB, GRID_QUADS, GRID_TRIS)
SPHERE, SMOKE = 1, 3   # 03_volume: the shape its five media share, the volumetric material


class Case:
    def __init__(self, scene, steps):
        self.scene, self.steps = scene, steps

    def path(self, tmp_path):
        """the scene file: a golden scene, or a synthetic one written into tmp_path"""
        if callable(self.scene):
            return self.scene(tmp_path)
        return os.path.join(SCENES, self.scene)


def crowd(count):
    return lambda tmp_path: synth_scenes.crowd_scene(str(tmp_path), count)[0]


# ---- dyadic frames ---------------------------------------------------------------------------------------------------------------------
QUARTER_TURNS = [np.eye(3), [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[1, 0, 0], [0, 0, -1], [0, 1, 0]], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],
                 [[-1, 0, 0], [0, -1, 0], [0, 0, 1]], [[0, 1, 0], [0, 0, 1], [1, 0, 0]]]
SCALES = [(0.25, 0.25, 0.25), (0.5, 0.25, 0.125), (0.125, 0.3125, 0.25), (0.25, -0.25, 0.25), (0.1875, 0.1875, 0.375)]


def frame(turn=0, scale=(1, 1, 1), o=(0, 0, 0)):
    """x, y, z, o of a quarter turn times a diagonal (a negative entry mirrors), every value a small multiple of 1/64"""
    m = np.asarray(QUARTER_TURNS[turn % len(QUARTER_TURNS)], np.float64) @ np.diag(scale)
    f = np.concatenate([m[:, 0], m[:, 1], m[:, 2], np.asarray(o, np.float64)]).astype(F)
    assert np.array_equal(f * F(64), np.round(f * F(64))), f
    return f


def scatter(k):
    """the k-th frame of a crowd: a position on a 1/64 lattice inside the crowd's extent, a quarter turn, a scale"""
    o = (((k * 37) % 129 - 64) / 64, ((k * 53) % 97 - 48) / 64, ((k * 29) % 113 - 56) / 64)
    return frame(k, SCALES[k % len(SCALES)], o)


# ---- steps -----------------------------------------------------------------------------------------------------------------------------
def remove_mid(h):
    h.remove_instances([5, 6, 40])


def remove_lamp(h):
    h.remove_instances([0])


def add_lit_grid(h):
    h.add_instance(frame(2, (0.5, 0.5, 0.5), (-0.75, 0.25, 0.5)), GRID_QUADS, MAT_LAMP_LARGE)


def grow(h):
    for k in range(200):
        h.add_instance(scatter(k), PLAIN[(k * 3) % 5], k % 2)


def set_three(h):
    # (another shape alone leaves this crowd's topology as it is: the instance also moves, so that the build differs)
    h.set_instance(7, frame=frame(4, (0.5, 0.5, 0.5), (1, -0.75, 0.5)), shape=BLOB if h.instance_ids(7)[0] != BLOB else GRID_TRIS)
    h.set_instance(9, material=MAT_LAMP_SMALL)
    h.set_instance(1, material=GREY)


def all_three(h):
    """one edit: instance 12 re-pointed and moved, 3 made emissive; 0 (the small lamp), 13 and 69 removed; four added, one of them lit"""
    h.set_instance(12, frame=frame(3, (0.25, 0.5, 0.25), (0.5, -0.25, 0.125)), shape=QUAD_LEAF, material=RED)
    h.set_instance(3, material=MAT_LAMP_SMALL)
    h.remove_instances([0, 13, 69])
    for k in range(3):
        h.add_instance(scatter(100 + k), PLAIN[k], k % 2)
    h.add_instance(frame(1, (0.25, 0.25, 0.25), (0.75, 0.5, -0.5)), LAMP_SMALL, MAT_LAMP_SMALL)


def vol_add_remove(h):
    h.remove_instances([h.count("instances") - 1])
    h.add_instance(frame(0, (0.5, 0.5, 0.5), (-0.625, 0.0625, 0.375)), SPHERE, 0)       # the floor's textured material
    h.add_instance(frame(1, (0.75, 0.5, 0.75), (0.625, 0.0625, 0.375)), SPHERE, SMOKE)


def curve_shapes(h):
    """the shapes of lines and of points"""
    return [s for s in range(h.count("shapes")) if len(h.shape_arrays(s)["lines"]) or len(h.shape_arrays(s)["points"])]


def curves_off(h):
    curved = set(curve_shapes(h))
    h.remove_instances([i for i in range(h.count("instances")) if h.instance_ids(i)[0] in curved])


def curves_on(h):
    lines = next(s for s in range(h.count("shapes")) if len(h.shape_arrays(s)["lines"]))
    points = next(s for s in range(h.count("shapes")) if len(h.shape_arrays(s)["points"]))
    h.add_instance(frame(0, (1, 1, 1), (-0.25, 0, 0.0625)), lines, 2)
    h.add_instance(frame(0, (1, 1.25, 1), (0.125, 0, -0.125)), points, 5)


def add_three(h):
    for k in range(3):
        h.add_instance(scatter(40 + k), PLAIN[k + 1], k % 2)


def remove_last_three(h):
    n = h.count("instances")
    h.remove_instances([n - 3, n - 2, n - 1])


CASES = {
    "crowd_remove_mid": Case(crowd(70), [remove_mid]),
    "crowd_remove_lamp": Case(crowd(70), [remove_lamp]),
    "crowd_add_lit_grid": Case(crowd(70), [add_lit_grid]),
    "crowd_grow": Case(crowd(16), [grow]),
    "crowd_set": Case(crowd(70), [set_three]),
    "crowd_all_three": Case(crowd(70), [all_three]),
    "vol_add_remove": Case(S03, [vol_add_remove]),
    "curves_off_on": Case(CURVES, [curves_off, curves_on]),
    "round_trip": Case(crowd(70), [add_three, remove_last_three]),
}


def apply(h, case, after=None):
    """every step of `case` on HostScene h; after(InstanceEdit) sees what the device is to be given"""
    for step in case.steps:
        step(h)
        edit = h.update_instances()
        if after:
            after(edit)


def scene_fields(h):
    """the scene BVH's integer fields, node count and primitive order"""
    a, _ = h.bvh_nodes()
    return ([a[k].tobytes() for k in ("start", "num", "axis", "internal")], len(a), h.bvh_prims()[0].tobytes())


def instances_of(h) -> np.ndarray:
    """the host scene's instances as the INSTANCE array DeviceScene.get_instances returns"""
    import vpt_loader
    vpt = vpt_loader.load()
    out = np.zeros(h.count("instances"), vpt.INSTANCE)
    for i in range(len(out)):
        out[i] = (h.instance_frame(i), *h.instance_ids(i))
    return out


def write_edited_scene(source, edited, out):
    """the scene file `source` with its instance array rewritten as the HostScene `edited` holds it, under directory `out`; every
    other item as it is, uris made relative to `out`.  Returns the path."""
    src_dir = os.path.dirname(source)
    d = json.load(open(source))
    os.makedirs(out, exist_ok=True)
    d["instances"] = [{"name": f"i{i}", "shape": int(s), "material": int(m), "frame": [float(x) for x in fr]}
                      for i, (fr, s, m) in enumerate((edited.instance_frame(i), *edited.instance_ids(i)) for i in range(edited.count("instances")))]
    for key in ("shapes", "textures", "subdivs", "volumes"):
        for item in d.get(key, []):
            if "uri" in item:
                item["uri"] = os.path.relpath(os.path.join(src_dir, item["uri"]), out)
    path = os.path.join(out, "edited.json")
    json.dump(d, open(path, "w"))
    return path
