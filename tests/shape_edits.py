"""Cases shared by the shape-edit tests (tests/test_shape_update_host.py, tests/test_shape_update_gpu.py) and their fixture script
(tests/golden/make_shape_edit_fixtures.py): name -> Case(scene, steps).  A step is ("shapes", f) or ("instances", f): f changes a
HostScene through add_shape / set_shape / remove_shapes, or through the instance setters of tests/instance_edits.py; the caller hands
the pending changes out with update_shapes() / update_instances() after every step.
New geometry is float32 from the start and is written as binary PLY, so a loader gives it back bit for bit; new texcoords are
multiples of 1/64, because the loaders flip v (1 - v is exact there); new frames are instance_edits' dyadic ones.
Every case changes the integer fields or counts of some shape BVH: the host test asserts it."""
import json
import os
import struct

import numpy as np

import instance_edits as I
import light_shapes
import synth_scenes

F = np.float32
SCENES = I.SCENES
S03, CURVES = I.S03, I.CURVES
TRI_LEAF, QUAD_LEAF, BLOB, GRID_QUADS, GRID_TRIS, LAMP_SMALL, LAMP_LARGE = range(7)   # crowd_scene's shapes
TRI_T, BLOB_T, GRID_T, LAMP_T = range(4)                                               # tri_scene's
SPHERE, AREALIGHT1 = 1, 2                                                              # 03_volume's
HAIR = 2                                                                               # curves.json: its line shape


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


def tri_scene(tmp_path):
    """a scene whose shapes all hold triangles (the compact records exist): a leaf, a blob, a grid and a lamp of two triangles"""
    w = synth_scenes._Writer(str(tmp_path))
    rng = np.random.default_rng(11)
    shapes = [w.shape("tri_leaf", [[-1, -1, 0], [1, -1, 0], [0, 1, 0.3], [0, 0, 1]], [[0, 1, 2], [0, 1, 3], [1, 2, 3]]),
              w.shape("blob", *synth_scenes._blob(rng, 40)), w.shape("grid_tris", *synth_scenes._grid(5, False))]
    lamp = w.shape("lamp", [[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], [[0, 1, 2], [0, 2, 3]])
    w.instance(lamp, I.frame(2, (0.25, 0.25, 0.25), (0, 0.75, 0)), 2)
    for k in range(12):
        w.instance(shapes[k % 3], I.scatter(k), k % 2)
    return w.write("tris", synth_scenes._look_at([0.4, 0.5, 4.2], [0, 0, 0]))[0]


# ---- geometry: float32, small ------------------------------------------------------------------------------------------------------------
def blob(n, seed=3, scale=1.0):
    v, f = synth_scenes._blob(np.random.default_rng(seed), n)
    return dict(positions=(v * scale).astype(F), triangles=f.astype(np.int32))


def grid(n, quads=True):
    v, f = synth_scenes._grid(n, quads)
    return dict(positions=v.astype(F), **{"quads" if quads else "triangles": f.astype(np.int32)})


def lamp(n, quads=True):
    """n elements of tests/light_shapes.py: varied areas over three decades, centred on the origin"""
    v, f = light_shapes.geometry(light_shapes.Case(f"lamp_{n}", n, quads=quads))
    return dict(positions=((v - F(0.5)) * F(2)).astype(F), **{"quads" if quads else "triangles": f.astype(np.int32)})


def with_attributes(m, seed=7):
    """normals (unit, float32) and texcoords (multiples of 1/64) for a mesh"""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(len(m["positions"]), 3))
    return dict(m, normals=(n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F), texcoords=(rng.integers(0, 65, (len(m["positions"]), 2)) / 64).astype(F))


def points(n, seed=5):
    rng = np.random.default_rng(seed)
    return dict(positions=rng.uniform(-1, 1, (n, 3)).astype(F), points=np.arange(n, dtype=np.int32), radius=rng.uniform(0.02, 0.08, n).astype(F))


def strands(count, verts, seed=9):
    """`count` polylines of `verts` vertices with radii thinning to the tip"""
    rng = np.random.default_rng(seed)
    s = np.linspace(0, 1, verts)
    roots, bend = rng.uniform(-0.3, 0.3, (count, 2)), rng.uniform(-0.4, 0.4, (count, 2))
    pos = np.zeros((count, verts, 3))
    pos[:, :, 0] = roots[:, None, 0] + bend[:, None, 0] * 0.5 * s ** 2
    pos[:, :, 1] = 0.5 * s[None, :]
    pos[:, :, 2] = roots[:, None, 1] + bend[:, None, 1] * 0.5 * s ** 2
    lines = np.array([[c * verts + k, c * verts + k + 1] for c in range(count) for k in range(verts - 1)], np.int32)
    radius = np.tile(0.012 * (1 - 0.8 * s), count)
    return dict(positions=pos.reshape(-1, 3).astype(F), lines=lines, radius=radius.astype(F))


def instances_of_shape(h, shape):
    return [i for i in range(h.count("instances")) if h.instance_ids(i)[0] == shape]


# ---- steps -----------------------------------------------------------------------------------------------------------------------------
def shapes(f):
    return ("shapes", f)


def instances(f):
    return ("instances", f)


def set_to(shape, make):
    return shapes(lambda h: h.set_shape(shape, **make()))


def drop_instances(shape):
    return instances(lambda h: h.remove_instances(instances_of_shape(h, shape)))


def add_two(h):
    h.add_shape(positions=np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0.25]], F), triangles=[[0, 1, 2]])
    h.add_shape(**blob(300, seed=21))


def instance_the_last_two(h):
    n = h.count("shapes")
    h.add_instance(I.frame(1, (0.25, 0.25, 0.25), (0.5, 0.25, -0.5)), n - 2, I.RED)
    h.add_instance(I.frame(3, (0.5, 0.25, 0.5), (-0.5, -0.25, 0.25)), n - 1, I.GREY)
    h.add_instance(I.frame(0, (0.25, 0.25, 0.25), (0.25, -0.5, 0.5)), n - 1, I.MAT_LAMP_LARGE)   # and a light on a new shape


def all_three(h):
    """one edit: the grid of triangles replaced by 50 triangles with normals and texcoords, the quad leaf (its instances are gone)
    removed, a grid of 9 quads and a blob of 20 added"""
    h.set_shape(GRID_TRIS, **with_attributes(blob(50, seed=4)))
    h.remove_shapes([QUAD_LEAF])
    h.add_shape(**grid(3))
    h.add_shape(**blob(20, seed=8))


def add_quads(h):
    h.add_shape(**grid(2))


def instance_the_last(h):
    h.add_instance(I.frame(2, (0.25, 0.25, 0.25), (0.25, 0.25, 0.5)), h.count("shapes") - 1, I.GREY)


def drop_the_last_shape(h):
    h.remove_shapes([h.count("shapes") - 1])


def curve_shapes(h):
    return [s for s in range(h.count("shapes")) if len(h.shape_arrays(s)["lines"]) or len(h.shape_arrays(s)["points"])]


def curves_to_triangles(h):
    for k, s in enumerate(curve_shapes(h)):
        h.set_shape(s, **blob(6 + k, seed=30 + k, scale=0.25))


def coloured_sphere(h):
    """the sphere the five media share, with vertex colours: the volumetric material's medium now varies over the surface"""
    a = h.shape_arrays(SPHERE)
    rng = np.random.default_rng(2)
    colors = np.concatenate([rng.integers(16, 65, (len(a["positions"]), 3)) / 64, np.ones((len(a["positions"]), 1))], 1).astype(F)
    kind = "triangles" if len(a["triangles"]) else "quads"
    h.set_shape(SPHERE, positions=a["positions"], normals=a["normals"], colors=colors, **{kind: a[kind]})


def plain_sphere(h):
    a = h.shape_arrays(SPHERE)
    kind = "triangles" if len(a["triangles"]) else "quads"
    h.set_shape(SPHERE, positions=a["positions"], normals=a["normals"], **{kind: a[kind][: len(a[kind]) // 2]})


def add_empty(h):
    h.add_shape(positions=np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F))


def small_lamp_mesh(n):
    def make():
        m = lamp(n)
        return dict(m, positions=(m["positions"] * F(0.5)).astype(F))
    return make


CASES = {
    "tri_leaf_5": Case(crowd(70), [set_to(TRI_LEAF, lambda: blob(5, seed=12))]),                    # the first internal node
    "blob_65_257": Case(crowd(70), [set_to(BLOB, lambda: blob(65)), set_to(BLOB, lambda: blob(257))]),   # more than a wave, than a workgroup of slots
    "grid_shrink_flip": Case(crowd(70), [set_to(GRID_QUADS, lambda: grid(6)), set_to(GRID_QUADS, lambda: with_attributes(blob(100, seed=6)))]),
    "remove_first": Case(crowd(70), [drop_instances(TRI_LEAF), shapes(lambda h: h.remove_shapes([TRI_LEAF]))]),
    "add_two": Case(crowd(70), [shapes(add_two), instances(instance_the_last_two)]),
    "all_three": Case(crowd(70), [drop_instances(QUAD_LEAF), shapes(all_three)]),
    "round_trip": Case(crowd(70), [shapes(add_two), shapes(lambda h: h.remove_shapes([7, 8]))]),
    "lamp_small_sizes": Case(crowd(70), [set_to(LAMP_SMALL, small_lamp_mesh(4)), set_to(LAMP_SMALL, small_lamp_mesh(5)), set_to(LAMP_SMALL, small_lamp_mesh(100))]),
    "lamp_large_2": Case(crowd(70), [set_to(LAMP_LARGE, lambda: lamp(2))]),
    "compact_off_on": Case(tri_scene, [shapes(add_quads), instances(instance_the_last), drop_instances(4), shapes(drop_the_last_shape)]),
    "curves_radii": Case(CURVES, [set_to(HAIR, lambda: strands(9, 4))]),
    "points_on": Case(crowd(70), [shapes(lambda h: h.add_shape(**points(40))), instances(instance_the_last)]),
    "curves_off": Case(CURVES, [shapes(curves_to_triangles)]),
    "vol_colours": Case(S03, [shapes(coloured_sphere), shapes(plain_sphere)]),
    "vol_lamp": Case(S03, [set_to(AREALIGHT1, lambda: lamp(3))]),
}
# The reference's loader refuses a shape file without elements ("empty shape"), and so does this library's, so this case cannot be
# pinned to the reference's statistics or to a fresh load: the expectation is whatever the mirror's make_bvh gives (one empty leaf),
# and on the device a fresh scene made from the mirror's descriptor.
UNPINNED = {"empty_shape": Case(crowd(70), [shapes(add_empty)])}
ALL_CASES = dict(CASES, **UNPINNED)
ROUND_TRIPS = ("round_trip", "compact_off_on")   # cases that end with the scene they began with: the original handle's tables come back


def apply(h, case, after_shapes=None, after_instances=None, names=None):
    """every step of `case` on HostScene h; after_shapes(ShapeEdit) / after_instances(InstanceEdit) see what the device is to be given.
    names: the scene file's shape entries, kept in step with the list (None for a shape the edit made) - see write_edited_scene"""
    for kind, step in case.steps:
        step(h)
        if kind == "shapes":
            edit = h.update_shapes()
            if names is not None:
                for i in edit.set:
                    names[i] = None
                for i in sorted(edit.remove, reverse=True):
                    del names[i]
                names += [None] * len(edit.add)
            if after_shapes:
                after_shapes(edit)
        else:
            edit = h.update_instances()
            if after_instances:
                after_instances(edit)


def shape_fields(h):
    """per shape: the BVH's integer fields and node count, and the primitive order"""
    _, nodes = h.bvh_nodes()
    _, prims = h.bvh_prims()
    return ([nodes[k].tobytes() for k in ("start", "num", "axis", "internal")], len(nodes), prims.tobytes())


def write_ply(path, m):
    """binary little-endian float32 PLY of a mesh dictionary (HostScene.shape_arrays); v is written flipped, as the loaders flip it back"""
    n = len(m["positions"])
    has = lambda k: m.get(k) is not None and len(m[k])
    cols, head = [np.asarray(m["positions"], F).reshape(n, 3)], ["ply", "format binary_little_endian 1.0", f"element vertex {n}", "property float x", "property float y", "property float z"]
    if has("normals"):
        cols.append(np.asarray(m["normals"], F).reshape(n, 3)), head.extend(f"property float {p}" for p in ("nx", "ny", "nz"))
    if has("texcoords"):
        uv = np.asarray(m["texcoords"], F).reshape(n, 2)
        cols.append(np.stack([uv[:, 0], F(1) - uv[:, 1]], 1)), head.extend(f"property float {p}" for p in ("u", "v"))
    if has("colors"):
        cols.append(np.asarray(m["colors"], F).reshape(n, 4)), head.extend(f"property float {p}" for p in ("red", "green", "blue", "alpha"))
    if has("radius"):
        cols.append(np.asarray(m["radius"], F).reshape(n, 1)), head.append("property float radius")
    lists = [("face", m["triangles"] if has("triangles") else m["quads"] if has("quads") else ()), ("line", m["lines"] if has("lines") else ()),
             ("point", np.asarray(m["points"]).reshape(-1, 1) if has("points") else ())]
    for name, items in lists:
        if len(items):
            head += [f"element {name} {len(items)}", "property list uchar int vertex_indices"]
    body = np.concatenate(cols, axis=1).astype("<f4").tobytes() if n else b""
    for _, items in lists:
        for it in items:
            body += struct.pack("<B", len(it)) + np.asarray(it, "<i4").tobytes()
    with open(path, "wb") as f:
        f.write(("\n".join(head + ["end_header"]) + "\n").encode() + body)


def shape_names(source):
    """the shape entries of a scene file, uris absolute: the `names` of apply()"""
    return [dict(s, uri=os.path.join(os.path.dirname(source), s["uri"])) for s in json.load(open(source))["shapes"]]


def write_edited_scene(source, edited, names, out):
    """the scene file `source` with its shape and instance arrays rewritten as the HostScene `edited` holds them, under directory `out`:
    an untouched shape keeps its file, a shape the edit made is written as binary PLY; every other item as it is, uris made relative
    to `out`.  Returns the path."""
    src_dir = os.path.dirname(source)
    d = json.load(open(source))
    os.makedirs(os.path.join(out, "shapes"), exist_ok=True)
    assert len(names) == edited.count("shapes") and not d.get("subdivs")
    d["shapes"] = []
    for j, entry in enumerate(names):
        if entry is None:
            write_ply(os.path.join(out, "shapes", f"edited_{j}.ply"), edited.shape_arrays(j))
            d["shapes"].append({"name": f"edited_{j}", "uri": f"shapes/edited_{j}.ply"})
        else:
            d["shapes"].append(dict(entry, uri=os.path.relpath(entry["uri"], out)))
    d["instances"] = [{"name": f"i{i}", "shape": int(s), "material": int(m), "frame": [float(x) for x in fr]}
                      for i, (fr, s, m) in enumerate((edited.instance_frame(i), *edited.instance_ids(i)) for i in range(edited.count("instances")))]
    for key in ("textures", "volumes"):
        for item in d.get(key, []):
            if "uri" in item:
                item["uri"] = os.path.relpath(os.path.join(src_dir, item["uri"]), out)
    path = os.path.join(out, "edited.json")
    json.dump(d, open(path, "w"))
    return path
