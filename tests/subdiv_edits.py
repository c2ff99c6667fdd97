"""What the subdiv tests share (tests/test_subdiv_plan.py, tests/test_subdiv_update_gpu.py): the scenes and their subdivs, seeded cage
moves, a numpy replay of an exported tesselation plan, copies of a scene under tmp_path whose cage files and JSON carry an edit, and
the parent's way of applying a subdiv edit to a resident scene (the host mirror's tesselate_surface, then a plain vertex edit).
Cage floats written to OBJ use 9 significant digits, which names every float32; a binary PLY takes the float32 itself."""
import json
import os

import numpy as np

from conftest import GOLDEN

F = np.float32
SCENES = os.path.join(GOLDEN, "scenes")
SYNTH = "08_subdiv_synth/subdiv_synth.json"
SURF = "01_surface_min/surface_min.json"
BOWTIE, TETRA, STRIP, BALL = range(4)   # the subdivs of SYNTH: non-manifold smooth 3 levels; closed flat 2 levels without texcoords;
#                                         smooth 2 levels with an 8-bit displacement; 0 levels, flat, float displacement on 6144 quads
CUBE = 3                                # of SURF: 4 levels, 26 / 98 / 386 / 1538 refined vertices


def path(scene_file):
    return os.path.join(SCENES, scene_file)


def moved(positions, seed, amount=0.01):
    """the cage moved by a seeded offset per coordinate, float32"""
    rng = np.random.default_rng(seed)
    return (positions + rng.uniform(-amount, amount, positions.shape).astype(F)).astype(F)


# ---- a numpy replay of a plan ----------------------------------------------------------------------------------------------------------
def replay(vpt, host, index):
    """the shape a plan makes, by the plan's own tables: the levels with the catmullclark helper (its quads must be the plan's), the
    gather through `verts`, normals and displacement with the host stage calls.  Returns the dict of HostScene.shape_arrays' float keys
    and triangles."""
    s, plan = host.subdiv(index), host.subdiv_plan(index)
    quads, pos = s["quadspos"], s["positions"]
    tquads, uv = s["quadstexcoord"], s["texcoords"]
    for level in plan.levels:
        assert len(level["valence"]) == len(pos) + len(level["edges"]) + len(level["faces"]) and np.array_equal(level["faces"], quads)
        quads, pos = vpt.catmullclark(quads, pos)
        assert np.array_equal(quads, level["new_faces"])
        if len(tquads):
            tquads, uv = vpt.catmullclark(tquads, uv, lock_boundary=True)
    assert np.array_equal(quads, plan.quads)
    normals = plan.cage_normals
    if plan.subdivisions > 0:
        normals = vpt.vertex_normals(pos, quads) if plan.smooth else np.zeros((0, 3), F)
    v = plan.verts
    out = {"positions": pos[v[:, 0]], "normals": normals[v[:, 1]] if len(normals) else np.zeros((0, 3), F),
           "texcoords": uv[v[:, 2]] if len(tquads) else np.zeros((0, 2), F)}
    # quads_to_triangles over the split quads: vertex ids by first appearance of their index triple, which is the order of `verts`
    triple = {tuple(t): i for i, t in enumerate(v.tolist())}
    nq, tq = (s["quadsnorm"] if plan.subdivisions == 0 else quads if plan.smooth else []), tquads
    tris = []
    for f in range(len(quads)):
        c = [triple[(int(quads[f][k]), int(nq[f][k]) if len(nq) else -1, int(tq[f][k]) if len(tq) else -1)] for k in range(4)]
        tris.append([c[0], c[1], c[3]])
        if c[2] != c[3]:
            tris.append([c[2], c[3], c[1]])
    out["triangles"] = np.array(tris, np.int32)
    if plan.displacement != 0 and plan.displacement_tex >= 0:
        texels, linear = host.texture(plan.displacement_tex)
        if not len(out["normals"]):
            out["normals"] = vpt.vertex_normals(out["positions"], out["triangles"])
        out["positions"] = vpt.displace_vertices(texels, linear, plan.displacement, out["positions"], out["normals"], out["texcoords"])
        out["normals"] = vpt.vertex_normals(out["positions"], out["triangles"]) if plan.smooth else np.zeros((0, 3), F)
    return out


# ---- a scene whose files carry an edit ---------------------------------------------------------------------------------------------------
def _patch_obj(src, dst, positions):
    k, lines = 0, []
    for line in open(src).read().splitlines():
        if line.startswith("v "):
            line = "v " + " ".join(f"{float(c):.9g}" for c in positions[k])
            k += 1
        lines.append(line)
    assert k == len(positions), (src, k, len(positions))
    open(dst, "w").write("\n".join(lines) + "\n")


def _patch_ply(src, dst, positions):
    """a binary little-endian PLY whose vertex properties are all floats, x / y / z replaced"""
    raw = open(src, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode().splitlines()
    assert lines[1] == "format binary_little_endian 1.0", src
    at = next(i for i, l in enumerate(lines) if l.startswith("element vertex"))
    count, props = int(lines[at].split()[2]), []
    for l in lines[at + 1:]:
        if not l.startswith("property"):
            break
        assert l.split()[1] == "float", (src, l)
        props.append(l.split()[2])
    assert props[:3] == ["x", "y", "z"] and count == len(positions), src
    verts = np.frombuffer(raw, "<f4", count * len(props), end).reshape(count, len(props)).copy()
    verts[:, :3] = positions
    open(dst, "wb").write(raw[:end] + verts.astype("<f4").tobytes() + raw[end + verts.nbytes:])


def write_scene(scene_file, out, cages=None, settings=None, change=None):
    """a copy of the scene under directory `out` (a pathlib.Path): the cage files of `cages` (subdiv id -> positions) rewritten, the
    subdiv entries of the JSON updated from `settings` (subdiv id -> dict), change(json dict) applied last; everything else is linked
    to where it is.  Returns the scene file's path."""
    src = os.path.dirname(path(scene_file))
    here = out / "scene"
    os.makedirs(here / "edited", exist_ok=True)
    for name in os.listdir(SCENES):   # "../03_volume/..." and "../shared_textures/..." resolve as they do in the golden tree
        if os.path.isdir(os.path.join(SCENES, name)) and not os.path.lexists(out / name):
            os.symlink(os.path.join(SCENES, name), out / name)
    for name in os.listdir(src):
        if os.path.isdir(os.path.join(src, name)) and not os.path.lexists(here / name):
            os.symlink(os.path.join(src, name), here / name)
    d = json.load(open(path(scene_file)))
    for index, positions in (cages or {}).items():
        uri = d["subdivs"][index]["uri"]
        name = f"edited/cage{index}" + os.path.splitext(uri)[1]
        (_patch_ply if uri.endswith(".ply") else _patch_obj)(os.path.join(src, uri), here / name, np.asarray(positions, F))
        d["subdivs"][index]["uri"] = name
    for index, values in (settings or {}).items():
        d["subdivs"][index].update(values)
    if change:
        change(d)
    file = here / os.path.basename(scene_file)
    file.write_text(json.dumps(d))
    return str(file)


# ---- the parent's way of a subdiv edit on a resident scene --------------------------------------------------------------------------------
def lit_shapes(host):
    """shapes that an instance with an emissive material uses"""
    out = set()
    for i in range(host.count("instances")):
        shape, material = host.instance_ids(i)
        if any(c != 0 for c in host.material(material).emission):
            out.add(shape)
    return out


def parents_way(vpt, dev, host, shapes):
    """`host` has re-tesselated `shapes` (set_subdiv): the tesselated vertices uploaded through vpt_scene_update - through
    vpt_scene_update_lights when a light's instance uses one of them"""
    edit = vpt.SceneEdit(shapes={s: (host.shape_positions(s), host.shape_normals(s) if len(host.shape_normals(s)) else None) for s in shapes})
    (dev.update_lights if lit_shapes(host) & set(shapes) else dev.update)(edit)
