#!/usr/bin/env python3
"""Builds the scenes of points and lines (hair, particles) and their reference renders.  Run from anywhere:

  python tests/golden/make_curves_scene.py           scenes/09_curves_synth/ (curves.json, dense.json, binary-LE PLYs)
  python tests/golden/make_curves_scene.py --render  + curves_states.npz, curves_stats.json, curves_volpath.jpg, rendered by the
                                                     reference itself (oracle/_ref/ref_driver through tests/oracle_lib.reference_render)

curves.json: polylines of several segments (hair strands) with per-vertex radius, normals, texcoords and colours under glossy,
matte and volumetric materials; a point cloud with varying radius and colours, once matte and once refractive under a scaled
(non-rigid) frame; a points shape without radius (the loader's 0.001 default); an emissive polyline; a triangle mesh; the floor
and area light of 03_volume (its PLYs, copied as data).  dense.json: about 20k segments of strands over the floor, for traversal.
Everything is generated from fixed formulas (no RNG state beyond a seeded numpy generator)."""
import json
import os
import shutil
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "scenes", "09_curves_synth")
SRC03 = os.path.join(HERE, "scenes", "03_volume", "shapes")

# every case of the parity tests: (shader, samples); 96 pixels wide at the camera's aspect 2.4
RESOLUTION, BOUNCES = 96, 8
CASES = (("volpathtrace", 4), ("pathtrace", 4), ("naive", 4), ("eyelight", 4), ("normal", 2), ("texcoord", 2), ("color", 2))
DENSE_CASE = ("volpathtrace", 64, 2)   # shader, resolution, samples


def write_ply(path, positions, normals=None, texcoords=None, colors=None, radius=None, lines=(), points=(), faces=()):
    """binary little-endian PLY with the vertex properties given and `line` / `point` / `face` elements of int lists"""
    n = len(positions)
    props = [("x", "y", "z")] + ([("nx", "ny", "nz")] if normals is not None else []) + \
            ([("u", "v")] if texcoords is not None else []) + \
            ([("red", "green", "blue", "alpha")] if colors is not None else []) + ([("radius",)] if radius is not None else [])
    cols = [np.asarray(positions, np.float32)] + [np.asarray(a, np.float32).reshape(n, -1)
                                                  for a in (normals, texcoords, colors, radius) if a is not None]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    head += [f"property float {p}" for group in props for p in group]
    for name, items in (("face", faces), ("line", lines), ("point", points)):
        if len(items):
            head += [f"element {name} {len(items)}", "property list uchar int vertex_indices"]
    head.append("end_header")
    body = np.concatenate(cols, axis=1).astype("<f4").tobytes()
    for items in (faces, lines, points):
        for it in items:
            body += struct.pack("<B", len(it)) + np.asarray(it, "<i4").tobytes()
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode() + body)


def strands(count, verts, spread, height, seed, base=(0.0, 0.0)):
    """`count` polylines of `verts` vertices growing up from a disc, bending with height"""
    g = np.random.default_rng(seed)
    roots = g.uniform(-spread, spread, (count, 2)) + np.asarray(base)
    bend = g.uniform(-0.6, 0.6, (count, 2))
    s = np.linspace(0, 1, verts)
    pos = np.zeros((count, verts, 3), np.float32)
    pos[:, :, 0] = roots[:, None, 0] + bend[:, None, 0] * height * s ** 2
    pos[:, :, 1] = height * s[None, :] * g.uniform(0.7, 1.0, (count, 1))
    pos[:, :, 2] = roots[:, None, 1] + bend[:, None, 1] * height * s ** 2
    return pos.reshape(-1, 3)


def frame(scale=(1, 1, 1), o=(0, 0, 0)):
    return [scale[0], 0, 0, 0, scale[1], 0, 0, 0, scale[2], o[0], o[1], o[2]]


def build():
    os.makedirs(os.path.join(OUT, "shapes"), exist_ok=True)
    for name in ("floor.ply", "arealight1.ply"):
        shutil.copy(os.path.join(SRC03, name), os.path.join(OUT, "shapes", name))
    # hair: 16 strands of 6 vertices (5 segments each), radius thinning to the tip
    nst, nv = 16, 6
    pos = strands(nst, nv, 0.06, 0.25, 1)
    s = np.tile(np.linspace(0, 1, nv), nst)
    rad = (0.008 - 0.005 * s).astype(np.float32)
    nrm = np.stack([np.cos(7 * s), np.full_like(s, 0.3), np.sin(7 * s)], 1)
    uv = np.stack([s, np.repeat(np.arange(nst) / nst, nv)], 1)
    col = np.stack([0.3 + 0.6 * s, 0.2 + 0.3 * (1 - s), np.full_like(s, 0.15), np.ones_like(s)], 1)
    write_ply(os.path.join(OUT, "shapes", "hair.ply"), pos, nrm, uv, col, rad,
              lines=[list(range(k * nv, (k + 1) * nv)) for k in range(nst)])
    # particle cloud: 48 points, radius 0.01 .. 0.03, colours and texcoords
    g = np.random.default_rng(2)
    cp = g.uniform([-0.12, 0.03, -0.08], [0.12, 0.2, 0.08], (48, 3))
    write_ply(os.path.join(OUT, "shapes", "cloud.ply"), cp, None, g.uniform(0, 1, (48, 2)),
              np.concatenate([g.uniform(0.2, 0.9, (48, 3)), np.ones((48, 1))], 1), g.uniform(0.01, 0.03, 48),
              points=[[k] for k in range(48)])
    # dust: points without radius (the loader gives every vertex 0.001)
    dp = g.uniform([-0.5, 0.02, -0.3], [0.5, 0.3, 0.3], (24, 3))
    write_ply(os.path.join(OUT, "shapes", "dust.ply"), dp, points=[[k] for k in range(24)])
    # an emissive polyline of 8 vertices, no normals (the element normal is the line tangent)
    t = np.linspace(0, 1, 8)
    ep = np.stack([-0.45 + 0.9 * t, 0.05 + 0.1 * np.sin(5 * t), 0.15 + 0.02 * t], 1)
    write_ply(os.path.join(OUT, "shapes", "glow.ply"), ep, radius=np.full(8, 0.01), lines=[list(range(8))])
    # a small triangle mesh: a pyramid
    pp = [[-0.06, 0, -0.06], [0.06, 0, -0.06], [0.06, 0, 0.06], [-0.06, 0, 0.06], [0, 0.12, 0]]
    write_ply(os.path.join(OUT, "shapes", "pyramid.ply"), pp, faces=[[0, 4, 1], [1, 4, 2], [2, 4, 3], [3, 4, 0]])

    base = json.load(open(os.path.join(HERE, "scenes", "03_volume", "volume.json")))
    light = [i for i in base["instances"] if i["name"] == "arealight1"][0]
    materials = [
        {"name": "floor", "color": [0.7, 0.7, 0.7], "type": "matte"},
        {"name": "arealight1", "emission": [20, 20, 20], "type": "matte"},
        {"name": "hair_glossy", "color": [0.6, 0.4, 0.2], "roughness": 0.3, "type": "glossy"},
        {"name": "hair_matte", "color": [0.8, 0.8, 0.8], "type": "matte"},
        {"name": "hair_smoke", "color": [0.5, 0.5, 0.5], "scattering": [0.6, 0.6, 0.6], "type": "volumetric"},
        {"name": "glass", "roughness": 0, "color": [1, 0.6, 0.6], "trdepth": 0.02, "type": "refractive"},
        {"name": "glow", "emission": [4, 2, 1], "color": [0.2, 0.2, 0.2], "type": "matte"},
        {"name": "pyramid", "color": [0.3, 0.5, 0.8], "type": "matte"},
    ]
    shapes = [{"name": n, "uri": f"shapes/{n}.ply"} for n in ("floor", "arealight1", "hair", "cloud", "dust", "glow", "pyramid")]
    instances = [
        {"name": "floor", "shape": 0, "material": 0},
        {"name": "arealight1", "frame": light["frame"], "shape": 1, "material": 1},
        {"name": "hair_glossy", "frame": frame(o=(-0.3, 0, 0)), "shape": 2, "material": 2},
        {"name": "hair_matte", "frame": frame(o=(0.05, 0, 0.05)), "shape": 2, "material": 3},
        {"name": "hair_smoke", "frame": frame(o=(0.32, 0, 0)), "shape": 2, "material": 4},
        {"name": "cloud_matte", "frame": frame(o=(-0.12, 0.02, -0.15)), "shape": 3, "material": 3},
        {"name": "cloud_glass", "frame": frame((1.5, 0.7, 1.0), (0.18, 0.03, -0.12)), "shape": 3, "material": 5},
        {"name": "dust", "shape": 4, "material": 5},
        {"name": "glow", "shape": 5, "material": 6},
        {"name": "pyramid", "frame": frame(o=(0.15, 0, 0.15)), "shape": 6, "material": 7},
    ]
    scene = {"asset": {"version": "4.2"}, "cameras": base["cameras"],
             "environments": [{"name": "sky", "emission": [0.2, 0.2, 0.25]}],
             "materials": materials, "shapes": shapes, "instances": instances}
    with open(os.path.join(OUT, "curves.json"), "w") as f:
        json.dump(scene, f, indent=1)

    # dense: 800 strands of 26 vertices = 20 000 segments over the floor
    dn, dv = 800, 26
    dpos = strands(dn, dv, 0.45, 0.2, 3)
    ds = np.tile(np.linspace(0, 1, dv), dn)
    write_ply(os.path.join(OUT, "shapes", "dense.ply"), dpos, radius=(0.003 - 0.002 * ds),
              lines=[list(range(k * dv, (k + 1) * dv)) for k in range(dn)])
    dense = dict(scene, shapes=[shapes[0], shapes[1], {"name": "dense", "uri": "shapes/dense.ply"}],
                 materials=materials[:3], instances=instances[:2] + [{"name": "dense", "shape": 2, "material": 2}])
    with open(os.path.join(OUT, "dense.json"), "w") as f:
        json.dump(dense, f, indent=1)


def render():
    sys.path.insert(0, os.path.dirname(HERE))
    import oracle_lib
    arrays, stats = {}, {}
    scene = os.path.join(OUT, "curves.json")
    for shader, spp in CASES:
        w, h, image, hits, rngs, info, st = oracle_lib.reference_render(scene, shader, RESOLUTION, spp, bounces=BOUNCES, stats=True)
        arrays[f"{shader}_image"], arrays[f"{shader}_hits"], arrays[f"{shader}_rngs"] = image, hits, rngs
        stats["curves"] = {k: st[k] for k in ("scene_bvh", "shapes", "lights")}
    shader, res, spp = DENSE_CASE
    w, h, image, hits, rngs, info, st = oracle_lib.reference_render(os.path.join(OUT, "dense.json"), shader, res, spp,
                                                                    bounces=BOUNCES, stats=True)
    arrays["dense_image"], arrays["dense_hits"], arrays["dense_rngs"] = image, hits, rngs
    stats["dense"] = {k: st[k] for k in ("scene_bvh", "shapes", "lights")}
    np.savez_compressed(os.path.join(HERE, "curves_states.npz"), **arrays)
    with open(os.path.join(HERE, "curves_stats.json"), "w") as f:
        json.dump(stats, f, indent=1)
    # the JPEG of the reference's own output stage for the ypathtrace test (volpathtrace, 48 pixels, 2 spp)
    oracle_lib.reference_render(scene, "volpathtrace", 48, 2, bounces=BOUNCES, output=os.path.join(HERE, "curves_volpath.jpg"))


if __name__ == "__main__":
    build()
    if "--render" in sys.argv:
        render()
