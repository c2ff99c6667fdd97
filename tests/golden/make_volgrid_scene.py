#!/usr/bin/env python3
"""Builds the scenes of the volgrid shader's tests (voxel grids as heterogeneous media).  Run from anywhere:

  python tests/golden/make_volgrid_scene.py      scenes/10_volgrid_synth/: volgrid.json and its siblings, sdfs/*.sdf (binary)

Every scene: an orthographic camera looking down -z at an axis-aligned grid box [0, 1]^3 (camera 0: the box with a margin; camera 1:
zoomed on the box's centre, for the sparse grid's block), an untextured environment of emission (0.5, 0.5, 0.5), one material
("medium": scattering 0.8, scanisotropy 0.6, trdepth 1).  The siblings differ in their volumes and grid instances:

  volgrid.json      the sparse grid: 32^3 nodes, the central 8-node block (nodes 12 .. 19 per axis) 1, everything else 0 - the
                    trilerp gives it a one-cell linear skirt; most bricks are empty
  constant.json     9^3 nodes, all 1
  ramp.json         17^3 nodes, 2 k / 16 along z: 0 .. 2, mean 1
  overlap.json      two instances of the constant grid with materials of different trdepth, the second moved by (0.25, 0.25, 0)
  messy.json        9 x 17 x 30 nodes of a seeded pattern with NaN, +-Inf, negative values and zeros (tables and lookups, not renders)
  furnace_tex.json  the sparse grid and a texture for the environment (the tests replace its texels by one colour: a CDF light)
  two_env.json      the sparse grid under two untextured environments of emission (0.25, 0.25, 0.25) each: two entries of the light list

Grids are written from fixed formulas and a seeded numpy generator; numpy only."""
import json
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "scenes", "10_volgrid_synth")
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def write_sdf(path, voxels, res):
    """the binary .sdf of the scene loader: int32 w h d, float res, 16 floats (ignored), the voxels x fastest; voxels of shape (d, h, w)"""
    voxels = np.ascontiguousarray(voxels, "<f4")
    d, h, w = voxels.shape
    with open(path, "wb") as f:
        f.write(struct.pack("<iiif", w, h, d, res) + bytes(64) + voxels.tobytes())


def sparse_grid():
    v = np.zeros((32, 32, 32), np.float32)
    v[12:20, 12:20, 12:20] = 1.0
    return v


def ramp_grid():
    v = np.zeros((17, 17, 17), np.float32)
    v[:] = (np.float32(2.0) * np.arange(17, dtype=np.float32) / np.float32(16.0))[:, None, None]
    return v


def messy_grid():
    g = np.random.default_rng(20241)
    v = g.uniform(-1.0, 3.0, (30, 17, 9)).astype(np.float32)
    flat = v.reshape(-1)
    pick = g.permutation(flat.size)
    flat[pick[0:40]] = np.nan
    flat[pick[40:80]] = np.inf
    flat[pick[80:120]] = -np.inf
    flat[pick[120:400]] = 0.0
    v[0:9, 0:9, :] = -0.5   # a whole brick without a positive node: majorant 0
    return v


def camera(name, extent):
    # orthographic: the film spans film / lens world units (eval_camera, yocto_scene.cpp:67-102); aspect 1
    return {"name": name, "frame": IDENTITY + [0.5, 0.5, 3.0], "orthographic": True, "lens": 0.036 / extent, "film": 0.036, "aspect": 1.0,
            "focus": 3.0, "aperture": 0.0}


def scene(volumes, instances, materials=None, textures=None, environments=None):
    out = {"asset": {"generator": "tests/golden/make_volgrid_scene.py", "version": "4.2"},
           "cameras": [camera("box", 1.25), camera("centre", 0.25)],
           "environments": environments or [{"name": "grey", "emission": [0.5, 0.5, 0.5]}],
           "materials": materials or [{"name": "medium", "type": "volumetric", "scattering": [0.8, 0.8, 0.8], "scanisotropy": 0.6, "trdepth": 1.0}],
           "volumes": [{"name": n, "uri": f"sdfs/{n}.sdf", "binary": True} for n in volumes],
           "vol_instances": instances}
    if textures:
        out["textures"] = textures
    return out


def instance(name, volume, material=0, origin=(0.0, 0.0, 0.0)):
    return {"name": name, "volume": volume, "material": material, "scale": 1, "frame": IDENTITY + [-float(o) for o in origin]}


def main():
    os.makedirs(os.path.join(OUT, "sdfs"), exist_ok=True)
    # res * W = 1 on every axis of the cubic grids: the box is [0, 1]^3; the messy grid's box is 9 x 17 x 30 times 1 / 30
    write_sdf(os.path.join(OUT, "sdfs", "sparse.sdf"), sparse_grid(), 1.0 / 32)
    write_sdf(os.path.join(OUT, "sdfs", "constant.sdf"), np.ones((9, 9, 9), np.float32), 1.0 / 9)
    write_sdf(os.path.join(OUT, "sdfs", "ramp.sdf"), ramp_grid(), 1.0 / 17)
    write_sdf(os.path.join(OUT, "sdfs", "messy.sdf"), messy_grid(), 1.0 / 30)
    two = [{"name": "thin", "type": "volumetric", "scattering": [0.8, 0.8, 0.8], "scanisotropy": 0.6, "trdepth": 2.0},
           {"name": "thick", "type": "volumetric", "scattering": [0.8, 0.8, 0.8], "scanisotropy": 0.6, "trdepth": 0.75}]
    scenes = {
        "volgrid.json": scene(["sparse"], [instance("cloud", 0)]),
        "constant.json": scene(["constant"], [instance("slab", 0)]),
        "ramp.json": scene(["ramp"], [instance("ramp", 0)]),
        "overlap.json": scene(["constant"], [instance("thin", 0, 0), instance("thick", 0, 1, (0.25, 0.25, 0.0))], materials=two),
        "messy.json": scene(["messy", "sparse"], [instance("messy", 0), instance("cloud", 1)]),
        "furnace_tex.json": scene(["sparse"], [instance("cloud", 0)], textures=[{"name": "sky", "uri": "../shared_textures/texture2.hdr"}]),
        "two_env.json": scene(["sparse"], [instance("cloud", 0)], environments=[{"name": n, "emission": [0.25, 0.25, 0.25]} for n in ("grey_a", "grey_b")]),
    }
    for name, content in scenes.items():
        with open(os.path.join(OUT, name), "w") as f:
            json.dump(content, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
