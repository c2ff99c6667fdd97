"""Shapes of points and lines (hair, particles) on the host side, without a GPU: the loader (PLY `line` / `point` / `radius`,
OBJ `l` / `p`, the 0.001 default radius), the shape BVHs over point_bounds / line_bounds and the lights against the reference's
own figures (tests/golden/curves_stats.json, written by ref_driver: tests/golden/make_curves_scene.py), and the refusals of
shapes that mix points, lines and faces - by the loader, by the flattening and by vpt_scene_create."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

from conftest import GOLDEN

SCENES = os.path.join(GOLDEN, "scenes", "09_curves_synth")
CURVES, DENSE = os.path.join(SCENES, "curves.json"), os.path.join(SCENES, "dense.json")
VPT_ERR_INVALID_ARG, VPT_ERR_NO_DEVICE, VPT_ERR_UNSUPPORTED = -1, -2, -5


def _stats(vpt, path):
    return json.loads(vpt.HostScene(path).stats())


def test_loader_counts_polylines_and_default_radius(vpt):
    shapes = _stats(vpt, CURVES)["shapes"]
    hair, cloud, dust, glow = shapes[2], shapes[3], shapes[4], shapes[5]
    # 16 strands of 6 vertices: every polyline of n vertices is n - 1 segments (get_lines, yocto_modelio.cpp:1212-1227)
    assert (hair["positions"], hair["lines"], hair["points"], hair["radius"], hair["normals"], hair["texcoords"], hair["colors"]) == \
        (96, 80, 0, 96, 96, 96, 96)
    assert (cloud["points"], cloud["lines"], cloud["radius"]) == (48, 0, 48)
    assert (glow["lines"], glow["radius"]) == (7, 8)
    # no radius in the file: add_missing_radius gives every vertex 0.001 (yocto_sceneio.cpp:2071-2076)
    assert (dust["points"], dust["radius"]) == (24, 24)
    assert dust["radius_fnv"] == "%016x" % _fnv1a(np.full(24, 0.001, np.float32).tobytes())
    # shapes of faces report what they always did (the lines oracle/ref_driver.cpp --stats writes)
    assert "points" not in shapes[0] and "lines" not in shapes[6]
    assert _stats(vpt, DENSE)["shapes"][2]["lines"] == 800 * 25


def _fnv1a(b):
    h = 0xcbf29ce484222325
    for x in b:
        h = ((h ^ x) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


REF_KEYS = ("positions", "normals", "texcoords", "colors", "triangles", "quads", "pos_fnv", "nrm_fnv", "uv_fnv", "tri_fnv", "quad_fnv",
            "bvh_nodes", "bvh_nodes_fnv", "bvh_prims_fnv")


@pytest.mark.parametrize("name,path", [("curves", CURVES), ("dense", DENSE)])
def test_bvh_and_lights_equal_the_references(vpt, name, path):
    ref = json.load(open(os.path.join(GOLDEN, "curves_stats.json")))[name]
    mine = _stats(vpt, path)
    assert mine["scene_bvh"] == ref["scene_bvh"]
    assert [{k: s[k] for k in REF_KEYS} for s in mine["shapes"]] == ref["shapes"]
    # make_lights skips shapes without faces (yocto_pathtrace.cpp:992): the emissive polyline is no light
    assert mine["lights"] == ref["lights"] and [l["instance"] for l in mine["lights"]] == [1, -1]


def _scene_with_shape(tmp_path, name, data):
    (tmp_path / name).write_bytes(data) if isinstance(data, bytes) else (tmp_path / name).write_text(data)
    cam = {"frame": [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 3], "lens": 0.05, "aspect": 1}
    scene = {"asset": {"version": "4.2"}, "cameras": [cam], "materials": [{"type": "matte", "color": [0.5, 0.5, 0.5]}],
             "shapes": [{"uri": name}], "instances": [{"shape": 0, "material": 0}]}
    path = tmp_path / "scene.json"
    path.write_text(json.dumps(scene))
    return str(path)


def test_obj_lines_and_points(vpt, tmp_path):
    st = _stats(vpt, _scene_with_shape(tmp_path, "a.obj", "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nl 1 2 3 4\nl 4 1\n"))["shapes"][0]
    assert (st["lines"], st["points"], st["radius"], st["triangles"]) == (4, 0, 4, 0)
    st = _stats(vpt, _scene_with_shape(tmp_path, "b.obj", "usemtl x\nv 0 0 0\nv 1 0 0\nv 1 1 0\np 1 2\np 3\n"))["shapes"][0]
    # every corner of a `p` element reads the element's first vertex (get_points, yocto_modelio.cpp:2419-2434)
    assert (st["points"], st["lines"], st["radius"]) == (3, 0, 3)
    assert st["points_fnv"] == "%016x" % _fnv1a(np.int32([0, 0, 2]).tobytes())
    # one element kind under at most one material, else refused at load (the reference's cursors skip without advancing)
    for bad in ("v 0 0 0\nv 1 0 0\nl 1 2\np 1\n", "v 0 0 0\nv 1 0 0\nusemtl a\nl 1 2\nusemtl b\nl 2 1\n"):
        with pytest.raises(vpt.VptError, match="one element kind"):
            _stats(vpt, _scene_with_shape(tmp_path, "c.obj", bad))


def _ply(vertices, radius=None, lines=(), points=(), faces=()):
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(vertices)}", "property float x", "property float y",
            "property float z"] + (["property float radius"] if radius is not None else [])
    body = b""
    for i, v in enumerate(vertices):
        body += struct.pack("<3f", *v) + (struct.pack("<f", radius[i]) if radius is not None else b"")
    for name, items in (("face", faces), ("line", lines), ("point", points)):
        if items:
            head += [f"element {name} {len(items)}", "property list uchar int vertex_indices"]
    for items in (faces, lines, points):
        for it in items:
            body += struct.pack("<B", len(it)) + struct.pack(f"<{len(it)}i", *it)
    return ("\n".join(head + ["end_header"]) + "\n").encode() + body


def test_mixed_shapes_and_bad_indices_are_refused(vpt, tmp_path):
    quad = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)]
    for data, why in ((_ply(quad, lines=[[0, 1, 2]], faces=[[0, 1, 2]]), "mixes points, lines and faces"),
                      (_ply(quad, lines=[[0, 1]], points=[[2]]), "mixes points, lines and faces")):
        with pytest.raises(vpt.VptError, match=why):
            vpt.HostScene(_scene_with_shape(tmp_path, "m.ply", data))
    with pytest.raises(vpt.VptError, match="parse error|read error|error"):
        vpt.HostScene(_scene_with_shape(tmp_path, "i.ply", _ply(quad, lines=[[0, 7]])))
    # a faces OBJ with `l` elements keeps them and is refused when flattened (tests/test_tesselate.py pins the same)
    with pytest.raises(vpt.VptError, match="mixes points, lines and faces"):
        vpt.HostScene(_scene_with_shape(tmp_path, "f.obj", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\nl 1 2\n"))


def _create(vpt, scene, curves=True):
    """vpt_scene_create_curves on device -1, which no machine has: the scene is prepared (and refused if it must be) before the
    call looks for a device"""
    out = C.c_void_p()
    rc = vpt.hip.vpt_scene_create_curves(C.c_void_p(scene.desc), C.c_void_p(scene.curves if curves else None), -1, C.byref(out))
    return rc, vpt.hip.vpt_last_error().decode()


class ShapeCurves(C.Structure):
    _fields_ = [("num_points", C.c_int32), ("point_offset", C.c_int32), ("num_lines", C.c_int32), ("line_offset", C.c_int32),
                ("radius_offset", C.c_int32)]


def test_scene_create_accepts_curves_and_refuses_mixed_descriptors(vpt):
    for path in (CURVES, DENSE):
        scene = vpt.HostScene(path)
        rc, msg = _create(vpt, scene)
        assert rc == VPT_ERR_NO_DEVICE, msg   # prepared in full, refused only for want of a device
    scene = vpt.HostScene(CURVES)
    # vpt_scene_curves (include/vpt.h): shape_curves, {num_points, points}, {num_lines, lines}, {num_radius, radius}
    words = (C.c_uint64 * 7).from_address(scene.curves)
    curves = (ShapeCurves * 7).from_address(words[0])
    assert words[1] == 48 + 24 and words[3] == 80 + 7 and words[5] == 96 + 48 + 24 + 8
    hair, floor = curves[2], curves[0]
    assert (hair.num_lines, hair.num_points, curves[3].num_points, floor.num_lines, floor.radius_offset) == (80, 0, 48, 0, -1)
    line_offset = hair.line_offset
    try:
        hair.num_points = 1   # the hair shape holds points and lines
        rc, msg = _create(vpt, scene)
        assert rc == VPT_ERR_UNSUPPORTED and "mixes points, lines and faces" in msg
        hair.num_points, floor.num_lines = 0, 1   # the floor (faces) with a line
        rc, msg = _create(vpt, scene)
        assert rc == VPT_ERR_UNSUPPORTED and "shape 0 mixes" in msg
        floor.num_lines, hair.line_offset = 0, 10 ** 6
        rc, msg = _create(vpt, scene)
        assert rc == VPT_ERR_INVALID_ARG and "lines out of range" in msg
        hair.line_offset, hair.radius_offset = line_offset, -1   # lines need a radius
        rc, msg = _create(vpt, scene)
        assert rc == VPT_ERR_INVALID_ARG and "radius out of range" in msg
    finally:
        hair.num_points, floor.num_lines, hair.line_offset = 0, 0, line_offset


def test_descriptor_alone_keeps_its_meaning(vpt):
    """vpt_scene_desc has the layout binaries built against earlier headers fill in: points and lines travel beside it.  A scene of
    faces has no side struct; the descriptor of a curves scene without it describes shapes with no elements, which is refused"""
    faces = vpt.HostScene(os.path.join(GOLDEN, "scenes", "03_volume", "volume.json"))
    assert faces.curves is None
    out = C.c_void_p()
    assert vpt.hip.vpt_scene_create(C.c_void_p(faces.desc), -1, C.byref(out)) == VPT_ERR_NO_DEVICE
    scene = vpt.HostScene(CURVES)
    assert vpt.hip.vpt_scene_create(C.c_void_p(scene.desc), -1, C.byref(out)) == VPT_ERR_INVALID_ARG
    rc, msg = _create(vpt, scene, curves=False)
    assert rc == VPT_ERR_INVALID_ARG and "bad leaf range" in msg
