"""Sculpt edits shared by tests/test_sculpt_host.py and tests/test_sculpt_gpu.py: brushes, strokes, regions, and a numpy replay of the
rule of vpt_scene_sculpt_volumes (include/vpt.h), float32 operation by operation.  A case is (volume, [Stamp, ...], region or None,
origin or None, step or None): what HostScene.sculpt_volume takes.

All cases run on 06_gridsdf_synth's bunny (volume 1: 40^3, res 0.0036; instances 2 and 3).  Its voxel space - origin 0, step
res * 40 / 39 - spans 0 .. 0.144 per axis and its values are distances in that space; the bunny lies low in its grid (voxels 3 .. 13 of y), so
a brush of a few hundredths around CENTRE straddles its surface: a union adds negative voxels outside the bunny, a subtraction and an
intersection turn negative voxels inside it positive.  test_sculpt_host.py checks that for every case (at least 1 % of the region's
voxels change, at least one changes sign), so that the GPU tests cannot pass on an edit that does nothing."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GRID = os.path.join(HERE, "golden", "scenes", "06_gridsdf_synth", "gridsdf_synth.json")
SDFS = os.path.join(HERE, "golden", "scenes", "07_sdfunction_synth", "sdfunction_synth.json")
F = np.float32
SACKBOY, BUNNY = 0, 1
BUNNY_INSTANCES = (2, 3)
REPLACE, UNION, SUBTRACT, INTERSECT = range(4)
OPS = {"replace": REPLACE, "union": UNION, "subtract": SUBTRACT, "intersect": INTERSECT}
TYPES = ["bbox", "box", "capped_cone", "plane", "sphere", "torus"]   # vpt.SDF_TYPES
BLENDS = (0.0, 0.01)
CENTRE = (0.072, 0.03, 0.072)
IDENTITY = np.eye(3, dtype=F)
REGION = ((1, 2, 3), (5, 3, 2))          # the region of tests/volume_edits.py
ROWS = ((3, 2, 1), (37, 5, 3))           # rows that are no multiple of a wave, a last block that is partial
ONE = ((39, 0, 17), (1, 1, 1))
WHOLE = ((0, 0, 0), (40, 40, 40))
BOX = ((4, 5, 6), (30, 28, 26))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def rotation(angle=0.6, tilt=0.35):
    """a rotation about y by `angle`, then about x by `tilt`: the rows are the brush's local axes in voxel space"""
    c, s, ct, st = np.cos(angle), np.sin(angle), np.cos(tilt), np.sin(tilt)
    ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    rx = np.array([[1, 0, 0], [0, ct, -st], [0, st, ct]])
    return (rx @ ry).astype(F)


def brush(vpt, kind, centre=CENTRE, axes=None, scale=1.0):
    """a VptSdf of type `kind` whose local origin lies at `centre` of the voxel space: local = axes @ (p - centre).  frame.x / y / z are
    the columns transform_point multiplies p.x / p.y / p.z by, frame.o = -(axes @ centre)."""
    axes = IDENTITY if axes is None else np.asarray(axes, F)
    f = vpt.VptSdf(type=TYPES.index(kind), material=0)
    f.frame.x[:], f.frame.y[:], f.frame.z[:] = [float(v) for v in axes[:, 0]], [float(v) for v in axes[:, 1]], [float(v) for v in axes[:, 2]]
    f.frame.o[:] = [float(v) for v in -(axes.astype(np.float64) @ np.asarray(centre, np.float64)).astype(F)]
    k = float(scale)
    if kind == "bbox":
        f.p[:] = (0.006 * k, 0.034 * k, 0.03 * k, 0.026 * k)
    elif kind == "box":
        f.whd[:] = (0.05 * k, 0.04 * k, 0.045 * k)
    elif kind == "capped_cone":
        f.p[:] = (0.03 * k, 0.034 * k, 0.014 * k, 0.0)
    elif kind == "sphere":
        f.p[:] = (0.03 * k, 0.0, 0.0, 0.0)
    elif kind == "torus":
        f.p[:] = (0.036 * k, 0.014 * k, 0.0, 0.0)
    return f


def voxel_centre(region, step=None):
    """the voxel-space point of the voxel in the middle of a region of the bunny's default grid"""
    lo, size = region
    step = F(0.0036) * F(40) / F(39) if step is None else step
    return tuple(float(F(lo[k] + size[k] // 2) * step) for k in range(3))


def shape_stamps(vpt, region):
    """a stroke that changes every region it is given: a subtraction of a large sphere (every voxel inside it becomes positive), then a
    union with a small one around the region's middle voxel (which becomes negative)"""
    c = voxel_centre(region)
    return [vpt.Stamp(brush(vpt, "sphere", c, scale=4.0), SUBTRACT), vpt.Stamp(brush(vpt, "sphere", c, rotation(), scale=0.25), UNION, 0.002)]


def stroke(vpt, n):
    """n spheres along a slanted line through the bunny, subtracting and uniting in turn, every third one blended"""
    out = []
    for s in range(n):
        t = (s + 0.5) / n
        c = (0.03 + 0.085 * t, 0.02 + 0.025 * t, 0.11 - 0.075 * t)
        out.append(vpt.Stamp(brush(vpt, "sphere", c, rotation(0.1 * s), scale=0.6), SUBTRACT if s % 2 == 0 else UNION, 0.004 if s % 3 == 2 else 0.0))
    return out


def single_cases(vpt):
    """every type x every op x both blends as one stamp, on a frame that is rotated and translated; odd ones on the region BOX"""
    out = {}
    for t, kind in enumerate(TYPES):
        for name, op in OPS.items():
            for blend in BLENDS:
                axes = rotation(0.6 + 0.2 * t, 0.35) if kind != "plane" else rotation(0.3, 0.5)
                region = BOX if (t + op) % 2 else None
                out[f"{kind}-{name}-{blend:g}"] = (BUNNY, [vpt.Stamp(brush(vpt, kind, CENTRE, axes), op, blend)], region, None, None)
    return out


def shape_cases(vpt):
    out = {"one_voxel": (BUNNY, shape_stamps(vpt, ONE), ONE, None, None),
           "region": (BUNNY, shape_stamps(vpt, REGION), REGION, None, None),
           "rows": (BUNNY, shape_stamps(vpt, ROWS), ROWS, None, None),
           "whole": (BUNNY, shape_stamps(vpt, WHOLE), WHOLE, None, None),
           "stroke_1": (BUNNY, stroke(vpt, 33)[8:9], BOX, None, None),   # one stamp of the stroke below that carves the bunny
           "stroke_33": (BUNNY, stroke(vpt, 33), BOX, None, None),
           "identity_axes": (BUNNY, [vpt.Stamp(brush(vpt, "box", (0.05, 0.01, 0.05)), SUBTRACT)], None, None, None),
           "replace_then_more": (BUNNY, [vpt.Stamp(brush(vpt, "torus", CENTRE, rotation()), REPLACE, 0.5), vpt.Stamp(brush(vpt, "sphere"), UNION, 0.01)], BOX, None, None),
           # a grid of the caller's own: the brush sits where that grid puts the middle of the volume
           "own_grid": (BUNNY, [vpt.Stamp(brush(vpt, "sphere", (0.07, 0.03, 0.076)), SUBTRACT)], None, (-0.01, 0.002, 0.0), (0.004, 0.0035, 0.0038))}
    return out


def cases(vpt):
    return {**single_cases(vpt), **shape_cases(vpt)}


SINGLE_NAMES = [f"{kind}-{name}-{blend:g}" for kind in TYPES for name in OPS for blend in BLENDS]
SHAPE_NAMES = ["one_voxel", "region", "rows", "whole", "stroke_1", "stroke_33", "identity_axes", "replace_then_more", "own_grid"]
NAMES = SINGLE_NAMES + SHAPE_NAMES


def apply(host, case):
    volume, stamps, region, origin, step = case
    return host.sculpt_volume(volume, stamps, region=region, origin=origin, step=step)


# ---- the rule again, in numpy: float32 operation by operation ----------------------------------------------------------------------------
def brush_distance(vpt, sdf, points):
    """vpth_sculpt_eval: the distance of `sdf` at (n, 3) float32 points of its local frame"""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    out = np.zeros(len(points), F)
    assert vpt.host.vpth_sculpt_eval(C.byref(sdf), points.ctypes.data, len(points), out.ctypes.data) == 0
    return out


def to_local(sdf, p):
    """transform_point(frame, p) = frame.x * p.x + frame.y * p.y + frame.z * p.z + frame.o, summed from the left, per component"""
    fx, fy, fz, fo = (np.array(v[:], F) for v in (sdf.frame.x, sdf.frame.y, sdf.frame.z, sdf.frame.o))
    return np.stack([((fx[k] * p[:, 0] + fy[k] * p[:, 1]).astype(F) + fz[k] * p[:, 2]).astype(F) + fo[k] for k in range(3)], axis=1).astype(F)


def smin(x, y, k):
    k = F(k)
    with np.errstate(invalid="ignore"):
        m = np.where(x < y, x, y).astype(F)
        d = (x - y).astype(F)
        ad = np.where(d < 0, -d, d).astype(F)
        t = (k - ad).astype(F)
        h = (np.where(t > 0, t, F(0)).astype(F) / k).astype(F)
        return (m - (((h * h).astype(F) * k).astype(F) * F(0.25)).astype(F)).astype(F)


def combine(op, k, a, b):
    """a: the resident values, b: the brush distances"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    with np.errstate(invalid="ignore"):
        if op == REPLACE:
            return b.copy()
        if k > 0:
            return smin(a, b, k) if op == UNION else -smin(b, -a, k) if op == SUBTRACT else -smin(-a, -b, k)
        if op == UNION:
            return np.where(a < b, a, b).astype(F)
        if op == SUBTRACT:
            return np.where(-b > a, -b, a).astype(F)
        return np.where(a > b, a, b).astype(F)


def replay(vpt, grid, res, case):
    """what a case makes of the (d, h, w) grid of a volume with `res`: the whole new grid"""
    _, stamps, region, origin, step = case
    d, h, w = grid.shape
    lo, size = ((0, 0, 0), (w, h, d)) if region is None else region
    origin = np.zeros(3, F) if origin is None else np.asarray(origin, F)
    step = np.array([F(res) * F(n) / F(max(1, n - 1)) for n in (w, h, d)], F) if step is None else np.asarray(step, F)
    axis = [(origin[k] + (np.arange(lo[k], lo[k] + size[k]).astype(F) * step[k]).astype(F)).astype(F) for k in range(3)]
    z, y, x = np.meshgrid(axis[2], axis[1], axis[0], indexing="ij")
    p = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1).astype(F)
    out = grid.copy()
    box = out[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]]
    v = box.reshape(-1).copy()
    for s in stamps:
        v = combine(int(s.op), float(s.blend), v, brush_distance(vpt, s.brush, to_local(s.brush, p)))
    box[...] = v.reshape(box.shape)
    return out
