"""The cases of the exact tests of points and lines (tests/curve_exact.py), built at test time: small binary PLYs and one scene JSON
under a directory the caller gives, and seeded float32 ray sets aimed at what the scene holds.

Five line shapes, one per set of vertex attributes, of 16 loose segments with radii 0.01 .. 0.08 and r0 != r1; the attribute-free one also
carries a degenerate segment, a segment of radius 0, a cone ending in r1 = 0 and an axis-aligned segment 2.5 long of radius 0.002.  Three
point shapes of 12 points; the colours-only one also carries a point of radius 0 and two points at one position with different radii (an
exact tie in t).  Every shape sits in its own cell of a 4 x 2 grid in shape space, and the eight appear three times: under the identity
frame, a rotated and translated rigid frame, and a frame scaled by (1.5, 0.7, 1.0).  One small pyramid of triangles; a camera of
aperture 0 that sees all of it; materials without textures."""
import json
import os
import struct

import numpy as np

LINE_VARIANTS = {"lines_all": ("normals", "texcoords", "colors"), "lines_normals": ("normals",), "lines_texcoords": ("texcoords",),
                 "lines_colors": ("colors",), "lines_bare": ()}
POINT_VARIANTS = {"points_all": ("texcoords", "colors"), "points_colors": ("colors",), "points_bare": ()}
VARIANTS = {**LINE_VARIANTS, **POINT_VARIANTS}
FRAMES = ("identity", "rigid", "scaled")
HALF = 0.15     # half the side of a shape's cell


def write_ply(path, positions, normals=None, texcoords=None, colors=None, radius=None, lines=(), points=(), faces=()):
    """binary little-endian PLY with the property names the loader reads (as tests/golden/make_curves_scene.py writes them)"""
    n = len(positions)
    props = [("x", "y", "z")] + ([("nx", "ny", "nz")] if normals is not None else []) + ([("u", "v")] if texcoords is not None else []) + \
            ([("red", "green", "blue", "alpha")] if colors is not None else []) + ([("radius",)] if radius is not None else [])
    cols = [np.asarray(positions, np.float32)] + [np.asarray(a, np.float32).reshape(n, -1) for a in (normals, texcoords, colors, radius) if a is not None]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"] + [f"property float {p}" for group in props for p in group]
    for name, items in (("face", faces), ("line", lines), ("point", points)):
        if len(items):
            head += [f"element {name} {len(items)}", "property list uchar int vertex_indices"]
    body = np.concatenate(cols, axis=1).astype("<f4").tobytes()
    for items in (faces, lines, points):
        for it in items:
            body += struct.pack("<B", len(it)) + np.asarray(it, "<i4").tobytes()
    with open(path, "wb") as f:
        f.write(("\n".join(head + ["end_header"]) + "\n").encode() + body)


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _attributes(g, n, names):
    out = {}
    if "normals" in names:
        out["normals"] = _unit(g.normal(size=(n, 3))) * g.uniform(0.5, 2.0, (n, 1))     # not unit: the lerp is normalised after
    if "texcoords" in names:
        out["texcoords"] = g.uniform(0, 1, (n, 2))
    if "colors" in names:
        out["colors"] = np.concatenate([g.uniform(0.1, 1.0, (n, 3)), np.ones((n, 1))], 1)
    return out


def _rotation(axis, angle):
    x, y, z = _unit(np.asarray(axis, np.float64))
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _frame(M, o):
    """x, y, z, o as the 12 numbers of a scene file, each a float32's exact value"""
    return [float(np.float32(v)) for v in list(np.asarray(M).T.reshape(9)) + list(o)]


def build(root):
    """writes <root>/curves_exact.json and its shapes; returns the scene's path.  Instance ids: 3 * shape + frame in the order of
    VARIANTS x FRAMES, then the pyramid."""
    os.makedirs(os.path.join(root, "shapes"), exist_ok=True)
    g = np.random.default_rng(20)
    for k, (name, attrs) in enumerate(VARIANTS.items()):
        centre = np.array([(k % 4 - 1.5) * 0.4, (k // 4 - 0.5) * 0.4, 0.0])
        if name in LINE_VARIANTS:
            p0 = g.uniform(-HALF, HALF, (16, 3)) * [1, 1, 0.6]
            p1 = np.clip(p0 + _unit(g.normal(size=(16, 3))) * g.uniform(0.08, 0.25, (16, 1)), -HALF, HALF)
            r0, r1 = g.uniform(0.01, 0.08, 16), g.uniform(0.01, 0.08, 16)
            if name == "lines_bare":
                p0 = np.concatenate([p0, [[0.05, 0.1, 0.1], [-0.1, -0.05, 0.12], [0.1, -0.1, 0.1], [-1.6, -0.45, 0.05]]])
                p1 = np.concatenate([p1, [[0.05, 0.1, 0.1], [0.1, -0.02, 0.13], [0.12, 0.05, 0.14], [0.9, -0.45, 0.05]]])
                r0, r1 = np.concatenate([r0, [0.03, 0.0, 0.04, 0.002]]), np.concatenate([r1, [0.05, 0.0, 0.0, 0.002]])
            pos = np.stack([p0, p1], 1).reshape(-1, 3) + centre
            pos[-2:, :] -= centre if name == "lines_bare" else 0      # the long segment runs under the whole grid
            rad = np.stack([r0, r1], 1).reshape(-1)
            write_ply(os.path.join(root, "shapes", name + ".ply"), pos, radius=rad, lines=[[2 * i, 2 * i + 1] for i in range(len(p0))],
                      **_attributes(g, len(pos), attrs))
        else:
            pos, rad = g.uniform(-HALF, HALF, (12, 3)) * [1, 1, 0.6], g.uniform(0.02, 0.06, 12)
            if name == "points_colors":
                pos = np.concatenate([pos, [[0.02, 0.03, 0.12], [-0.08, 0.09, 0.1], [-0.08, 0.09, 0.1]]])
                rad = np.concatenate([rad, [0.0, 0.03, 0.05]])
            write_ply(os.path.join(root, "shapes", name + ".ply"), pos + centre, radius=rad, points=[[i] for i in range(len(pos))],
                      **_attributes(g, len(pos), attrs))
    write_ply(os.path.join(root, "shapes", "pyramid.ply"), [[-0.1, 0, -0.1], [0.1, 0, -0.1], [0.1, 0, 0.1], [-0.1, 0, 0.1], [0, 0.2, 0]],
              faces=[[0, 4, 1], [1, 4, 2], [2, 4, 3], [3, 4, 0]])
    frames = {"identity": _frame(np.eye(3), (0, 0, 0)), "rigid": _frame(_rotation((0.3, 0.5, 0.8), 0.6), (0.05, 1.1, -0.2)),
              "scaled": _frame(np.diag([1.5, 0.7, 1.0]), (0.0, -0.8, 0.1))}
    materials = [{"name": n, "type": "matte", "color": [float(c) for c in np.round(g.uniform(0.2, 0.9, 3), 3)]} for n in list(VARIANTS) + ["pyramid"]]
    shapes = [{"name": n, "uri": f"shapes/{n}.ply"} for n in list(VARIANTS) + ["pyramid"]]
    instances = [{"name": f"{n}_{f}", "shape": k, "material": k, "frame": frames[f]} for k, n in enumerate(VARIANTS) for f in FRAMES]
    instances.append({"name": "pyramid", "shape": len(VARIANTS), "material": len(VARIANTS), "frame": _frame(np.eye(3), (1.25, 0.9, 0.0))})
    camera = {"name": "default", "lens": 0.06, "film": 0.036, "aspect": 1.0, "aperture": 0.0, "focus": 5.0, "frame": _frame(np.eye(3), (0.0, 0.4, 5.0))}
    path = os.path.join(root, "curves_exact.json")
    with open(path, "w") as f:
        json.dump({"asset": {"version": "4.2"}, "cameras": [camera], "materials": materials, "shapes": shapes, "instances": instances}, f, indent=1)
    return path


def instance_of(variant, frame):
    return 3 * list(VARIANTS).index(variant) + FRAMES.index(frame)


PYRAMID = 3 * len(VARIANTS)
FAR = np.array([500.0, 500.0, 500.0, 0.25, 0.5, 0.75], np.float32)   # a ray that misses the scene and is parallel to nothing in it, for sparse waves


def _perpendicular(g, a):
    """unit vectors perpendicular to the rows of a"""
    return _unit(np.cross(a, g.normal(size=a.shape)))


def _to_world(el, o, d):
    return np.concatenate([o @ el.M.T + el.f, d @ el.M.T], 1).astype(np.float32)


def _aimed(g, el, n, only=None, s=(-0.2, 1.2), k=(0.0, 1.3), back=(1.0, 4.0), unit=False):
    """n rays in the shape space of `el` aimed at p0 + (p1 - p0) s +- r k across the element (the offset is perpendicular to the ray and
    to the segment, so that is the closest approach): s over the end caps, a quarter of the k in [0.97, 1.03] where k's range holds 1;
    origins `back` before the target in units of d; half of the directions not unit unless `unit`.  Returns (o, d)."""
    e = g.integers(0, len(el), n) if only is None else g.choice(only, n)
    s = np.zeros(n) if el.points else g.uniform(s[0], s[1], n)
    k = np.where((np.arange(n) % 4 == 0) & (k[1] > 1), g.uniform(0.97, 1.03, n), g.uniform(k[0], k[1], n))
    v = el.p1[e] - el.p0[e]
    d = _unit(g.normal(size=(n, 3)))
    side = _unit(np.cross(d, np.where((np.abs(v).sum(-1) > 0)[:, None], v, g.normal(size=(n, 3)))))
    sc = np.clip(s, 0, 1)
    r = el.r0[e] * (1 - sc) + el.r1[e] * sc
    target = el.p0[e] + v * s[:, None] + side * (r * k * g.choice([-1.0, 1.0], n))[:, None]
    d = d * (1.0 if unit else np.where(np.arange(n) % 2 == 0, 1.0, g.uniform(0.1, 10.0, n))[:, None])
    return target - d * g.uniform(back[0], back[1], (n, 1)), d


def ray_sets(elements, lo, hi, seed=7):
    """{name: (n, 6) float32 rays in world space} over a list of curve_exact.Elements; lo, hi: the scene's box, for kat_lib.edge_rays"""
    import kat_lib
    g = np.random.default_rng(seed)
    lines, points = [el for el in elements if not el.points], [el for el in elements if el.points]
    out = {}
    out["lines"] = np.concatenate([_to_world(el, *_aimed(g, el, 112)) for el in lines])
    out["points"] = np.concatenate([_to_world(el, *_aimed(g, el, 112)) for el in points])
    # with them, 8 per instance parallel to a segment, exactly (the float32 difference of its float32 ends) and to within 1e-6, passing
    # beside it: undecidable against that segment by construction
    rays = []
    for el in lines:
        e = g.choice(np.nonzero(~el.degenerate)[0], 8)             # a degenerate segment gives no direction
        v = (el.p1[e].astype(np.float32) - el.p0[e].astype(np.float32)).astype(np.float64)
        d = np.where((np.arange(8) % 2 == 0)[:, None], v, v + 1e-6 * np.linalg.norm(v, axis=1, keepdims=True) * _perpendicular(g, v + 1e-30))
        o = el.p0[e] - 3 * d + _perpendicular(g, v + 1e-30) * (el.r0[e] * g.uniform(0, 1.3, 8))[:, None]
        rays.append(_to_world(el, o, d))
    out["lines"] = np.concatenate([out["lines"]] + rays)
    out["edge"] = kat_lib.edge_rays(g, lo, hi, 512).astype(np.float32)
    # origins 0.5e-4 to 2e-4 before the closest approach of a ray that passes well inside the radius (unit directions: t is a length);
    # the thin and the empty elements left out
    rays = []
    for el in elements:
        thick = np.nonzero((el.r0 > 0.005) & (el.r1 > 0.005) & ~el.degenerate)[0]
        rays.append(_to_world(el, *_aimed(g, el, 16, only=thick, s=(0.1, 0.9), k=(0.0, 0.5), back=(0.5e-4, 2e-4), unit=True)))
    out["tmin"] = np.concatenate(rays)
    # origins inside a capsule or a sphere, any direction
    rays = []
    for el in elements:
        thick = np.nonzero((el.r0 > 0.005) & (el.r1 > 0.005) & ~el.degenerate)[0]
        e = g.choice(thick, 16)
        s = g.uniform(0, 1, (16, 1)) * (0 if el.points else 1)
        o = el.p0[e] + (el.p1[e] - el.p0[e]) * s + _unit(g.normal(size=(16, 3))) * (np.minimum(el.r0[e], el.r1[e]) * g.uniform(0, 0.9, 16))[:, None]
        rays.append(_to_world(el, o, _unit(g.normal(size=(16, 3))) * g.uniform(0.5, 2.0, (16, 1))))
    out["inside"] = np.concatenate(rays)
    return out


def sparse(rays, keep=3):
    """the waves of 64 keep `keep` of their rays; the others are sent far away (as tests/test_traversal_depth.py does)"""
    out = rays.copy()
    out[(np.arange(len(rays)) % 64 * 7 + 3) % 64 >= keep] = FAR
    return out


def dense_rays():
    """the 512 rays of tests/test_curves_gpu.py::test_intersect_on_dense_strands against 09_curves_synth/dense.json (the same seed and draws)"""
    g = np.random.default_rng(5)
    n = 512
    o = np.stack([g.uniform(-0.5, 0.5, n), np.full(n, 0.15), np.full(n, 1.0)], 1)
    tgt = np.stack([g.uniform(-0.45, 0.45, n), g.uniform(0.0, 0.2, n), g.uniform(-0.45, 0.45, n)], 1)
    return np.concatenate([o, tgt - o], 1).astype(np.float32)


class Case:
    """the scene built under `root` with what the tests share: its Elements, ray sets and one Reference per set (pairs kept)"""
    LO, HI = np.array([-1.6, -1.3, -0.4]), np.array([1.6, 2.0, 0.4])

    def __init__(self, vpt, root):
        import curve_exact
        self.path = build(str(root))
        self.scene = vpt.HostScene(self.path)
        self.elements = curve_exact.curve_instances(self.scene)
        self.sets = ray_sets(self.elements, self.LO, self.HI)
        self.refs = {name: curve_exact.Reference(self.elements, rays, keep=True) for name, rays in self.sets.items()}

    def variant_of(self, instance):
        return list(VARIANTS)[instance // 3] if 0 <= instance < PYRAMID else None

    def material_color(self, instance):
        return np.array(list(self.scene.material(self.scene.instance_ids(instance)[1]).color), np.float64)
