"""Meshes for the signed-distance bake tests (test_bake_sdf_host.py, test_bake_sdf_gpu.py), made in numpy: closed, outward winding."""
import numpy as np

F = np.float32


def box_mesh(lo, hi):
    """the axis-aligned box [lo, hi]^3 (or per-axis bounds): 8 vertices, 12 triangles"""
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), (3,)), np.broadcast_to(np.asarray(hi, np.float64), (3,))
    verts = np.array([[(hi if (v >> a) & 1 else lo)[a] for a in range(3)] for v in range(8)], F)   # vertex v: bit a set = hi on axis a
    quads = [(0, 4, 6, 2), (1, 3, 7, 5),   # x = lo, x = hi
             (0, 1, 5, 4), (2, 6, 7, 3),   # y = lo, y = hi
             (0, 2, 3, 1), (4, 5, 7, 6)]   # z = lo, z = hi
    tris = []
    for a, b, c, d in quads:
        tris += [(a, b, c), (a, c, d)]
    return verts, np.array(tris, np.int32)


def check_outward(verts, tris):
    """every face normal points away from the centroid (convex meshes) - a guard for the generators here"""
    v = verts.astype(np.float64)
    c = v.mean(axis=0)
    n = np.cross(v[tris[:, 1]] - v[tris[:, 0]], v[tris[:, 2]] - v[tris[:, 0]])
    return bool(np.all(np.einsum("ij,ij->i", n, v[tris].mean(axis=1) - c) > 0))


def unweld(verts, tris):
    """every triangle gets its own three vertices"""
    return verts[tris.reshape(-1)].copy(), np.arange(3 * len(tris), dtype=np.int32).reshape(-1, 3)


def icosphere(subdivisions=2, radius=1.0, center=(0, 0, 0)):
    """20 * 4^subdivisions triangles on a sphere (subdivisions = 2: 320)"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius + np.asarray(center, np.float64)).astype(F), np.array(f, np.int32)


def torus(nu=40, nv=40, major=0.6, minor=0.25):
    """2 * nu * nv triangles, axis z"""
    u = np.arange(nu) * (2 * np.pi / nu)
    w = np.arange(nv) * (2 * np.pi / nv)
    uu, ww = np.meshgrid(u, w, indexing="ij")
    verts = np.stack([(major + minor * np.cos(ww)) * np.cos(uu), (major + minor * np.cos(ww)) * np.sin(uu), minor * np.sin(ww)], axis=-1).reshape(-1, 3)
    k = lambda i, j: (i % nu) * nv + (j % nv)   # noqa: E731
    tris = []
    for i in range(nu):
        for j in range(nv):
            tris += [(k(i, j), k(i + 1, j), k(i + 1, j + 1)), (k(i, j), k(i + 1, j + 1), k(i, j + 1))]
    return verts.astype(F), np.array(tris, np.int32)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def write_volume_scene(path, sdf_name, frame, scale=1.0):
    """a scene with one volume and one instance of it, in the JSON shape of tests/golden/scenes/06_gridsdf_synth: the camera looks
    down -z at the origin from z = 2"""
    import json
    scene = {
        "asset": {"version": "4.2"},
        "cameras": [{"name": "default", "frame": [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 2], "aspect": 1.0, "focus": 2.0}],
        "materials": [{"name": "baked", "type": "glossy", "color": [0.8, 0.8, 0.8], "roughness": 0.5}],
        "volumes": [{"name": "baked", "uri": sdf_name, "binary": True}],
        "vol_instances": [{"name": "baked", "volume": 0, "material": 0, "scale": float(scale), "frame": [float(x) for x in np.asarray(frame).reshape(12)]}],
    }
    with open(path, "w") as f:
        json.dump(scene, f, indent=1)
