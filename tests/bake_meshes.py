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


def spiky(height, subdivisions=0, radius=0.35):
    """an icosphere with every face replaced by three triangles that meet at a new vertex, the face's centroid pushed out to
    radius * (1 + height): acute convex apexes, concave valleys along the old edges, saddles at the old vertices.  Not convex:
    confirm its winding with sdf_exact.winding, not with check_outward."""
    verts, tris = icosphere(subdivisions, radius)
    v = verts.astype(np.float64)
    mid = v[tris].mean(axis=1)
    mid *= radius * (1 + height) / np.linalg.norm(mid, axis=1, keepdims=True)
    out = []
    for i, (a, b, c) in enumerate(tris):
        m = len(v) + i
        out += [(a, b, m), (b, c, m), (c, a, m)]
    return np.concatenate([v, mid]).astype(F), np.array(out, np.int32)


def fan_spike(k, apex, r=0.3):
    """a tetrahedron on the base B0 B1 B2 (in z = -0.4, on a circle of radius r at the angles pi/2 + i 2 pi / 3) whose edge B0 B1
    carries k - 1 extra points: the side (apex, B0, B1) is a fan of k triangles from the apex, the base a fan of k triangles from
    B2, the two other sides stay whole.  2 k + 2 triangles; the apex and B2 see many narrow angles on one side and one wide angle
    on the others, which is what tells angle weights from plain sums."""
    ang = np.pi / 2 + np.arange(3) * (2 * np.pi / 3)
    base = np.stack([r * np.cos(ang), r * np.sin(ang), np.full(3, -0.4)], axis=1)
    rail = [base[0] + (base[1] - base[0]) * (j / k) for j in range(k + 1)]   # B0, the extra points, B1
    rail[k] = base[1]
    verts = np.array([np.asarray(apex, np.float64), base[2]] + rail)
    A, B2, P = 0, 1, lambda j: 2 + j   # noqa: E731
    tris = [(A, P(j), P(j + 1)) for j in range(k)] + [(B2, P(j + 1), P(j)) for j in range(k)] + [(A, P(k), B2), (A, B2, P(0))]
    return verts.astype(F), np.array(tris, np.int32)


BIPYRAMID_TURN = (0.37, -0.52, 0.29)   # a fixed generic rotation, as a rotation vector (axis * angle in radians)


def rotation(vector):
    """the rotation matrix of a rotation vector (Rodrigues)"""
    w = np.asarray(vector, np.float64)
    t = np.linalg.norm(w)
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / t
    return np.eye(3) + np.sin(t) * k + (1 - np.cos(t)) * (k @ k)


def flat_bipyramid(n=720, h=0.02, turn=None, scale=1.0, offset=0.0):
    """a rim of n points on the unit circle in z = 0 and the apexes (0, 0, +-h): 2 n needle triangles (n = 720: about 1 : 115) that
    meet at the rim under less than 3 degrees.  turn / scale / offset: the same mesh rotated by the rotation vector, then scaled,
    then moved - with BIPYRAMID_TURN, 1000 and 1000 the stress case of DESIGN.md §16's pruning margin."""
    ang = np.arange(n) * (2 * np.pi / n)
    verts = np.concatenate([np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], axis=1), [[0, 0, h], [0, 0, -h]]])
    top, bottom = n, n + 1
    tris = [(i, (i + 1) % n, top) for i in range(n)] + [((i + 1) % n, i, bottom) for i in range(n)]
    if turn is not None:
        verts = verts @ rotation(turn).T
    return (verts * scale + offset).astype(F), np.array(tris, np.int32)


# the meshes with teeth: name -> (generator, offset of the grid).  On a box every feature is a right angle and a wrong pseudonormal
# still gives the right sign; on these it does not (tests/test_bake_sdf_host.py).
TOOTHED = {
    "spiky_1.0": (lambda: spiky(1.0, 0, 0.35), 0.0137),
    "spiky_2.0": (lambda: spiky(2.0, 0, 0.25), 0.0137),
    "spiky_0.8_fine": (lambda: spiky(0.8, 1, 0.4), 0.0171),   # with 0.0137 a point of the 21^3 grid lies 2.6e-6 from the surface
    "fan_8": (lambda: fan_spike(8, (0.55, 0.1, 0.8)), 0.0137),
    "fan_16": (lambda: fan_spike(16, (0.8, 0.3, 0.5)), 0.0137),
}


def toothed_grid(name, whd):
    """(origin, step) of the grid over [-1, 1]^3 moved by the mesh's offset, whd an int or (w, h, d): no sample point within 1e-5 of the
    surface at 21^3 and 25^3, which the tests assert from the float64 reference before they compare a sign"""
    whd = np.broadcast_to(np.asarray(whd), (3,))
    return F(-1 + TOOTHED[name][1]), (2 / (whd - 1)).astype(F)


def bipyramid_grid(scale=1.0, offset=0.0):
    """(whd, origin, step) of the 24^3 grid around flat_bipyramid: for the unit copy a slab around the disc, 23 steps over
    [-1.1, 1.1] in x and y and over [-0.12, 0.12] in z (three layers cut the inside); for a turned copy a cube"""
    if scale == 1.0 and offset == 0.0:
        return 24, F([-1.1 + 0.0137, -1.1 + 0.0137, -0.12 + 0.00137]), F([2.2 / 23, 2.2 / 23, 0.24 / 23])
    return 24, F((-1.1 + 0.0137) * scale + offset), F(2.2 * scale / 23)


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
