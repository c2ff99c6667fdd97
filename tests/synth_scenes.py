"""Synthetic scenes that reach the traversal branches the golden scenes never execute (vpt_mesh_kernel.hip.h: traverse()).

  crowd_scene      17 / 33 / ~200 instances of a handful of shared shapes: more than VPT_HOIST_MAX (16) and more than the 32 bits of the
                   `reach` mask, so phase C tests every root box itself; overlapping instances, scene leaves of up to four instances,
                   identity / translation / rotation / non-uniform scale / mirrored frames, quads and triangles, single-leaf shapes and
                   shapes with real BVHs, one small and one large emissive instance (the mesh-light pdf walk on instanced geometry).
  chain_scene      one shape whose BVH the reference's split_middle builder (leaf size 4) grows one primitive per level: a shape BVH
                   tens of levels deep, whose worst-case stack puts the traversal into its HBM-overflow variant without any override.
  deep_scene       instances laid out the same way, two per binary level, so that every quad level of the scene BVH holds three leaf
                   siblings and one internal node: the quad-stack need of the scene BVH passes 255 while its binary depth stays under
                   the create-time limit.  Optionally one instance of a chain shape in the innermost leaf, of a depth that puts the
                   scene exactly at the limit or one past it.

How the chains are laid out.  split_middle splits at the middle of the primitives' centroid box along its longest axis, and the side
below the middle goes first (child 0).  Item i of a chain is placed on axis i % 3 with its centroid at (.., v_i, ..) and 0 on the other
two axes, its box spanning [0, 2 v_i] on its axis and [-1, 1] on the others.  With v_{i+1} = 0.77 v_i the outermost item of a set is
alone above the middle of its axis (0.77^3 * 17/16 < 1/2) and its axis is the longest: every split peels exactly one item off.  The
boxes all reach the corner of the positive octant at the origin, so a ray that crosses the three coordinate planes close to the origin
in the positive direction passes every box and visits the inner part of the chain first: it pushes every sibling on its way down.

Each function writes a scene JSON with OBJ shapes into `dirpath` and returns (path, facts); the facts are computed here from the same
bounding boxes the loader builds its BVHs from (vpt.build_bvh(bboxes, device=None) is the host build the loader uses), with bvh_depth /
quad_need mirroring bvh_depth / build_quad_nodes of vpt_scene_prep.cpp."""
import json
import os

import numpy as np

F = np.float32

STACK_LIMIT = 256        # vpt_scene_prep.cpp: stack_cap (need rounded up to 4) * VPT_BLOCK (64) * 4 bytes must fit 64 KiB
HOIST_MAX = 16           # vpt_mesh_kernel.hip.h VPT_HOIST_MAX
REFERENCE_STACK = 128    # the reference's intersect_bvh keeps 128 nodes per BVH level: a binary depth of 127 at most (depth + 1 entries)
CHAIN_RATIO = 0.77       # v_{i+1} / v_i of a chain (module docstring)


# ---- BVH figures (vpt_scene_prep.cpp) ------------------------------------------------------------------------------------------------
def bvh_depth(nodes) -> int:
    """binary depth of the deepest leaf (root = 0); vpt_scene_prep.cpp bvh_depth"""
    if len(nodes) == 0:
        return 0
    best, todo = 0, [(0, 0)]
    while todo:
        i, d = todo.pop()
        if nodes[i]["internal"]:
            todo += [(int(nodes[i]["start"]), d + 1), (int(nodes[i]["start"]) + 1, d + 1)]
        else:
            best = max(best, d)
    return best


def quad_need(nodes) -> int:
    """worst-case quad-stack entries of a traversal of this BVH: per quad level, the passing grandchildren but the first visited one,
    plus the need of the deepest internal one; vpt_scene_prep.cpp build_quad_nodes (*need)"""
    if len(nodes) == 0 or not nodes[0]["internal"]:
        return 0

    def slots(i):
        out = []
        for side in range(2):
            c = int(nodes[i]["start"]) + side
            out += [int(nodes[c]["start"]), int(nodes[c]["start"]) + 1] if nodes[c]["internal"] else [c]
        return out

    order, todo = [], [0]        # preorder of the binary nodes that become quad nodes; filled bottom-up like the host
    while todo:
        i = todo.pop()
        order.append(i)
        todo += [s for s in reversed(slots(i)) if nodes[s]["internal"]]
    need = {}
    for i in reversed(order):
        sl = slots(i)
        need[i] = len(sl) - 1 + max([need[s] for s in sl if nodes[s]["internal"]], default=0)
    return need[0]


def line_entry_depths(nodes) -> dict:
    """leaf -> stack depth with which a ray that passes every box and is positive along every axis reaches it, in the traversal's own
    form (the first-visited grandchild of a quad node is taken, the others pushed); for a scene BVH: the pop floor (shape_base) the
    instances of that leaf are entered with"""
    out = {}
    if len(nodes) == 0:
        return out
    stack, cur = [], 0
    while True:
        if nodes[cur]["internal"]:
            sl = []
            for side in range(2):       # positive along every axis: child 0 before child 1 on both levels
                c = int(nodes[cur]["start"]) + side
                sl += [int(nodes[c]["start"]), int(nodes[c]["start"]) + 1] if nodes[c]["internal"] else [c]
            stack += sl[:0:-1]
            cur = sl[0]
            continue
        out[cur] = len(stack)
        if not stack:
            return out
        cur = stack.pop()


def stack_need(scene_depth: int, max_shape_depth: int) -> int:
    """the binary-stack figure the create-time limit is checked on (vpt_scene_prep.cpp: need <= 256 is accepted)"""
    return scene_depth + 2 + max_shape_depth + 2


# ---- bounding boxes as the loader computes them (float32, the reference's operation order) -----------------------------------------
def _prim_boxes(verts, faces):
    p = verts[faces]                                         # (n, 3 | 4, 3)
    return np.concatenate([p.min(axis=1), p.max(axis=1)], axis=1).astype(F)


def _transform_bbox(frame, box):
    """transform_bbox(frame, bbox) (yocto_geometry.h): the eight corners through x * p.x + y * p.y + z * p.z + o, merged"""
    fr = np.asarray(frame, F).reshape(4, 3)
    lo, hi = box[:3], box[3:]
    corners = [F([a[0], b[1], c[2]]) for a in (lo, hi) for b in (lo, hi) for c in (lo, hi)]
    pts = np.array([((fr[0] * p[0] + fr[1] * p[1]) + fr[2] * p[2]) + fr[3] for p in corners], F)
    return np.concatenate([pts.min(axis=0), pts.max(axis=0)]).astype(F)


class _Writer:
    """collects shapes / instances / materials and writes the scene; keeps what the BVH figures need"""

    def __init__(self, dirpath):
        self.dir = str(dirpath)
        os.makedirs(os.path.join(self.dir, "shapes"), exist_ok=True)
        self.shapes, self.instances, self.boxes, self.shape_boxes, self.shape_nodes, self.prims = [], [], [], [], [], []
        self.materials = [{"name": "grey", "type": "matte", "color": [0.6, 0.6, 0.6]},
                          {"name": "red", "type": "glossy", "color": [0.7, 0.2, 0.2], "roughness": 0.3},
                          {"name": "lamp_small", "type": "matte", "color": [0, 0, 0], "emission": [30, 28, 24]},
                          {"name": "lamp_large", "type": "matte", "color": [0, 0, 0], "emission": [2, 2.5, 3]}]

    def shape(self, name, verts, faces):
        """faces: (n, 3) triangles or (n, 4) quads (one kind per shape)"""
        import vpt_loader
        vpt = vpt_loader.load()
        verts, faces = np.asarray(verts, F), np.asarray(faces, np.int64)
        lines = ["v " + " ".join(repr(float(c)) for c in v) for v in verts]
        lines += ["f " + " ".join(str(int(k) + 1) for k in f) for f in faces]
        with open(os.path.join(self.dir, "shapes", name + ".obj"), "w") as f:
            f.write("\n".join(lines) + "\n")
        boxes = _prim_boxes(verts, faces)
        nodes, _ = vpt.build_bvh(boxes, device=None)
        self.shapes.append({"name": name, "uri": f"shapes/{name}.obj"})
        self.shape_nodes.append(nodes)
        self.shape_boxes.append(np.concatenate([boxes[:, :3].min(axis=0), boxes[:, 3:].max(axis=0)]).astype(F))
        self.prims.append(len(faces))
        return len(self.shapes) - 1

    def instance(self, shape, frame, material=0):
        frame = [float(F(c)) for c in np.asarray(frame, F).reshape(12)]
        self.instances.append({"name": f"i{len(self.instances)}", "shape": shape, "material": material, "frame": frame})
        self.boxes.append(_transform_bbox(frame, self.shape_boxes[shape]))
        return len(self.instances) - 1

    def write(self, name, camera_frame, env=0.25):
        import vpt_loader
        vpt = vpt_loader.load()
        desc = {"asset": {"version": "4.2"},
                "cameras": [{"name": "cam", "lens": 0.05, "aspect": 1.0, "frame": [float(c) for c in camera_frame]}],
                "environments": [{"name": "sky", "emission": [env, env, env]}] if env else [],
                "materials": self.materials, "shapes": self.shapes, "instances": self.instances}
        path = os.path.join(self.dir, name + ".json")
        with open(path, "w") as f:
            json.dump(desc, f)
        nodes, prims = vpt.build_bvh(np.array(self.boxes, F), device=None)
        used = sorted({i["shape"] for i in self.instances})
        facts = {
            "instances": len(self.instances),
            "shapes": len(self.shapes),
            "scene_nodes": nodes, "scene_prims": prims,
            "scene_depth": bvh_depth(nodes),
            "scene_need4": quad_need(nodes),
            "max_leaf": int(max(n["num"] for n in nodes if not n["internal"])),
            "shape_depth": [bvh_depth(self.shape_nodes[s]) if self.prims[s] > 4 else 0 for s in range(len(self.shapes))],
            "shape_need4": [quad_need(self.shape_nodes[s]) for s in range(len(self.shapes))],
        }
        facts["max_shape_depth"] = max(facts["shape_depth"][s] for s in used)
        facts["max_shape_need4"] = max(facts["shape_need4"][s] for s in used)
        facts["need"] = stack_need(facts["scene_depth"], facts["max_shape_depth"])
        facts["need4"] = facts["scene_need4"] + facts["max_shape_need4"] + 1
        depth_of, todo = {}, [(0, 0)]      # instance id -> binary depth of its scene leaf
        while todo:
            i, d = todo.pop()
            if nodes[i]["internal"]:
                todo += [(int(nodes[i]["start"]), d + 1), (int(nodes[i]["start"]) + 1, d + 1)]
            else:
                for k in range(int(nodes[i]["num"])):
                    depth_of[int(prims[int(nodes[i]["start"]) + k])] = d
        facts["depth_of"] = depth_of
        facts["line_entry_sp"] = max(line_entry_depths(nodes).values())
        return path, facts


def _look_at(eye, target):
    """a camera frame (x, y, z, o) looking from eye at target: the camera looks down its -z"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.concatenate([x, y, z, eye]).astype(F)


# ---- shapes ------------------------------------------------------------------------------------------------------------------------
def _grid(n, quads):
    """an n x n grid over [-1, 1]^2 in the z = 0 plane, slightly warped in z"""
    u = np.linspace(-1, 1, n + 1)
    xx, yy = np.meshgrid(u, u, indexing="ij")
    verts = np.stack([xx, yy, 0.15 * np.sin(2.5 * xx) * np.cos(1.7 * yy)], axis=-1).reshape(-1, 3)
    k = lambda i, j: i * (n + 1) + j   # noqa: E731
    q = np.array([[k(i, j), k(i + 1, j), k(i + 1, j + 1), k(i, j + 1)] for i in range(n) for j in range(n)])
    return verts, q if quads else np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]])


def _blob(rng, n):
    """n small triangles scattered in the unit ball: a BVH several levels deep"""
    c = rng.normal(size=(n, 3))
    c *= (rng.uniform(0, 1, size=(n, 1)) ** (1 / 3)) / np.linalg.norm(c, axis=1, keepdims=True)
    verts = (c[:, None, :] + 0.18 * rng.normal(size=(n, 3, 3))).reshape(-1, 3)
    return verts, np.arange(3 * n).reshape(n, 3)


def chain_geometry(depth):
    """triangles that split_middle peels off one per level: item i on axis i % 3, box [0, 2 w_i] on it and [-1, 1] on the others, the
    innermost leaf holding the last four; two small triangles at the corners (2, 2, 2) and (-2, -2, -2), peeled off first, make the root
    box [-2, 2]^3 (centroid 0: in the deep scene the chain's instance sits in the innermost leaf).  BVH depth = `depth`."""
    verts = [[2, 2, 2], [1.875, 2, 2], [2, 1.875, 2], [-2, -2, -2], [-1.875, -2, -2], [-2, -1.875, -2]]
    faces = [[0, 1, 2], [3, 4, 5]]
    w = 1.0
    for i in range(depth + 2):
        a = i % 3
        w32 = float(F(w))
        tri = np.array([[0, -1, -1], [2 * w32, 1, -1], [0, 1, 1]], np.float64)   # local (along, across1, across2)
        tri = np.roll(tri, a, axis=1)                                             # along -> axis a
        faces.append([len(verts), len(verts) + 1, len(verts) + 2])
        verts += tri.tolist()
        w *= CHAIN_RATIO
    return np.array(verts, F), np.array(faces)


def _slab_geometry(n=24):
    """the deep scene's shape: box [0, 2] x [-1, 1]^2 (centroid (1, 0, 0)), a plane of 2 n^2 triangles at x = 1 facing the rays
    (a BVH of several levels) and two small triangles at the box's far corners that give it its extent along x"""
    u = np.linspace(-1, 1, n + 1)
    yy, zz = np.meshgrid(u, u, indexing="ij")
    verts = np.stack([np.ones_like(yy), yy, zz], axis=-1).reshape(-1, 3)
    k = lambda i, j: i * (n + 1) + j   # noqa: E731
    q = np.array([[k(i, j), k(i + 1, j), k(i + 1, j + 1), k(i, j + 1)] for i in range(n) for j in range(n)])
    faces = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]])
    m = len(verts)
    corner = np.array([[0, 1, 1], [0, 0.875, 1], [0, 1, 0.875], [2, -1, -1], [2, -0.875, -1], [2, -1, -0.875]], np.float64)
    return np.concatenate([verts, corner]).astype(F), np.concatenate([faces, [[m, m + 1, m + 2], [m + 3, m + 4, m + 5]]])


def _shield_geometry():
    """the deep scene's innermost blocker: 2 x 2 grids at x = -1/64, y = -1/64 and z = -1/64 over [-1, 1]^2, in front of every chain item
    for the line rays, plus the two corner triangles that make its box [-2, 2]^3 (centroid 0: it sits in the innermost leaf)"""
    verts, faces = [], []
    u = np.linspace(-1, 1, 3)
    for a in range(3):
        base = len(verts)
        for p in u:
            for q in u:
                verts.append(np.roll([-1 / 64, p, q], a).tolist())
        k = lambda i, j: base + 3 * i + j   # noqa: E731
        for i in range(2):
            for j in range(2):
                faces += [[k(i, j), k(i + 1, j), k(i + 1, j + 1)], [k(i, j), k(i + 1, j + 1), k(i, j + 1)]]
    m = len(verts)
    verts += [[2, 2, 2], [1.875, 2, 2], [2, 1.875, 2], [-2, -2, -2], [-1.875, -2, -2], [-2, -1.875, -2]]
    faces += [[m, m + 1, m + 2], [m + 3, m + 4, m + 5]]
    return np.array(verts, F), np.array(faces)


def _decoy_geometry():
    """an innermost instance the line rays enter but never hit: its box is [-2, 2]^3 (centroid 0), its triangles sit in four clusters
    away from the diagonal, so that a line ray meets a shape BVH none of whose children it passes and pops straight back to the scene
    entries below its pop floor"""
    verts, faces = [], []
    for c in ([1.5, -1.5, 0], [-1.5, 1.5, 0], [0, 1.5, -1.5], [1.5, 0, -1.5]):
        for k in range(3):
            base = np.array(c, np.float64) + 0.125 * k
            faces.append([len(verts), len(verts) + 1, len(verts) + 2])
            verts += [base.tolist(), (base + [0.25, 0, 0]).tolist(), (base + [0, 0.25, 0.25]).tolist()]
    m = len(verts)
    verts += [[2, 2, 2], [1.875, 2, 2], [2, 1.875, 2], [-2, -2, -2], [-1.875, -2, -2], [-2, -1.875, -2]]
    faces += [[m, m + 1, m + 2], [m + 3, m + 4, m + 5]]
    return np.array(verts, F), np.array(faces)


def _axis_frame(axis, v):
    """local x -> world axis `axis` scaled by v, local y / z -> the next two axes (cyclic: det = v > 0)"""
    cols = np.zeros((4, 3), F)
    cols[0, axis] = v
    cols[1, (axis + 1) % 3] = 1
    cols[2, (axis + 2) % 3] = 1
    return cols.reshape(12)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def crowd_scene(dirpath, count, seed=5):
    """`count` instances of seven shared shapes (see the module docstring).  Facts: the BVH figures plus
    `frame_kinds` (kind -> number of instances) and `lights` (instance ids of the two emissive instances, small and large)."""
    rng = np.random.default_rng(seed)
    w = _Writer(dirpath)
    tri_leaf = w.shape("tri_leaf", [[-1, -1, 0], [1, -1, 0], [0, 1, 0.3], [0, 0, 1]], [[0, 1, 2], [0, 1, 3], [1, 2, 3]])
    quad_leaf = w.shape("quad_leaf", [[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0], [-1, -1, 1], [1, -1, 1]], [[0, 1, 2, 3], [0, 1, 5, 4]])
    blob = w.shape("blob", *_blob(rng, 160))
    grid_q = w.shape("grid_quads", *_grid(10, True))
    grid_t = w.shape("grid_tris", *_grid(7, False))
    lamp_small = w.shape("lamp_small", [[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], [[0, 1, 2, 3]])
    lamp_large = w.shape("lamp_large", *_grid(6, True))
    kinds = {"identity": 0, "translation": 0, "rotation": 0, "scale": 0, "mirror": 0}
    order = ["identity", "translation", "rotation", "scale", "mirror"]
    shapes = [tri_leaf, quad_leaf, blob, grid_q, grid_t]
    lights = []
    extent = 0.6 + 0.6 * min(1.0, count / 64)             # the bigger crowds spread further: still overlapping, more levels
    for i in range(count):
        if i == 0:
            kind, shape, mat, s = "rotation", lamp_small, 2, 0.08
        elif i == 1:
            kind, shape, mat, s = "translation", lamp_large, 3, 0.35
        else:
            kind, shape, mat, s = order[i % 5], shapes[(i * 7) % 5], i % 2, float(rng.uniform(0.12, 0.3))
        o = rng.uniform(-extent, extent, 3) if kind != "identity" else np.zeros(3)
        if i == 1:
            o = np.array([0.0, 0.9 * extent, -0.2])
        m = np.eye(3)
        if kind in ("rotation", "mirror", "scale"):
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            ang = rng.uniform(0, 2 * np.pi)
            kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
            m = np.eye(3) + np.sin(ang) * kx + (1 - np.cos(ang)) * kx @ kx
        if kind == "scale":
            m = m @ np.diag(rng.uniform(0.5, 1.8, 3))
        if kind == "mirror":
            m = m @ np.diag([1.0, -1.0, 1.0])
        if kind == "identity":
            s = 1.0
        frame = np.concatenate([(m * s)[:, 0], (m * s)[:, 1], (m * s)[:, 2], o])  # columns: the frame's x, y, z axes
        if i == 1:                                          # the large lamp faces down onto the crowd
            frame = np.concatenate([[s, 0, 0], [0, 0, s], [0, -s, 0], o])
        inst = w.instance(shape, frame, mat)
        if mat >= 2:
            lights.append(inst)
        kinds[kind] += 1
    path, facts = w.write(f"crowd_{count}", _look_at([0.4, 0.5, 4.2], [0, 0, 0]))
    facts["frame_kinds"] = kinds
    facts["lights"] = lights
    return path, facts


def chain_scene(dirpath, depth=40):
    """one instance of a chain shape `depth` levels deep over a floor of two triangles.  Facts: the BVH figures; `chain` = its shape id."""
    w = _Writer(dirpath)
    chain = w.shape("chain", *chain_geometry(depth))
    floor = w.shape("floor", [[-4, -1.5, -4], [4, -1.5, -4], [4, -1.5, 4], [-4, -1.5, 4]], [[0, 1, 2], [0, 2, 3]])
    w.instance(floor, np.concatenate([np.eye(3).reshape(-1), [0, 0, 0]]), 0)
    w.instance(chain, np.concatenate([np.eye(3).reshape(-1), [0, 0, 0]]), 1)
    path, facts = w.write("chain", _look_at([-2.2, -1.8, -2.6], [0.3, 0.3, 0.3]))
    facts["chain"] = chain
    return path, facts


def deep_scene(dirpath, levels=86, chain_depth=None, name="deep", blocker="shield"):
    """2 * levels chain items of instances of one slab shape (module docstring): item 2q (a pair of leaves: three instances at v and two
    at v * 17/16) and item 2q + 1 (one instance) are the three leaf siblings of quad level q.  The innermost leaf holds two small slab
    instances, a shield (the nearest hit of every line ray, so that their hits show that they reached the innermost leaf: the chain
    items' own planes are too close to each other to be told apart at the rays' distances) and, with `chain_depth`, an instance of a
    chain shape of that depth.  blocker = "decoy" puts an instance there that the line rays enter but never hit instead of the shield:
    they walk on to the chain items' planes and to siblings far down the stack.  The shapes are listed smallest first: their leaf records precede the slab's 1154.  Facts: the BVH figures and `deepest` (the instances of the innermost leaf).  Every scene's facts carry `depth_of`
    (instance id -> binary depth of its scene leaf) and `line_entry_sp` (the largest of line_entry_depths of the scene BVH)."""
    w = _Writer(dirpath)
    if chain_depth is not None:
        chain = w.shape("chain", *chain_geometry(chain_depth))
    shield = w.shape(blocker, *(_shield_geometry() if blocker == "shield" else _decoy_geometry()))
    slab = w.shape("slab", *_slab_geometry())
    v = 0.5
    for i in range(2 * levels):
        a = i % 3
        if i % 2 == 0:
            for k in range(5):
                w.instance(slab, np.concatenate([_axis_frame(a, float(F(v) * (F(17) / F(16) if k >= 3 else F(1))))[:9], [0, 0, 0]]), k % 2)
        else:
            w.instance(slab, np.concatenate([_axis_frame(a, v)[:9], [0, 0, 0]]), 1)
        v *= CHAIN_RATIO
    core = [w.instance(slab, np.concatenate([_axis_frame(0, v)[:9], [0, 0, 0]]), 0),
            w.instance(slab, np.concatenate([_axis_frame(1, v * 0.5)[:9], [0, 0, 0]]), 1),
            w.instance(shield, np.concatenate([np.eye(3).reshape(-1), [0, 0, 0]]), 0)]
    if chain_depth is not None:
        core.append(w.instance(chain, np.concatenate([np.eye(3).reshape(-1), [0, 0, 0]]), 0))
    path, facts = w.write(name, _look_at([-1.5, -1.2, -1.8], [0.05, 0.05, 0.05]))
    facts["deepest"] = core
    return path, facts


def line_rays(rng, n, spread=0.15):
    """rays that cross the three coordinate planes close to the origin, in the positive octant's direction: along the line of a chain's
    boxes (module docstring), they pass every box and walk the inner part of the chain first"""
    o = -rng.uniform(0.02, spread, size=(n, 3))
    d = rng.uniform(0.45, 1.0, size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], axis=1).astype(F)
