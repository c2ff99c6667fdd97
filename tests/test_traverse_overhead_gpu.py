"""The per-step bookkeeping of traverse() (vpt_mesh_kernel.hip.h): the group form of the node phase keeps its level's base address for a whole
call, leaves its loop by one test at the bottom, and pops the top stack entry in straight-line code before it enters the pop loop.  None
of it may change a bit: vpt_intersect against the CPU oracle on instance, element, uv and distance, for whole-scene and single-instance
queries, with dense waves (the own form first) and with 12 / 3 / 1 real rays per wave (the group form from the first node on), on

  five      one shape of 5 quads: a single quad node with an empty slot and a leaf in a slot;
  seventeen one shape of 17 quads: two quad levels;
  onion     64 concentric cubes of 6 quads each around the origin, rays from inside the innermost: after the hit on the innermost cube the
            entries stacked for the outer ones fail their pop test one after another (the straight-line pop, then the loop);
  pair      two instances of two different shapes: the second shape's node base and leaf base are not 0, and a ray leaves one level and
            enters the other;
  volume    tests/03_volume with 2 000 rays from a sphere around it;

and all of it once more in a child process under VPT_STACK_LDS=4 (read when a scene is created), where pops cross from HBM into LDS.
A model of the stack discipline in Python, checked against the oracle's hits, shows on the CPU that the onion does what it is there for."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import SCENE_03
from kat_lib import edge_rays
from synth_scenes import _Writer, _look_at

F = np.float32
FAR = F([1e3, 1e3, 1e3, 0.57735027, 0.57735027, 0.57735027])   # misses every scene here: its lane finishes at once
BOX_K = 1.00000024
IDENTITY = np.concatenate([np.eye(3).reshape(-1), [0, 0, 0]])
SCENES = ("five", "seventeen", "onion", "pair", "volume")


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def _strip(n, seed):
    """n unit-ish quads scattered in [-1, 1]^3, each facing a random direction"""
    rng = np.random.default_rng(seed)
    verts, faces = [], []
    for _ in range(n):
        c = rng.uniform(-0.8, 0.8, 3)
        a = rng.normal(size=3)
        a /= np.linalg.norm(a)
        b = np.cross(a, rng.normal(size=3))
        b /= np.linalg.norm(b)
        s = rng.uniform(0.15, 0.35)
        faces.append([len(verts) + k for k in range(4)])
        verts += [c - s * a - s * b, c + s * a - s * b, c + s * a + s * b, c - s * a + s * b]
    return np.array(verts, F), np.array(faces)


def _onion(shells=64):
    """cube i has half-width 1 + i / 8: 6 quads each"""
    verts, faces = [], []
    for i in range(shells):
        r = 1.0 + i / 8.0
        for axis in range(3):
            for side in (-r, r):
                quad = [[side, -r, -r], [side, r, -r], [side, r, r], [side, -r, r]]
                faces.append([len(verts) + k for k in range(4)])
                verts += [np.roll(p, axis).tolist() for p in quad]
    return np.array(verts, F), np.array(faces)


def _write_scene(dirpath, name):
    """writes scene `name` under dirpath -> (its path, the writer)"""
    w = _Writer(os.path.join(str(dirpath), name))
    if name == "five":
        w.instance(w.shape("five", *_strip(5, 11)), IDENTITY)
    elif name == "seventeen":
        w.instance(w.shape("seventeen", *_strip(17, 12)), IDENTITY)
    elif name == "onion":
        w.instance(w.shape("onion", *_onion()), IDENTITY)
    else:   # pair: the first shape has quad nodes and leaf records of its own, so the second's bases are not 0
        a, b = w.shape("a", *_strip(23, 13)), w.shape("b", *_strip(41, 14))
        w.instance(a, np.concatenate([np.eye(3).reshape(-1), [-0.6, 0, 0]]))
        c, s = np.cos(0.7), np.sin(0.7)
        w.instance(b, np.concatenate([[c, s, 0], [-s, c, 0], [0, 0, 1], [0.7, 0.1, 0]]))
    path, _ = w.write(name, _look_at([0, 0, 6], [0, 0, 0]))
    return path, w


def _sphere_rays(rng, n, radius, aim):
    """from a sphere of `radius` around the origin towards points within `aim` of it"""
    o = rng.normal(size=(n, 3))
    o *= radius / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.uniform(-aim, aim, size=(n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], axis=1).astype(F)


def _rays(name):
    rng = np.random.default_rng(21)
    if name == "volume":
        return _sphere_rays(rng, 2000, 2.0, 0.6) + F([0, 0.2, 0, 0, 0, 0])
    if name == "onion":   # from inside the innermost cube, outwards; edge-case rays from there too
        inner = np.concatenate([rng.uniform(-0.5, 0.5, size=(1024, 3)), rng.normal(size=(1024, 3))], axis=1).astype(F)
        inner[:, 3:] /= np.linalg.norm(inner[:, 3:], axis=1, keepdims=True)
        return np.concatenate([inner, edge_rays(rng, (-0.9, -0.9, -0.9), (0.9, 0.9, 0.9), 1024)])
    lo, hi = ((-1.6, -1.2, -1.2), (1.7, 1.3, 1.2)) if name == "pair" else ((-1.1, -1.1, -1.1), (1.1, 1.1, 1.1))
    return np.concatenate([_sphere_rays(rng, 1024, 3.0, 1.0), edge_rays(rng, lo, hi, 1024)])


def _batches(rays):
    """dense waves, then waves that keep 12 / 3 / 1 of their 64 rays (the others miss the scene)"""
    lane = np.arange(len(rays)) % 64
    out = [("dense", rays)]
    for keep in (12, 3, 1):
        sparse = rays.copy()
        sparse[(lane * 7 + 3) % 64 >= keep] = FAR
        out.append((f"{keep} per wave", sparse))
    return out


# ---- the check itself (also what the child process runs) ----------------------------------------------------------------------------
_REFERENCE = {}   # scene name -> (host scene, [(batch name, rays, instance, oracle ids, oracle uvt)]): computed once, never changed


def _reference(vpt, oracle, dirpath, name):
    if name not in _REFERENCE:
        scene = vpt.HostScene(SCENE_03 if name == "volume" else _write_scene(dirpath, name)[0])
        cases = []
        for bname, batch in _batches(_rays(name)):
            for instance in (-1, 0, 1)[:3 if name == "pair" else 2]:
                ids, uvt = oracle.oracle_intersect(scene, batch, instance)
                ids.setflags(write=False), uvt.setflags(write=False)
                cases.append((bname, batch, instance, ids, uvt))
        _REFERENCE[name] = (scene, cases)
    return _REFERENCE[name]


def _check_scene(vpt, oracle, dirpath, name):
    scene, cases = _reference(vpt, oracle, dirpath, name)
    dev = vpt.DeviceScene(scene, 0)
    for bname, batch, instance, rids, ruvt in cases:
        ids, uvt = dev.intersect(batch, instance)
        if bname == "dense" and instance < 0:
            assert (rids[:, 0] >= 0).mean() > 0.05, (name, "the rays hit too little", float((rids[:, 0] >= 0).mean()))
        bad = np.nonzero((ids != rids).any(axis=1) | (uvt.view(np.uint32) != ruvt.view(np.uint32)).any(axis=1))[0]
        assert len(bad) == 0, (name, bname, instance, len(bad), bad[:8].tolist(), ids[bad[:3]].tolist(), rids[bad[:3]].tolist(),
                               uvt[bad[:3]].tolist(), ruvt[bad[:3]].tolist())


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("traverse_overhead")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_intersect_is_bit_identical(vpt, oracle, scene_dir, monkeypatch, name):
    monkeypatch.delenv("VPT_STACK_LDS", raising=False)
    monkeypatch.delenv("VPT_NO_GROUP_FORMS", raising=False)
    _check_scene(vpt, oracle, scene_dir, name)


@pytest.mark.gpu
def test_intersect_is_bit_identical_with_four_stack_entries_in_lds(scene_dir):
    """every scene again in a process of its own under VPT_STACK_LDS=4: the overflow-stack instance, pops across the HBM / LDS boundary"""
    env = {k: v for k, v in os.environ.items() if k != "VPT_NO_GROUP_FORMS"}
    env["VPT_STACK_LDS"] = "4"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(scene_dir)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.count("equal bits") == len(SCENES), r.stdout[-2000:]


# ---- the onion on the CPU: a model of the stack discipline, tied to the oracle by its hits ---------------------------------------------
def _hit_quad(o, d, p, tmax):
    """distance of the nearest hit of the quad's two triangles (p0 p1 p3, p2 p3 p1) within (1e-4, tmax], or None"""
    best = None
    for a, b, c in ((p[0], p[1], p[3]), (p[2], p[3], p[1])):
        e1, e2 = b - a, c - a
        pv = np.cross(d, e2)
        det = e1 @ pv
        if det == 0:
            continue
        tv = o - a
        u = (tv @ pv) / det
        qv = np.cross(tv, e1)
        v = (d @ qv) / det
        t = (e2 @ qv) / det
        if u < 0 or u > 1 or v < 0 or u + v > 1 or t < 1e-4 or t > tmax:
            continue
        tmax, best = t, t
    return best


def _walk(nodes, prims, verts, faces, o, d):
    """the quad-node traversal of one shape (file header of vpt_mesh_kernel.hip.h) in float64: -> (element, distance, longest run of pops
    rejected one after another)"""
    inv = 1.0 / d

    def entry(i, tmax):
        a, b = (nodes[i]["bbox_min"] - o) * inv, (nodes[i]["bbox_max"] - o) * inv
        t0, t1 = max(np.minimum(a, b).max(), 1e-4), min(np.maximum(a, b).min(), tmax) * BOX_K
        return t0 if t0 <= t1 else None

    tmax, element, longest, stack = np.inf, -1, 0, []
    cur = 0 if entry(0, tmax) is not None else None
    while cur is not None:
        n = nodes[cur]
        nxt = None
        if n["internal"]:
            order = []
            for side in ((1, 0) if d[n["axis"]] < 0 else (0, 1)):
                c = int(n["start"]) + side
                if nodes[c]["internal"]:
                    order += [int(nodes[c]["start"]) + m for m in ((1, 0) if d[nodes[c]["axis"]] < 0 else (0, 1))]
                else:
                    order.append(c)
            passing = [(g, entry(g, tmax)) for g in order]
            passing = [(g, t0) for g, t0 in passing if t0 is not None]
            if passing:
                nxt = passing[0][0]
                stack += passing[:0:-1]
        else:
            for k in range(int(n["start"]), int(n["start"]) + int(n["num"])):
                t = _hit_quad(o, d, verts[faces[prims[k]]].astype(np.float64), tmax)
                if t is not None:
                    tmax, element = t, int(prims[k])
        run = 0
        while nxt is None and stack:
            g, t0 = stack.pop()
            if t0 <= tmax * BOX_K:
                nxt = g
            else:
                run += 1
                longest = max(longest, run)
        cur = nxt
    return element, tmax, longest


def test_onion_rays_reject_stacked_entries_in_a_row(vpt, oracle, tmp_path):
    """no GPU: the onion's rays do make two or more pops in a row fail, and the model that says so finds the oracle's hits"""
    path, w = _write_scene(tmp_path, "onion")
    scene = vpt.HostScene(path)
    verts, faces = _onion()
    nodes, prims = vpt.build_bvh(np.concatenate([verts[faces].min(axis=1), verts[faces].max(axis=1)], axis=1).astype(F), device=None)
    rays = _rays("onion")[:48]
    ids, uvt = oracle.oracle_intersect(scene, rays)
    runs = []
    for ray, rid, ruvt in zip(rays.astype(np.float64), ids, uvt):
        element, t, longest = _walk(nodes, prims, verts, faces, ray[:3], ray[3:])
        assert rid[0] == 0 and element == rid[1] and abs(t - ruvt[2]) <= 1e-5 * t, (ray, element, t, rid, ruvt)
        runs.append(longest)
    assert max(runs) >= 2 and np.mean(np.array(runs) >= 2) > 0.5, runs


if __name__ == "__main__":   # the child of test_intersect_is_bit_identical_with_four_stack_entries_in_lds
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import oracle_lib
    import vpt_loader
    for scene_name in SCENES:
        _check_scene(vpt_loader.load(), oracle_lib, sys.argv[1], scene_name)
        print(f"{scene_name}: equal bits with VPT_STACK_LDS={os.environ.get('VPT_STACK_LDS')}", flush=True)
