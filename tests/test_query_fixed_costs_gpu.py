"""The fixed costs of a BVH query in traverse() (vpt_mesh_kernel.hip.h): the root-box pre-pass of scenes with at most 16 instances, which
is only a filter in front of phase C (an instance it lets through, or does not look at, is tested there as the reference does) with
a cheap arm for translated instances and a general arm for the others and for waves that hold a NaN-prone ray; and the group form of
the node step, which reads the visit rank of a grandchild from a table in the quad node (vpt_device.h).  Whatever arm or table a ray
goes through, no bit may change.  (The scenes were chosen for a change of the pre-pass - its general arm taken out - that was measured
and NOT taken, DESIGN.md §4 v22: they now pin the arms as they are.  Of the rank table this test sees a wrong order through ties and
stack positions only; its contents are checked entry by entry on the host, csrc/check_visit_ranks.cpp.)  vpt_intersect against the CPU oracle on instance, element, uv and distance, for whole-scene and
single-instance queries, with dense waves and with 12 / 3 / 1 real rays per wave (the group form from the first node on), on

  mixed      one translated and one rotated instance of different shapes: both arms of the pre-pass in one query;
  rotated    two rotated instances: the general arm alone;
  sixteen    sixteen instances, translated and rotated by turns, of three shapes: the largest scene with a pre-pass;
  seventeen  one more: no pre-pass, every instance is tested in phase C;
  any_slow   `mixed` again with rays whose every wave of 64 holds one ray with a zero direction component (in a lane that the sparse
             batches keep): the whole wave takes the general arm for every instance;
  volume     tests/03_volume with 2 000 rays from a sphere around it;

and all of it once more in a child process under VPT_STACK_LDS=4 (read when a scene is created)."""
import json
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
KEPT_LANE = 27   # (lane * 7 + 3) % 64 == 0: the lane every sparse batch below keeps
SCENES = ("mixed", "rotated", "sixteen", "seventeen", "any_slow", "volume")


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def _strip(n, seed, spread=0.8):
    """n quads scattered in [-1, 1]^3, each facing a random direction"""
    rng = np.random.default_rng(seed)
    verts, faces = [], []
    for _ in range(n):
        c = rng.uniform(-spread, spread, 3)
        a = rng.normal(size=3)
        a /= np.linalg.norm(a)
        b = np.cross(a, rng.normal(size=3))
        b /= np.linalg.norm(b)
        s = rng.uniform(0.15, 0.35)
        faces.append([len(verts) + k for k in range(4)])
        verts += [c - s * a - s * b, c + s * a - s * b, c + s * a + s * b, c - s * a + s * b]
    return np.array(verts, F), np.array(faces)


def _translated(o):
    return np.concatenate([np.eye(3).reshape(-1), o])


def _rotated(axis, angle, o):
    """Rodrigues: a rotation by `angle` about `axis`, then the translation o (frame rows x, y, z, o)"""
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)
    return np.concatenate([r.T.reshape(-1), o])


def _write_scene(dirpath, name):
    w = _Writer(os.path.join(str(dirpath), name))
    if name == "mixed":
        a, b = w.shape("a", *_strip(23, 31)), w.shape("b", *_strip(41, 32))
        w.instance(a, _translated([-0.6, 0.1, 0]))
        w.instance(b, _rotated([0.3, 1, 0.2], 0.7, [0.7, -0.1, 0.2]))
    elif name == "rotated":
        a, b = w.shape("a", *_strip(19, 33)), w.shape("b", *_strip(37, 34))
        w.instance(a, _rotated([1, 0.2, 0], 1.1, [-0.5, 0, 0.3]))
        w.instance(b, _rotated([0, 0.4, 1], -0.6, [0.6, 0.2, -0.2]))
    else:   # sixteen / seventeen: on a 3 x 3 x 2 grid, translated and rotated by turns, three shapes of one / two quad levels and a single leaf
        shapes = [w.shape("a", *_strip(9, 35, 0.6)), w.shape("b", *_strip(21, 36, 0.6)), w.shape("c", *_strip(3, 37, 0.5))]
        rng = np.random.default_rng(38)
        for i in range(16 if name == "sixteen" else 17):
            o = np.array([i % 3 - 1, (i // 3) % 3 - 1, (i // 9) - 0.5]) * 1.3 + rng.uniform(-0.2, 0.2, 3)
            frame = _translated(o) if i % 2 == 0 else _rotated(rng.normal(size=3), rng.uniform(0.3, 2.5), o)
            w.instance(shapes[i % 3], frame)
    return w.write(name, _look_at([0, 0, 8], [0, 0, 0]))[0]


def _sphere_rays(rng, n, radius, aim):
    """from a sphere of `radius` around the origin towards points within `aim` of it"""
    o = rng.normal(size=(n, 3))
    o *= radius / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.uniform(-aim, aim, size=(n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], axis=1).astype(F)


def _rays(name):
    rng = np.random.default_rng(41)
    if name == "volume":
        return _sphere_rays(rng, 2000, 2.0, 0.6) + F([0, 0.2, 0, 0, 0, 0])
    if name == "any_slow":   # no edge-case rays but one per wave: a zero x component, in the lane that every sparse batch keeps
        rays = _sphere_rays(rng, 2048, 3.0, 1.0)
        slow = rays[KEPT_LANE::64]
        slow[:, 3] = 0
        slow[:, 3:] /= np.linalg.norm(slow[:, 3:], axis=1, keepdims=True)
        rays[KEPT_LANE::64] = slow
        return rays
    if name in ("sixteen", "seventeen"):
        return np.concatenate([_sphere_rays(rng, 1024, 5.0, 2.0), edge_rays(rng, (-2.4, -2.4, -1.8), (2.4, 2.4, 1.8), 1024)])
    return np.concatenate([_sphere_rays(rng, 1024, 3.0, 1.0), edge_rays(rng, (-1.6, -1.2, -1.2), (1.7, 1.3, 1.2), 1024)])


def _batches(rays):
    """dense waves, then waves that keep 12 / 3 / 1 of their 64 rays (the others miss the scene)"""
    lane = np.arange(len(rays)) % 64
    out = [("dense", rays)]
    for keep in (12, 3, 1):
        sparse = rays.copy()
        sparse[(lane * 7 + 3) % 64 >= keep] = FAR
        out.append((f"{keep} per wave", sparse))
    return out


def _instances(name):
    """the whole scene, then single-instance queries: a translated and a rotated one, and the last"""
    return {"volume": (-1, 0), "sixteen": (-1, 0, 1, 15), "seventeen": (-1, 0, 1, 16)}.get(name, (-1, 0, 1))


# ---- the check itself (also what the child process runs) ----------------------------------------------------------------------------
_REFERENCE = {}   # scene name -> (host scene, [(batch name, rays, instance, oracle ids, oracle uvt)]): computed once, never changed


def _reference(vpt, oracle, dirpath, name):
    if name not in _REFERENCE:
        scene = vpt.HostScene(SCENE_03 if name == "volume" else _write_scene(dirpath, "mixed" if name == "any_slow" else name))
        cases = []
        for bname, batch in _batches(_rays(name)):
            for instance in _instances(name):
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
            share = float((rids[:, 0] >= 0).mean())
            print(f"{name}: {share:.3f} of the dense rays hit")
            assert share >= 0.05, (name, "the rays hit too little", share)
        bad = np.nonzero((ids != rids).any(axis=1) | (uvt.view(np.uint32) != ruvt.view(np.uint32)).any(axis=1))[0]
        assert len(bad) == 0, (name, bname, instance, len(bad), bad[:8].tolist(), ids[bad[:3]].tolist(), rids[bad[:3]].tolist(),
                               uvt[bad[:3]].tolist(), ruvt[bad[:3]].tolist())


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("query_fixed_costs")


def test_the_chosen_rays_do_what_they_are_there_for(vpt, oracle, scene_dir):
    """no GPU: by the oracle, at least 5 % of every scene's dense rays hit, each instance kind is hit, and every wave of the any_slow
    batch holds its zero-component ray in all four batches"""
    for name in SCENES:
        scene, cases = _reference(vpt, oracle, scene_dir, name)
        rids = next(ids for bname, _, instance, ids, _ in cases if bname == "dense" and instance < 0)
        assert (rids[:, 0] >= 0).mean() >= 0.05, (name, float((rids[:, 0] >= 0).mean()))
        if name != "volume":
            hit = set(rids[rids[:, 0] >= 0, 0].tolist())
            assert {0, 1} <= hit, (name, sorted(hit))   # a translated and a rotated instance (in `rotated`: both rotated)
    for bname, batch, instance, _, _ in _reference(vpt, oracle, scene_dir, "any_slow")[1]:
        waves = batch.reshape(-1, 64, 6)
        assert ((waves[:, :, 3] == 0) & (waves[:, :, 0] != FAR[0])).any(axis=1).all(), bname
    translation_only = [bool(np.array_equal(np.asarray(i["frame"], F)[:9].reshape(3, 3), np.eye(3, dtype=F)))
                        for i in json.load(open(os.path.join(str(scene_dir), "sixteen", "sixteen.json")))["instances"]]
    assert len(translation_only) == 16 and sum(translation_only) == 8


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_intersect_is_bit_identical(vpt, oracle, scene_dir, monkeypatch, name):
    monkeypatch.delenv("VPT_STACK_LDS", raising=False)
    monkeypatch.delenv("VPT_NO_GROUP_FORMS", raising=False)
    _check_scene(vpt, oracle, scene_dir, name)


@pytest.mark.gpu
def test_intersect_is_bit_identical_with_four_stack_entries_in_lds(scene_dir):
    """every scene again in a process of its own under VPT_STACK_LDS=4: the overflow-stack instance of the kernels"""
    env = {k: v for k, v in os.environ.items() if k != "VPT_NO_GROUP_FORMS"}
    env["VPT_STACK_LDS"] = "4"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(scene_dir)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.count("equal bits") == len(SCENES), r.stdout[-2000:]


if __name__ == "__main__":   # the child of test_intersect_is_bit_identical_with_four_stack_entries_in_lds
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import oracle_lib
    import vpt_loader
    for scene_name in SCENES:
        _check_scene(vpt_loader.load(), oracle_lib, sys.argv[1], scene_name)
        print(f"{scene_name}: equal bits with VPT_STACK_LDS={os.environ.get('VPT_STACK_LDS')}", flush=True)
