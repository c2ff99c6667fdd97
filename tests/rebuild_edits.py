"""Cases shared by the BVH-rebuild tests (tests/test_bvh_rebuild_host.py, tests/test_bvh_rebuild_gpu.py) and their fixture script
(tests/golden/make_rebuild_fixtures.py): name -> Case(scene, steps).  A step is (edit, shapes): edit(h) changes a HostScene through
its setters (every formula in float32, step by step, as in tests/scene_edits.py), the caller hands the pending edit out
(update_lights(): a refit, and the light tables where an emitter moved) and then rebuilds `shapes` and the scene BVH.  The LAST step
is the case's own; earlier steps bring the scene into the state the case starts from (chain_unfold starts from the folded chain).
A case is valid only if the rebuilt tree's integer fields differ from the refitted tree's: the host test asserts it for every case."""
import os

import numpy as np

import scene_edits as E
import synth_scenes

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = os.path.join(HERE, "golden", "scenes")
S03 = "03_volume/volume.json"
CURVES = "09_curves_synth/curves.json"
HAIR, DUST = 2, 4          # curves.json: the shape of lines, the shape of points
CHAIN_DEPTH = 40
ALL = "all"


class Case:
    def __init__(self, scene, steps):
        self.scene, self.steps = scene, steps

    def path(self, tmp_path):
        """the scene file: a golden scene, or a synthetic one written into tmp_path"""
        if callable(self.scene):
            return self.scene(tmp_path)
        return os.path.join(SCENES, self.scene)


def twist(p):
    """(x, z) turned about y by the angle 3 y, then x += 0.25 z'^2: float32 throughout, sine and cosine rounded from double"""
    p = np.array(p, F).copy()
    a = (p[:, 1] * F(3)).astype(F)
    c, s = np.cos(a.astype(np.float64)).astype(F), np.sin(a.astype(np.float64)).astype(F)
    x = ((c * p[:, 0]).astype(F) + (s * p[:, 2]).astype(F)).astype(F)
    z = ((c * p[:, 2]).astype(F) - (s * p[:, 0]).astype(F)).astype(F)
    p[:, 0] = (x + (F(0.25) * (z * z).astype(F)).astype(F)).astype(F)
    p[:, 2] = z
    return p


def curves_twist(h):
    for s in (HAIR, DUST):
        h.set_shape_positions(s, twist(h.shape_positions(s)))


def chain_file(tmp_path):
    return synth_scenes.chain_scene(str(tmp_path), depth=CHAIN_DEPTH)[0]


CHAIN = 0   # chain_scene: the chain is its first shape


def blob_positions():
    """the chain's 44 triangles (they share no vertices) as a blob: a shallow tree"""
    count = len(synth_scenes.chain_geometry(CHAIN_DEPTH)[1])
    return np.asarray(synth_scenes._blob(np.random.default_rng(44), count)[0], F)


def chain_fold(h):
    h.set_shape_positions(CHAIN, blob_positions())


def chain_unfold(h):
    h.set_shape_positions(CHAIN, synth_scenes.chain_geometry(CHAIN_DEPTH)[0])


CASES = {
    "vol_light_rotation": Case(S03, [(lambda h: E.rotate_instance(h, E.light_instances(h)[0], 0.4), ())]),
    "vol_last_y005": Case(S03, [(lambda h: E.translate(h, h.count("instances") - 1, dy=0.05), ())]),
    "vol_times2": Case(S03, [(lambda h: E.move_all_vertices(h, E.times2), ALL)]),
    "curves_twist": Case(CURVES, [(curves_twist, (HAIR, DUST))]),
    "chain_fold": Case(chain_file, [(chain_fold, (CHAIN,))]),
    "chain_unfold": Case(chain_file, [(chain_fold, (CHAIN,)), (chain_unfold, (CHAIN,))]),
}


def shapes_of(h, shapes):
    return list(range(h.count("shapes"))) if shapes == ALL else list(shapes)


def integer_fields(h):
    """what a refit keeps and a rebuild may change: start, num, axis, internal of every node, the node counts, the primitive orders"""
    a, b = h.bvh_nodes()
    pa, pb = h.bvh_prims()
    return ([x[k].tobytes() for x in (a, b) for k in ("start", "num", "axis", "internal")], len(a), len(b), pa.tobytes(), pb.tobytes())


def apply(h, case, after_edit=None, after_rebuild=None, refitted=None):
    """every step of `case` on HostScene h.  after_edit(SceneEdit) / after_rebuild(BvhRebuild) see what the device is to be given;
    refitted (a list) receives integer_fields(h) after the last step's refit, before its rebuild."""
    for k, (edit, shapes) in enumerate(case.steps):
        edit(h)
        pending = h.update_lights()
        if after_edit:
            after_edit(pending)
        if refitted is not None and k == len(case.steps) - 1:
            refitted.append(integer_fields(h))
        rebuild = h.rebuild_bvh(shapes_of(h, shapes), True)
        if after_rebuild:
            after_rebuild(rebuild)
