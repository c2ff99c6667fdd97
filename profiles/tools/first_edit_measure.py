"""What a resident scene's host mirrors cost and where: vpt_scene_create, the FIRST edit a fresh handle sees, and an edit in the steady
state.  The workloads are those of scene_update_measure.py, texture_update_measure.py and volume_update_measure.py
(their edit functions, imported from them); every edit is a real change - an edit and its inverse take turns.

Per case, --repeat rounds after --discard warm-up rounds, each round on a handle of its own:
 - create:  vpt_scene_destroy of the previous round's handle + vpt_scene_create of the host scene as it stands;
 - first:   the first update call on that handle;
 - steady:  the fourth update call on it.
Wall-clock milliseconds by the host clock (every call returns with the device idle); all values are kept, with their minimum,
median and maximum, so that two builds can be compared against each other's spread.  One JSON line per case, and the list in
<out>/first_edit_measure.json.

  python profiles/tools/first_edit_measure.py [--out DIR (default .)] [--repeat 5] [--discard 1] [--label TEXT]"""
import argparse
import json
import os
import pathlib
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))
import scene_update_measure as S  # noqa: E402
import texture_edits as TE  # noqa: E402
import texture_update_measure as T  # noqa: E402
import volume_update_measure as V  # noqa: E402
import vpt_loader  # noqa: E402


def cases(vpt, work):
    """(name, scene file, function(host scene) -> (apply(h, forward), the host's half: h -> edit, the call measured: (device scene, edit)))"""
    def scene(kind):
        return lambda h: (S.edit_kinds(h)[kind], lambda h: h.update_bvh(), lambda A, edit: A.update(edit))

    def texture(kind):
        return lambda h: (T.workloads(vpt, work)[kind][1], lambda h: h.update_textures(), lambda A, edit: A.update_textures(edit))

    def sdf_frame(h):
        def apply(h, fwd):
            f = h.sdf(V.LAMP)
            f.frame.o[0] += 0.05 if fwd else -0.05
            h.set_sdf(V.LAMP, f)
        return apply, lambda h: h.update_volumes(), lambda A, edit: A.update_volumes(edit)

    scenes = {k: os.path.join(S.SCENES, f) for k, f in S.WORKLOADS.items()}
    sky = os.path.join(TE.SCENES, TE.S03)
    return [("03_volume camera", scenes["03_volume"], scene("camera")), ("03_volume one_instance", scenes["03_volume"], scene("one_instance")),
            ("05_head1ss_sub camera", scenes["05_head1ss_sub"], scene("camera")),
            ("05_head1ss_sub all_vertices_of_largest_shape", scenes["05_head1ss_sub"], scene("all_vertices_of_largest_shape")),
            ("09_curves_dense camera", scenes["09_curves_dense"], scene("camera")), ("09_curves_dense all_instances", scenes["09_curves_dense"], scene("all_instances")),
            ("03_volume sky_dim", sky, texture("sky_dim")), ("03_volume floor_repaint", sky, texture("floor_repaint")),
            ("06_gridsdf_full sdf_frame", V.SCENE, sdf_frame)]


def spread(xs):
    return {"min_ms": float(np.min(xs)), "median_ms": float(np.median(xs)), "max_ms": float(np.max(xs)), "all_ms": [round(float(x), 4) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--discard", type=int, default=1)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    vpt = vpt_loader.load()
    if vpt.device_count() < 1:
        raise SystemExit("first_edit_measure needs a GPU: a time taken elsewhere says nothing")
    records = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, path, make in cases(vpt, pathlib.Path(tmp)):
            h = vpt.HostScene(path)
            apply, host_half, update = make(h)
            A = vpt.DeviceScene(h, 0)
            t = {"create": [], "first": [], "steady": []}
            fwd = True
            for r in range(a.discard + a.repeat):
                t0 = time.perf_counter()
                A.close()
                A = vpt.DeviceScene(h, 0)
                t1 = time.perf_counter()
                took = []
                for _ in range(4):
                    apply(h, fwd)
                    fwd = not fwd
                    edit = host_half(h)
                    t2 = time.perf_counter()
                    update(A, edit)
                    took.append((time.perf_counter() - t2) * 1e3)
                if r >= a.discard:
                    t["create"].append((t1 - t0) * 1e3), t["first"].append(took[0]), t["steady"].append(took[3])
            launches, sent, _ = A.update_stats()
            A.close()
            rec = {"label": a.label, "case": name, "create": spread(t["create"]), "first_edit": spread(t["first"]), "steady_edit": spread(t["steady"]),
                   "launches": launches, "bytes": sent}
            print(json.dumps(rec), flush=True)
            records.append(rec)
    os.makedirs(a.out, exist_ok=True)
    json.dump(records, open(os.path.join(a.out, "first_edit_measure.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
