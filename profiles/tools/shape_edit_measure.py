"""vpt_scene_update_shapes measured against what the library offered for the same change before it: vpt_scene_destroy and
vpt_scene_create on the edited descriptor.

Per workload - 05_head1ss_sub with a 300-triangle prop added, and with its head replaced by itself; 03_volume with a lamp's mesh
replaced; crowd_scene(4096) with one small shape replaced - the wall-clock time of the vpt_scene_update_shapes call and of destroy +
create of the edited descriptor (the host mirror's own work - replace / erase / push_back, make_bvh of the new shapes, make_lights,
the flatten - is timed apart: both ways need it), both in ONE process in interleaved rounds, median and minimum of --repeat rounds
after --discard warm-up rounds; the launches, the bytes of both directions and the device time of the call
(vpt_scene_update_stats).  Every round starts from the workload's own scene: the edit is undone by its inverse, untimed, on the host
and on the edited handle.  In every round the shape, instance and light table hashes are checked against the fresh handle's.
No threshold is set for any time.  One JSON line per record, and the list in <out>/shape_edit_measure.json.

  python profiles/tools/shape_edit_measure.py [--out DIR (default .)] [--repeat 12] [--discard 2] [--workloads a,b]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vpt_loader  # noqa: E402

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
ELEMENTS = ("triangles", "quads", "points", "lines")


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "n": len(xs)}


def crowd(tmp):
    import synth_scenes
    return synth_scenes.crowd_scene(tmp, 4096)[0]


def mesh_of(h, shape):
    """the arrays of a shape as add_shape / set_shape take them"""
    a = h.shape_arrays(shape)
    return {k: (v if len(v) else None) for k, v in a.items()}


def add_prop(h):
    import shape_edits as S
    h.add_shape(**S.blob(300, seed=21, scale=0.25))


def replace_largest_by_itself(h):
    """the shape with the most elements (the head's 144 k triangles) set to its own arrays: everything of it is made anew"""
    sizes = [max(len(h.shape_arrays(s)[k]) for k in ELEMENTS) for s in range(h.count("shapes"))]
    shape = int(np.argmax(sizes))
    h.set_shape(shape, **mesh_of(h, shape))


def replace_lamp(h):
    import shape_edits as S
    h.set_shape(S.AREALIGHT1, **S.lamp(3))


def replace_small(h):
    import shape_edits as S
    h.set_shape(S.TRI_LEAF, **S.blob(5, seed=12))


# name -> (scene: a golden file or a function of a temporary directory, the edit through the HostScene setters)
WORKLOADS = {
    "05_head1ss_sub_add_prop300": ("05_head1ss_sub/head1ss_sub.json", add_prop),
    "05_head1ss_sub_replace_head": ("05_head1ss_sub/head1ss_sub.json", replace_largest_by_itself),
    "03_volume_replace_lamp": ("03_volume/volume.json", replace_lamp),
    "crowd4096_replace_small": (crowd, replace_small),
}


def undo(h, before, edit):
    """notes on HostScene h the changes that undo `edit`: added shapes off the end, replaced ones set back (`before`: their meshes)"""
    n = h.count("shapes")
    if edit.add:
        h.remove_shapes(range(n - len(edit.add), n))
    for i, m in before.items():
        h.set_shape(i, **m)


def measure(vpt, name, scene, edit_fn, repeat, discard, tmp):
    path = scene(tmp) if callable(scene) else os.path.join(SCENES, scene)
    h = vpt.HostScene(path)
    A, B = vpt.DeviceScene(vpt.HostScene(path), 0), vpt.DeviceScene(h, 0)
    new, host_ms, old, dev_ms, same = [], [], [], [], True
    for r in range(repeat + discard):
        edit_fn(h)
        before = {i: mesh_of(h, i) for i in h._shape_edit.set}
        t0 = time.perf_counter()
        edit = h.update_shapes()   # the host mirror: both ways need the edited descriptor
        desc, curves = h.desc, h.curves
        t1 = time.perf_counter()
        abi, keep = edit.to_abi()
        t2 = time.perf_counter()
        vpt._check(vpt.hip.vpt_scene_update_shapes(A.handle, C.byref(abi)), "vpt_scene_update_shapes")
        t3 = time.perf_counter()
        vpt.hip.vpt_scene_destroy(B.handle)
        B.handle = vpt._p()
        vpt._check(vpt.hip.vpt_scene_create_curves(desc, curves, 0, C.byref(B.handle)), "vpt_scene_create")
        t4 = time.perf_counter()
        launches, moved, ms = A.update_stats()
        same = same and (A.shape_tables_hash(), A.instance_tables_hash(), A.light_tables_hash()) == (B.shape_tables_hash(), B.instance_tables_hash(), B.light_tables_hash())
        if r >= discard:
            new.append((t3 - t2) * 1e3), host_ms.append((t1 - t0) * 1e3), old.append((t4 - t3) * 1e3), dev_ms.append(ms)
        undo(h, before, edit)   # untimed: back to the workload's own scene, on the host and on A
        A.update_shapes(h.update_shapes())
    elements = sum(max((0 if m[k] is None else len(m[k])) for k in ELEMENTS) for m in list(edit.set.values()) + list(edit.add))
    rec = {"workload": name, "shapes": h.count("shapes"), "edit": {"remove": len(edit.remove), "set": len(edit.set), "add": len(edit.add), "elements": int(elements)},
           "update_shapes": stat(new), "update_shapes_device_span": stat(dev_ms), "launches": launches, "bytes_both_directions": moved,
           "destroy_create": stat(old), "host_mirror_either_way": stat(host_ms), "same_tables_as_a_fresh_handle": bool(same)}
    rec["destroy_create_over_update_median"] = rec["destroy_create"]["median_ms"] / rec["update_shapes"]["median_ms"]
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--repeat", type=int, default=12)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    a = ap.parse_args()
    vpt = vpt_loader.load()
    records = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.workloads.split(","):
            scene, edit_fn = WORKLOADS[name]
            records.append(measure(vpt, name, scene, edit_fn, a.repeat, a.discard, os.path.join(tmp, name)))
    os.makedirs(a.out, exist_ok=True)
    json.dump(records, open(os.path.join(a.out, "shape_edit_measure.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
