"""vpt_scene_update_instances measured against what the library offered for the same change before it: vpt_scene_destroy and
vpt_scene_create on the edited descriptor.

Per workload - crowd_scene(4096) with one instance added, one removed, 1024 added; 05_head1ss_sub with one more copy of the head;
03_volume with a sphere added - the wall-clock time of the vpt_scene_update_instances call and of destroy + create of the edited
descriptor (the host mirror's own work - erase / push_back, make_bvh's scene level, make_lights, the flatten - is timed apart: both
ways need it), both in ONE process in interleaved rounds, median and minimum of --repeat rounds after --discard warm-up rounds; the
launches, the bytes of both directions and the device time of the call (vpt_scene_update_stats).  Every round starts from the
workload's own scene: the edit is undone by its inverse, untimed, on both handles.  No threshold is set for any time.
One JSON line per record, and the list in <out>/instance_edit_measure.json.

  python profiles/tools/instance_edit_measure.py [--out DIR (default .)] [--repeat 12] [--discard 2] [--workloads a,b]"""
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


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "n": len(xs)}


def crowd(tmp):
    import synth_scenes
    return synth_scenes.crowd_scene(tmp, 4096)[0]


def add(count, shape, material):
    import instance_edits as I

    def edit(h):
        for k in range(count):
            h.add_instance(I.scatter(k), shape(k) if callable(shape) else shape, material)
    return edit


def remove_mid(h):
    h.remove_instances([h.count("instances") // 2])


# name -> (scene: a golden file or a function of a temporary directory, the edit through the HostScene setters)
WORKLOADS = {
    "crowd4096_add1": (crowd, add(1, 2, 0)),
    "crowd4096_remove1": (crowd, remove_mid),
    "crowd4096_add1024": (crowd, add(1024, lambda k: k % 5, 1)),
    "05_head1ss_sub_add1": ("05_head1ss_sub/head1ss_sub.json", add(1, 0, 0)),
    "03_volume_add1": ("03_volume/volume.json", add(1, 1, 2)),
}


def inverse(vpt, before, edit):
    """the InstanceEdit that undoes `edit` on a list that was `before` (an INSTANCE array): added instances off the end, removed ones
    cannot be put back in the middle, so a removal is undone by setting every later survivor back and adding the last"""
    n_kept = len(before) - len(edit.remove)
    if not edit.remove:
        return vpt.InstanceEdit(remove=range(n_kept, n_kept + len(edit.add)), set={i: tuple(before[i]) for i in edit.set})
    first = min(edit.remove)
    return vpt.InstanceEdit(remove=range(n_kept, n_kept + len(edit.add)), set={i: tuple(before[i]) for i in range(first, n_kept)},
                            add=[tuple(r) for r in before[n_kept:]])


def measure(vpt, name, scene, edit_fn, repeat, discard, tmp):
    import instance_edits as I
    path = scene(tmp) if callable(scene) else os.path.join(SCENES, scene)
    h = vpt.HostScene(path)
    A, B = vpt.DeviceScene(vpt.HostScene(path), 0), vpt.DeviceScene(h, 0)
    before = I.instances_of(h)
    new, host_ms, old, dev_ms = [], [], [], []
    for r in range(repeat + discard):
        edit_fn(h)
        t0 = time.perf_counter()
        edit = h.update_instances()   # the host mirror: both ways need the edited descriptor
        desc, curves = h.desc, h.curves
        t1 = time.perf_counter()
        abi, keep = edit.to_abi()
        t2 = time.perf_counter()
        vpt._check(vpt.hip.vpt_scene_update_instances(A.handle, C.byref(abi)), "vpt_scene_update_instances")
        t3 = time.perf_counter()
        vpt.hip.vpt_scene_destroy(B.handle)
        B.handle = vpt._p()
        vpt._check(vpt.hip.vpt_scene_create_curves(desc, curves, 0, C.byref(B.handle)), "vpt_scene_create")
        t4 = time.perf_counter()
        launches, moved, ms = A.update_stats()
        same = A.instance_tables_hash() == B.instance_tables_hash() and A.light_tables_hash() == B.light_tables_hash()
        if r >= discard:
            new.append((t3 - t2) * 1e3), host_ms.append((t1 - t0) * 1e3), old.append((t4 - t3) * 1e3), dev_ms.append(ms)
        back = inverse(vpt, before, edit)   # untimed: back to the workload's own scene, on the host and on A
        for i, rec in back.set.items():
            h.set_instance(i, *rec)
        h.remove_instances(back.remove)
        for rec in back.add:
            h.add_instance(*rec)
        A.update_instances(h.update_instances())
        assert I.instances_of(h).tobytes() == before.tobytes()
    rec = {"workload": name, "instances": len(before), "edit": {"remove": len(edit.remove), "set": len(edit.set), "add": len(edit.add)},
           "update_instances": stat(new), "update_instances_device_span": stat(dev_ms), "launches": launches, "bytes_both_directions": moved,
           "destroy_create": stat(old), "host_mirror_either_way": stat(host_ms), "same_tables_as_a_fresh_handle": bool(same)}
    rec["destroy_create_over_update_median"] = rec["destroy_create"]["median_ms"] / rec["update_instances"]["median_ms"]
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
    json.dump(records, open(os.path.join(a.out, "instance_edit_measure.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
