"""vpt_scene_update_volume_set measured against the only way there was to add or remove a volume of a resident scene before it
(DESIGN.md §30): the host edit with its flatten, vpt_scene_destroy and a whole vpt_scene_create - plus vpt_bake_sdf for a baked
addition, whose voxels come back over PCIe and go down again with the new scene.  On 06_gridsdf_full (a 96^3 and a 64^3 grid, four
instances, two SDFs).  Three edits, in ONE process, both sides alternating in every round, median and range of --repeat rounds after
--discard warm-up rounds:
 1. copy: a COPY of the 96^3 grid added with an instance;
 2. remove: that volume and its instance removed again;
 3. bake: tests/golden/scenes/03_volume/shapes/bunny.ply baked at 64^3 into a new volume with an instance (removed again, unmeasured).
New way: the wall-clock time of the vpt_scene_update_volume_set call (host clock; the call returns with the device idle), its device
time by events around the gather and the bake (vpt_scene_update_stats), its launches and its bytes over PCIe.  Old way: a second host
scene takes the same edit (for the bake: vpt_bake_sdf, then the voxels as a FROM_HOST volume), flattens, and a handle is destroyed and
created from it - each timed, and their sum.  The new way's own host edit (the mirror, no flatten of voxels is sent) is reported beside
it and charged to neither side.  After the last round the two handles are compared: voxels of every volume and the six light hashes.
One JSON line per record, and the list in <out>/volume_set_measure.json (profiles/volume_set_measure.json by default).

  python profiles/tools/volume_set_measure.py [--out DIR (default profiles/)] [--repeat 5] [--discard 1]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))
import vpt_loader  # noqa: E402
from bake_sdf_measure import load_shape  # noqa: E402

SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "06_gridsdf_full", "gridsdf_full.json")
FRAME = [1, 0, 0, 0, 1, 0, 0, 0, 1, -0.4, 0.0, 0.0]


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "max_ms": float(np.max(xs)), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--discard", type=int, default=1)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    vpt = vpt_loader.load()
    if vpt.device_count() < 1:
        raise SystemExit("volume_set_measure needs a GPU: a time taken elsewhere says nothing")
    positions, triangles = load_shape(vpt, a.out)
    whd = (64, 64, 64)
    res, origin, step, fit_frame = vpt.fit_volume(positions.min(axis=0), positions.max(axis=0), whd, 2)

    new_host, old_host = vpt.HostScene(SCENE), vpt.HostScene(SCENE)
    A = vpt.DeviceScene(vpt.HostScene(SCENE), 0)
    old = [vpt.DeviceScene(old_host, 0)]

    def copy(h, baked=None):
        h.add_volume_instance(FRAME, h.add_volume(copy_of=0), 3, 0.001)

    def remove(h, baked=None):
        h.remove_volumes([2])
        h.remove_volume_instances([4])

    def bake(h, baked=None):
        v = h.add_volume(bake=(positions, triangles, origin, step), whd=whd, res=res) if baked is None else h.add_volume(baked, res=res)
        h.add_volume_instance(fit_frame.reshape(12), v, 4, 1.0)

    def recreate():
        old[0].close()
        old[0] = vpt.DeviceScene(old_host, 0)

    names = {"copy": copy, "remove": remove, "bake": bake}
    keys = ("update_wall", "update_device", "new_host_edit", "old_host_edit_and_flatten", "old_bake_call", "old_destroy_create", "old_way")
    t = {n: {k: [] for k in keys} for n in names}
    stats = {}
    for r in range(a.discard + a.repeat):
        for name in ("copy", "remove", "bake", "remove"):
            measured = r >= a.discard and not (name == "remove" and "bake" in stats.get("last", ""))
            edit, new_host_ms = timed(lambda: (names[name](new_host), new_host.update_volume_set())[1])
            _, wall = timed(lambda: A.update_volume_set(edit))
            launches, sent, device_ms = A.update_stats()
            baked, bake_ms = (None, 0.0)
            if name == "bake":
                (baked, _), bake_ms = timed(lambda: vpt.bake_sdf_grid(positions, triangles, whd, origin, step, device=0))
            _, host_ms = timed(lambda: (names[name](old_host, baked), old_host.update_volume_set(), old_host.desc)[2])
            _, create = timed(recreate)
            if measured:
                rec = t[name]
                rec["update_wall"].append(wall), rec["update_device"].append(device_ms), rec["new_host_edit"].append(new_host_ms)
                rec["old_host_edit_and_flatten"].append(host_ms), rec["old_bake_call"].append(bake_ms), rec["old_destroy_create"].append(create)
                rec["old_way"].append(host_ms + bake_ms + create)
                stats[name] = (launches, sent)
            stats["last"] = name
    vols = len(A.get_volumes()[0])
    same = all(np.array_equal(A.get_voxels(k).view(np.uint32), old[0].get_voxels(k).view(np.uint32)) for k in range(vols))
    same = bool(same and A.light_tables_hash() == old[0].light_tables_hash() and [v.offset for v in A.get_volumes()[0]] == [v.offset for v in old[0].get_volumes()[0]])
    records = []
    for name in names:
        rec = {"workload": name, "scene": "06_gridsdf_full", "update_launches": stats[name][0], "update_bytes": stats[name][1],
               "voxel_bytes_of_the_volume": 4 * (96 ** 3 if name != "bake" else 64 ** 3)}
        rec.update({k: stat(v) for k, v in t[name].items()})
        rec["ratio_old_over_update"] = float(np.median(t[name]["old_way"]) / np.median(t[name]["update_wall"]))
        rec["handles_equal_after_the_last_round"] = same
        print(json.dumps(rec), flush=True)
        records.append(rec)
    with open(os.path.join(a.out, "volume_set_measure.json"), "w") as f:
        json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
