"""vpt_scene_update_volumes measured against the only way there was to re-bake a grid of a resident scene or move an SDF before it
(DESIGN.md §17): vpt_bake_sdf (the voxels come back over PCIe), the new grid put into the host scene, vpt_scene_destroy and a whole
vpt_scene_create of 06_gridsdf_full.

Bake: tests/golden/scenes/03_volume/shapes/bunny.ply baked into the scene's second volume at 64^3 (its size: in place) and at 128^3
(a new size: the discarded round moves the volume to fresh room, the measured rounds write in place), on a grid fitted around the
mesh.  Per size, in ONE process, in interleaved rounds, median and minimum of --repeat rounds after --discard warm-up rounds:
 - update: the wall-clock time of the vpt_scene_update_volumes call with one bake entry (host clock; the call returns with the device
   idle) and its device time by events around the bake kernel (vpt_scene_update_stats), with its launches and bytes;
 - old way: vpt_bake_sdf (wall, and its kernel by events), HostScene.set_volume + update_volumes (the host's flatten of the edited
   scene), then destroy + create - each timed, and their sum.
The host preparation of a bake (feature normals, the tree, the records) is vpt_bake_sdf's on both sides; this change does not remove it.
The resident voxels after the last update are compared bit for bit with vpt_bake_sdf's.
SDF: the frame of the scene's emissive box moved and back: the update call against destroy + create.  Both ways take the edit from
the host mirror (set_sdf + update_volumes: the host's flatten), so that time is reported beside them and charged to neither;
ratio_with_host_mirror has it on both sides.
One JSON line per record, and the list in <out>/volume_update_measure.json.

  python profiles/tools/volume_update_measure.py [--out DIR (default .)] [--res 64,128] [--repeat 5] [--discard 1]"""
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
from bake_sdf_measure import load_shape, stat  # noqa: E402

SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "06_gridsdf_full", "gridsdf_full.json")
VOLUME, LAMP = 1, 1


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--res", default="64,128")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--discard", type=int, default=1)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    vpt = vpt_loader.load()
    if vpt.device_count() < 1:
        raise SystemExit("volume_update_measure needs a GPU: a time taken elsewhere says nothing")
    positions, triangles = load_shape(vpt, a.out)
    records = []

    def save(rec):
        print(json.dumps(rec), flush=True)
        records.append(rec)
        with open(os.path.join(a.out, "volume_update_measure.json"), "w") as f:
            json.dump(records, f, indent=1)

    for n in [int(r) for r in a.res.split(",")]:
        whd = (n, n, n)
        res, origin, step, _ = vpt.fit_volume(positions.min(axis=0), positions.max(axis=0), whd, 2)
        edit = vpt.VolumeEdit(volumes={VOLUME: vpt.VolumeSource(whd, res, (0, 0, 0), whd, vpt.VOXELS_REPLACE, None, (positions, triangles, origin, step))})
        host = vpt.HostScene(SCENE)
        A = vpt.DeviceScene(vpt.HostScene(SCENE), 0)
        old = vpt.DeviceScene(host, 0)
        t = {k: [] for k in ("update_wall", "update_device", "bake_wall", "bake_device", "host", "create", "old_way")}
        stats = baked = None
        for r in range(a.discard + a.repeat):
            _, wall = timed(lambda: A.update_volumes(edit))
            stats = A.update_stats()
            (baked, bstats), bake_wall = timed(lambda: vpt.bake_sdf_grid(positions, triangles, whd, origin, step, device=0))

            def mirror():
                host.set_volume(VOLUME, baked, res)
                host.update_volumes()
                return host.desc
            _, host_ms = timed(mirror)

            def recreate():
                old.close()
                return vpt.DeviceScene(host, 0)
            old, create = timed(recreate)
            if r >= a.discard:
                t["update_wall"].append(wall), t["update_device"].append(stats[2]), t["bake_wall"].append(bake_wall)
                t["bake_device"].append(bstats["device_ms"]), t["host"].append(host_ms), t["create"].append(create)
                t["old_way"].append(bake_wall + host_ms + create)
        same = bool(np.array_equal(A.get_voxels(VOLUME).view(np.uint32), baked.view(np.uint32)))
        rec = {"workload": "bake", "scene": "06_gridsdf_full", "shape": "bunny.ply", "triangles": int(len(triangles)), "res": n,
               "regrown_in_the_discarded_round": n != 64, "update_launches": stats[0], "update_bytes": stats[1], "voxel_bytes": 4 * n ** 3,
               "update_wall": stat(t["update_wall"]), "update_device": stat(t["update_device"]),
               "old_bake_call_wall": stat(t["bake_wall"]), "old_bake_device": stat(t["bake_device"]), "old_host_flatten": stat(t["host"]),
               "old_destroy_create": stat(t["create"]), "old_way_wall": stat(t["old_way"]),
               "ratio_old_over_update": float(np.median(t["old_way"]) / np.median(t["update_wall"])), "resident_equals_vpt_bake_sdf": same}
        save(rec)
        A.close(), old.close()

    # an SDF's frame moved and back
    host = vpt.HostScene(SCENE)
    A = vpt.DeviceScene(vpt.HostScene(SCENE), 0)
    old = vpt.DeviceScene(host, 0)
    t = {k: [] for k in ("update_wall", "host", "create")}
    stats = None
    for r in range(2 * (a.discard + a.repeat)):
        f = host.sdf(LAMP)
        f.frame.o[0] += 0.05 if r % 2 == 0 else -0.05
        _, host_ms = timed(lambda: (host.set_sdf(LAMP, f), host.update_volumes())[1])
        edit = vpt.VolumeEdit(sdfs={LAMP: host.sdf(LAMP)})
        _, wall = timed(lambda: A.update_volumes(edit))
        stats = A.update_stats()

        def recreate():
            old.close()
            return vpt.DeviceScene(host, 0)
        old, create = timed(recreate)
        if r >= 2 * a.discard:
            t["update_wall"].append(wall), t["host"].append(host_ms), t["create"].append(create)
    u, c, m = (float(np.median(t[k])) for k in ("update_wall", "create", "host"))
    save({"workload": "sdf_frame", "scene": "06_gridsdf_full", "update_launches": stats[0], "update_bytes": stats[1],
          "update_wall": stat(t["update_wall"]), "old_destroy_create": stat(t["create"]), "host_mirror_either_way": stat(t["host"]),
          "ratio_old_over_update": c / u, "ratio_with_host_mirror": (c + m) / (u + m),
          "same_light_tables": A.light_tables_hash() == old.light_tables_hash()})


if __name__ == "__main__":
    main()
