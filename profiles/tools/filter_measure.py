"""vpt_scene_filter_volumes measured against the way the same voxels were reached before it, on 06_gridsdf_full's 96^3
grid (volume 0) and on a 256^3 bake of 03_volume's bunny put into volume 0 of a second handle.

Workloads, each over the whole grid: to_density; a blur at R = 1, 2 and 4; a four-octave noise.  Per workload, in ONE process, both sides
alternating in every round after --discard warm-up rounds, each round starting from the same voxels (written back untimed); median,
minimum and maximum of --repeat rounds:
 - resident: the wall-clock time of DeviceScene.filter_volumes (host clock; the call returns with the device idle), its device time by
   events around the launches (vpt_scene_update_stats), its launches and bytes, and the region's read-plus-write bytes (8 per voxel
   and op) over the device time;
 - old way: vpt_scene_get_voxels (the whole volume comes back over PCIe), the op on the host - density_from_sdf in numpy for to_density, the
   host mirror (vpth_filter_voxels) for the others - and vpt_scene_update_volumes with the whole grid in REPLACE mode: each timed, and their sum.
After the last round the resident voxels of both ways are compared bit for bit (to_density: as numbers).  One JSON line per record, and
the list in <out>/filter_measure.json.

  python profiles/tools/filter_measure.py [--out DIR (default .)] [--repeat 7] [--discard 2] [--bake 256]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vpt_loader  # noqa: E402
from bake_sdf_measure import load_shape  # noqa: E402

SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "06_gridsdf_full", "gridsdf_full.json")
F = np.float32


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "max_ms": float(np.max(xs)), "n": len(xs)}


def mirror(vpt, grid, entry):
    """the host mirror of `entry` on a copy of the (d, h, w) grid"""
    out = grid.copy()
    whd = np.array(out.shape[::-1], np.int32)
    abi, keep = vpt.FilterEdit([entry]).to_abi()
    err = C.create_string_buffer(256)
    if vpt.host.vpth_filter_voxels(out.ctypes.data, whd.ctypes.data, C.cast(abi.entries, C.POINTER(vpt.VptFilterEntry)), abi.ops, abi.num_ops, err, len(err)) != 0:
        raise SystemExit(err.value.decode())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--bake", type=int, default=256)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    vpt = vpt_loader.load()
    if vpt.device_count() < 1:
        raise SystemExit("filter_measure needs a GPU: a time taken elsewhere says nothing")
    records = []

    def save(rec):
        print(json.dumps(rec), flush=True)
        records.append(rec)
        with open(os.path.join(a.out, "filter_measure.json"), "w") as f:
            json.dump(records, f, indent=1)

    small, res_small = vpt.HostScene(SCENE).volume(0)
    positions, triangles = load_shape(vpt, a.out)
    baked = vpt.bake_sdf(positions, triangles, a.bake, device=0)
    subjects = [("sackboy_96", np.ascontiguousarray(small, F), res_small), (f"bunny_bake_{a.bake}", np.ascontiguousarray(baked.voxels, F), baked.res)]
    for subject, start, res in subjects:
        whd = start.shape[::-1]
        step = tuple(float(F(res) * F(w) / F(w - 1)) for w in whd)
        width = 2 * step[0]
        workloads = [("to_density", [vpt.FilterOp.to_density(width)])] + [(f"blur_r{r}", [vpt.FilterOp.blur(0.6 * r, r)]) for r in (1, 2, 4)] + \
                    [("noise_4_octaves", [vpt.FilterOp.noise(0.5, 24.0 / (step[0] * whd[0]), 0.5, 4, seed=1)])]
        pairs = []
        for _ in range(2):   # the resident way's handle and the old way's, each holding `start` in volume 0
            h = vpt.HostScene(SCENE)
            h.set_volume(0, start, res=res)
            d = vpt.DeviceScene(vpt.HostScene(SCENE), 0)
            d.update_volumes(h.update_volumes())
            pairs.append(d)
        A, B = pairs
        restore = vpt.VolumeEdit(volumes={0: vpt.VolumeSource(whd, res, (0, 0, 0), whd, vpt.VOXELS_REPLACE, start)})
        for name, ops in workloads:
            entry = vpt.FilterEntry(0, (0, 0, 0), whd, (0.0, 0.0, 0.0), step, ops)
            edit = vpt.FilterEdit([entry])
            t = {k: [] for k in ("wall", "device", "get", "host", "update", "old")}
            stats = None
            for r in range(a.discard + a.repeat):
                A.update_volumes(restore), B.update_volumes(restore)
                _, wall = timed(lambda: A.filter_volumes(edit))
                stats = A.update_stats()
                resident, get_ms = timed(lambda: B.get_voxels(0))
                box, host_ms = timed((lambda: vpt.density_from_sdf(resident, width)) if name == "to_density" else (lambda: mirror(vpt, resident, entry)))
                old_edit = vpt.VolumeEdit(volumes={0: vpt.VolumeSource(whd, res, (0, 0, 0), whd, vpt.VOXELS_REPLACE, box)})
                _, upd_ms = timed(lambda: B.update_volumes(old_edit))
                if r >= a.discard:
                    t["wall"].append(wall), t["device"].append(stats[2]), t["get"].append(get_ms), t["host"].append(host_ms), t["update"].append(upd_ms)
                    t["old"].append(get_ms + host_ms + upd_ms)
            got, old = A.get_voxels(0), B.get_voxels(0)
            same = bool(np.array_equal(got, old) if name == "to_density" else np.array_equal(got.view(np.uint32), old.view(np.uint32)))
            voxels = int(np.prod(whd))
            save({"subject": subject, "workload": name, "grid": list(whd), "voxels": voxels, "launches": stats[0], "bytes_sent": stats[1],
                  "resident_wall": stat(t["wall"]), "resident_device": stat(t["device"]),
                  "read_plus_write_GBps_of_device_time": float(8 * voxels / (np.median(t["device"]) * 1e-3) / 1e9),
                  "old_get_voxels": stat(t["get"]), "old_host_op": stat(t["host"]), "old_update_volumes": stat(t["update"]), "old_way_wall": stat(t["old"]),
                  "old_bytes_down": 4 * voxels, "old_bytes_up": 4 * voxels,
                  "ratio_old_over_resident": float(np.median(t["old"]) / np.median(t["wall"])),
                  "ratio_transfers_alone": float((np.median(t["get"]) + np.median(t["update"])) / np.median(t["wall"])),
                  "resident_equal_both_ways": same})
        A.close(), B.close()


if __name__ == "__main__":
    main()
