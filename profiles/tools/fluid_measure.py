"""vpt_scene_fluid_step measured: the sweeps a Jacobi launch blocks (VPT_FLUID_BLOCK = 1, 2, 4) against each other, the
pressure's share of a step, and the resident call against the way the same voxels were reached before it.  Two grids, --small^3 (96) and --large^3
(256): a smooth density blob in volume 0 of 06_gridsdf_full's scene and three random velocity volumes added behind it; one step at
--iterations (40) Jacobi sweeps, closed walls.

In ONE process, the variants alternating in every round after --discard warm-up rounds, each variant of each round starting from the same
voxels (written back untimed); median, minimum and maximum of --repeat rounds:
 - resident, K = 1, 2, 4: the wall-clock time of DeviceScene.fluid_step (host clock; the call returns with the device idle), its device
   time by events around the launches (vpt_scene_update_stats), its launches and bytes;
 - resident at 0 sweeps (K plays no part): force, advect, place, divergence and project alone - a step's device time less this is the
   pressure's;
 - old way: four vpt_scene_get_voxels, the host mirror (vpth_fluid_step: a plain SERIAL loop, a statement of the rule and no fast CPU
   solver) and vpt_scene_update_volumes with the four grids in REPLACE mode: each timed, and their sum.
After the last round the resident voxels of all ways are compared bit for bit.  One JSON line per record, and the list in
<out>/fluid_measure.json.

  python profiles/tools/fluid_measure.py [--out DIR (default .)] [--repeat 5] [--discard 2] [--small 96] [--large 256] [--iterations 40]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import vpt_loader  # noqa: E402

SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "06_gridsdf_full", "gridsdf_full.json")
F = np.float32


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "max_ms": float(np.max(xs)), "n": len(xs)}


def start_fields(n):
    """a density blob low in the box and a random velocity of about a node per unit time"""
    g = np.random.default_rng(n)
    z, y, x = np.meshgrid(*(np.linspace(-1, 1, n, dtype=F),) * 3, indexing="ij")
    rho = np.clip(1.5 - 4 * np.sqrt(x * x + (y + 0.5) ** 2 + z * z), 0, 1).astype(F)
    return [rho] + [g.normal(0, 0.7, (n, n, n)).astype(F) for _ in range(3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--small", type=int, default=96)
    ap.add_argument("--large", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=40)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    vpt = vpt_loader.load()
    if vpt.device_count() < 1:
        raise SystemExit("fluid_measure needs a GPU: a time taken elsewhere says nothing")
    records = []

    def save(rec):
        print(json.dumps(rec), flush=True)
        records.append(rec)
        with open(os.path.join(a.out, "fluid_measure.json"), "w") as f:
            json.dump(records, f, indent=1)

    for n in sorted({a.small, a.large}):
        start, whd, res = start_fields(n), (n, n, n), 2.0 / n
        host = vpt.HostScene(SCENE)
        host.set_volume(0, start[0], res=res)
        host.update_volumes()
        ids = [0] + [host.add_volume(v, res=res) for v in start[1:]]
        host.update_volume_set()
        A, B = vpt.DeviceScene(host, 0), vpt.DeviceScene(host, 0)   # the resident way's handle and the old way's
        restore = vpt.VolumeEdit(volumes={i: vpt.VolumeSource(whd, res, (0, 0, 0), whd, vpt.VOXELS_REPLACE, v) for i, v in zip(ids, start)})
        step = vpt.FluidStep(ids[0], tuple(ids[1:]), steps=1, iterations=a.iterations, open_faces=0, dt=1.0, lift=(0.0, 0.5, 0.0), keep_density=0.995, keep_velocity=0.99)
        idle = vpt.FluidStep(ids[0], tuple(ids[1:]), steps=1, iterations=0, open_faces=0, dt=1.0, lift=(0.0, 0.5, 0.0), keep_density=0.995, keep_velocity=0.99)
        abi, shape = step.to_abi()[0], np.array(whd, np.int32)
        variants = ["1", "2", "4"]
        t = {k: [] for k in [f"wall_{v}" for v in variants] + [f"device_{v}" for v in variants] + ["wall_0", "device_0", "get", "host", "update", "old"]}
        stats, ends = {}, {}
        for r in range(a.discard + a.repeat):
            keep = r >= a.discard
            for v in variants + ["0"]:
                A.update_volumes(restore)
                if v != "0":
                    os.environ["VPT_FLUID_BLOCK"] = v
                _, wall = timed(lambda: A.fluid_step(idle if v == "0" else step))
                stats[v] = A.update_stats()
                if keep:
                    t[f"wall_{v}"].append(wall), t[f"device_{v}"].append(stats[v][2])
                if r == a.discard + a.repeat - 1 and v != "0":
                    ends[v] = [A.get_voxels(i) for i in ids]
            B.update_volumes(restore)
            grids, get_ms = timed(lambda: [np.ascontiguousarray(B.get_voxels(i), F) for i in ids])
            err = C.create_string_buffer(256)
            rc, host_ms = timed(lambda: vpt.host.vpth_fluid_step(*[g.ctypes.data for g in grids], shape.ctypes.data, C.byref(abi), err, len(err)))
            if rc != 0:
                raise SystemExit(err.value.decode())
            old_edit = vpt.VolumeEdit(volumes={i: vpt.VolumeSource(whd, res, (0, 0, 0), whd, vpt.VOXELS_REPLACE, g) for i, g in zip(ids, grids)})
            _, upd_ms = timed(lambda: B.update_volumes(old_edit))
            if keep:
                t["get"].append(get_ms), t["host"].append(host_ms), t["update"].append(upd_ms), t["old"].append(get_ms + host_ms + upd_ms)
        ends["old"] = [B.get_voxels(i) for i in ids]
        same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for e in ends.values() for x, y in zip(e, ends["1"]))
        rest = float(np.median(t["device_0"]))
        save({"grid": list(whd), "nodes": n ** 3, "iterations": a.iterations, "bytes_sent": stats["1"][1],
              "resident": {v: {"launches": stats[v][0], "wall": stat(t[f"wall_{v}"]), "device": stat(t[f"device_{v}"]),
                               "pressure_share_of_device_time": float(1 - rest / np.median(t[f"device_{v}"]))} for v in variants},
              "resident_without_sweeps": {"launches": stats["0"][0], "wall": stat(t["wall_0"]), "device": stat(t["device_0"])},
              "old_get_voxels_x4": stat(t["get"]), "old_host_mirror_serial": stat(t["host"]), "old_update_volumes": stat(t["update"]), "old_way_wall": stat(t["old"]),
              "old_bytes_down": 16 * n ** 3, "old_bytes_up": 16 * n ** 3,
              "ratio_old_over_resident_k1": float(np.median(t["old"]) / np.median(t["wall_1"])),
              "ratio_transfers_alone_k1": float((np.median(t["get"]) + np.median(t["update"])) / np.median(t["wall_1"])),
              "resident_equal_all_ways": bool(same)})
        A.close(), B.close()


if __name__ == "__main__":
    main()
