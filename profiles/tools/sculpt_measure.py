"""vpt_scene_sculpt_volumes measured against the way the same voxels were reached before it, on 06_gridsdf_full's 96^3
grid (volume 0; voxel space: origin 0, step res * 96 / 95).

Workloads: a one-stamp dent (a sphere of radius 6 voxels, the region its box of 15^3 voxels) as SUBTRACT and as UNION, and a stroke of 64
such spheres along a line through the figure (the region the stroke's box) as SUBTRACT.  Per workload, in ONE process, both sides
alternating in every round after --discard warm-up rounds; median, minimum and maximum of --repeat rounds:
 - sculpt: the wall-clock time of DeviceScene.sculpt_volumes with the edit (host clock; the call returns with the device idle), its
   device time by events around the launches (vpt_scene_update_stats), its launches and bytes;
 - old way, SUBTRACT: vpt_scene_get_voxels (the whole volume comes back over PCIe), the host mirror of the rule over the region, and
   vpt_scene_update_volumes with the box in REPLACE mode - each timed, and their sum;
 - old way, UNION: the host mirror evaluates the brush over the region (a REPLACE into a scratch scene), then vpt_scene_update_volumes
   with that box in UNION mode;
 - the stroke also as 64 one-stamp entries in one call (64 launches) and as 64 calls, against its one launch.
Both ways keep a host copy current in an editor (HostScene.sculpt_volume): on the old way that work IS the evaluation and is on its path;
for sculpt it is reported beside the call (host_mirror_beside) and charged to neither.  HostScene.update_sculpts (the host's flatten of the
edited scene, which a fresh DeviceScene would read) is the same on both ways, timed (host_flatten_either_way) and charged to neither.  After the last round the resident voxels of both
ways are compared bit for bit.  One JSON line per record, and the list in <out>/sculpt_measure.json.

  python profiles/tools/sculpt_measure.py [--out DIR (default .)] [--repeat 7] [--discard 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import vpt_loader  # noqa: E402

SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "06_gridsdf_full", "gridsdf_full.json")
VOLUME, N = 0, 96
F = np.float32


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "max_ms": float(np.max(xs)), "n": len(xs)}


def sphere(vpt, centre, radius):
    f = vpt.VptSdf(type=vpt.SDF_TYPES.index("sphere"))
    f.frame.x[:], f.frame.y[:], f.frame.z[:], f.frame.o[:] = (1, 0, 0), (0, 1, 0), (0, 0, 1), [-float(c) for c in centre]
    f.p[0] = float(radius)
    return f


def box_around(centres, reach):
    """(lo, size) of the voxels within `reach` voxels of the centres (in voxels), one voxel to spare, clipped to the grid"""
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    lo = np.clip(np.floor(c.min(axis=0) - reach).astype(int) - 1, 0, N)
    hi = np.clip(np.ceil(c.max(axis=0) + reach).astype(int) + 2, 0, N)
    return tuple(int(v) for v in lo), tuple(int(v) for v in hi - lo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--discard", type=int, default=2)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    vpt = vpt_loader.load()
    if vpt.device_count() < 1:
        raise SystemExit("sculpt_measure needs a GPU: a time taken elsewhere says nothing")
    records = []

    def save(rec):
        print(json.dumps(rec), flush=True)
        records.append(rec)
        with open(os.path.join(a.out, "sculpt_measure.json"), "w") as f:
            json.dump(records, f, indent=1)

    res = vpt.HostScene(SCENE).volume(VOLUME)[1]
    step = float(F(res) * F(N) / F(N - 1))
    radius = 6.0
    dent = [(48.0, 45.0, 60.0)]
    line = [(30.0 + 36.0 * t, 30.0 + 30.0 * t, 62.0 - 20.0 * t) for t in (np.arange(64) + 0.5) / 64]
    workloads = [("dent_subtract", dent, vpt.SCULPT_SUBTRACT), ("dent_union", dent, vpt.SCULPT_UNION), ("stroke64_subtract", line, vpt.SCULPT_SUBTRACT)]
    for name, centres, op in workloads:
        region = box_around(centres, radius)
        stamps = [vpt.Stamp(sphere(vpt, [c * step for c in centre], radius * step), op) for centre in centres]
        new_host, old_host, scratch = vpt.HostScene(SCENE), vpt.HostScene(SCENE), vpt.HostScene(SCENE)
        A, B = vpt.DeviceScene(vpt.HostScene(SCENE), 0), vpt.DeviceScene(vpt.HostScene(SCENE), 0)
        keys = ("sculpt_wall", "sculpt_device", "mirror_beside", "old_get_voxels", "old_host", "old_update", "old_way", "entries_wall", "entries_device",
                "calls_wall", "flatten")
        t = {k: [] for k in keys}
        stats = None
        whd = (N, N, N)
        lo, size = region
        cut = (slice(lo[2], lo[2] + size[2]), slice(lo[1], lo[1] + size[1]), slice(lo[0], lo[0] + size[0]))
        for r in range(a.discard + a.repeat):
            # this change: the host copy beside it, then the call
            entry, mirror_ms = timed(lambda: new_host.sculpt_volume(VOLUME, stamps, region=region))
            edit, flatten_ms = timed(new_host.update_sculpts)
            _, wall = timed(lambda: A.sculpt_volumes(edit))
            stats = A.update_stats()
            # the old way to the same voxels
            if op == vpt.SCULPT_SUBTRACT:
                resident, get_ms = timed(lambda: B.get_voxels(VOLUME))

                def on_host():
                    old_host.sculpt_volume(VOLUME, stamps, region=region)
                    return np.ascontiguousarray(old_host.volume(VOLUME)[0][cut])
                box, host_ms = timed(on_host)
                old_host.update_sculpts()
                mode = vpt.VOXELS_REPLACE
            else:
                get_ms = 0.0

                def on_host():
                    scratch.sculpt_volume(VOLUME, [vpt.Stamp(s.brush, vpt.SCULPT_REPLACE) for s in stamps], region=region)
                    return np.ascontiguousarray(scratch.volume(VOLUME)[0][cut])
                box, host_ms = timed(on_host)
                scratch.update_sculpts()
                mode = vpt.VOXELS_UNION
            old_edit = vpt.VolumeEdit(volumes={VOLUME: vpt.VolumeSource(whd, res, lo, size, mode, box)})
            _, upd_ms = timed(lambda: B.update_volumes(old_edit))
            if r >= a.discard:
                t["sculpt_wall"].append(wall), t["sculpt_device"].append(stats[2]), t["mirror_beside"].append(mirror_ms), t["flatten"].append(flatten_ms)
                t["old_get_voxels"].append(get_ms), t["old_host"].append(host_ms), t["old_update"].append(upd_ms), t["old_way"].append(get_ms + host_ms + upd_ms)
            if len(stamps) > 1:   # the stroke as 64 launches: one call of 64 one-stamp entries, and 64 calls
                singles = vpt.SculptEdit([vpt.SculptEntry(VOLUME, entry.region_lo, entry.region_whd, entry.origin, entry.step, [s]) for s in stamps])
                _, e_wall = timed(lambda: A.sculpt_volumes(singles))
                e_stats = A.update_stats()
                parts = [vpt.SculptEdit([e]) for e in singles.entries]
                _, c_wall = timed(lambda: [A.sculpt_volumes(p) for p in parts])
                if r >= a.discard:
                    t["entries_wall"].append(e_wall), t["entries_device"].append(e_stats[2]), t["calls_wall"].append(c_wall)
        # (a stroke applied again is idempotent for SUBTRACT and UNION without blend: max and min; so A, which ran it three times per
        # round, B and the two host copies hold the same voxels)
        same = bool(np.array_equal(A.get_voxels(VOLUME).view(np.uint32), B.get_voxels(VOLUME).view(np.uint32)))
        same_host = bool(np.array_equal(A.get_voxels(VOLUME).view(np.uint32), new_host.volume(VOLUME)[0].view(np.uint32)))
        rec = {"workload": name, "scene": "06_gridsdf_full", "grid": N, "stamps": len(stamps), "region": [list(lo), list(size)],
               "region_voxels": int(np.prod(size)), "sculpt_launches": stats[0], "sculpt_bytes": stats[1],
               "old_bytes_down": 4 * N ** 3 if op == vpt.SCULPT_SUBTRACT else 0, "old_bytes_up": 4 * int(np.prod(size)),
               "sculpt_wall": stat(t["sculpt_wall"]), "sculpt_device": stat(t["sculpt_device"]), "host_mirror_beside": stat(t["mirror_beside"]),
               "host_flatten_either_way": stat(t["flatten"]),
               "old_get_voxels": stat(t["old_get_voxels"]), "old_host_mirror": stat(t["old_host"]), "old_update_volumes": stat(t["old_update"]),
               "old_way_wall": stat(t["old_way"]), "ratio_old_over_sculpt": float(np.median(t["old_way"]) / np.median(t["sculpt_wall"])),
               "ratio_transfers_alone": float((np.median(t["old_get_voxels"]) + np.median(t["old_update"])) / np.median(t["sculpt_wall"])),
               "resident_equal_both_ways": same, "resident_equals_host_mirror": same_host}
        if len(stamps) > 1:
            rec.update({"one_call_64_entries_wall": stat(t["entries_wall"]), "one_call_64_entries_device": stat(t["entries_device"]),
                        "sixty_four_calls_wall": stat(t["calls_wall"]),
                        "ratio_64_launches_over_one_device": float(np.median(t["entries_device"]) / np.median(t["sculpt_device"])),
                        "ratio_64_calls_over_one_wall": float(np.median(t["calls_wall"]) / np.median(t["sculpt_wall"]))})
        save(rec)
        A.close(), B.close()


if __name__ == "__main__":
    main()
