"""vpt_scene_fluid_step_detail measured in fluid_measure.py's protocol and on its scene: one step, closed walls, the default
multigrid solver, at --small^3 (96) and --large^3 (256), with the detail off (the step as it was), with the confinement alone, with
MacCormack alone and with both - and the confinement alone once more with VPT_FLUID_CONFINE_FUSED = 0: fluid_force_kernel and then the
confinement launch staging plain loads, in place of the one launch that applies the force as it stages.

In ONE process, the variants alternating in every round after --discard warm-up rounds, each starting from the same voxels (written back
untimed); median, minimum and maximum over --repeat rounds of the step's device time (events around the launches, vpt_scene_update_stats).
At --small the stepped voxels of every variant are compared with the host mirror's.  One JSON line per record, and the list in
<out>/fluid_detail_measure.json.

  python profiles/tools/fluid_detail_measure.py [--out DIR (default .)] [--repeat 5] [--discard 2] [--small 96] [--large 256]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fluid_measure import SCENE, F, start_fields, stat, vpt_loader  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--small", type=int, default=96)
    ap.add_argument("--large", type=int, default=256)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    vpt = vpt_loader.load()
    if vpt.device_count() < 1:
        raise SystemExit("fluid_detail_measure needs a GPU: a time taken elsewhere says nothing")
    records = []
    for n in sorted({a.small, a.large}):
        start, whd, res = start_fields(n), (n, n, n), 2.0 / n
        host = vpt.HostScene(SCENE)
        host.set_volume(0, start[0], res=res)
        host.update_volumes()
        ids = [0] + [host.add_volume(v, res=res) for v in start[1:]]
        host.update_volume_set()
        A = vpt.DeviceScene(host, 0)
        restore = vpt.VolumeEdit(volumes={i: vpt.VolumeSource(whd, res, (0, 0, 0), whd, vpt.VOXELS_REPLACE, v) for i, v in zip(ids, start)})
        step = vpt.FluidStep(ids[0], tuple(ids[1:]), steps=1, open_faces=0, dt=1.0, lift=(0.0, 0.5, 0.0), keep_density=0.995, keep_velocity=0.99)
        solver = vpt.FluidSolver()
        details = {"off": None, "confine": vpt.FluidDetail(vorticity=0.3), "maccormack": vpt.FluidDetail(vpt.FLUID_MACCORMACK),
                   "both": vpt.FluidDetail(vpt.FLUID_MACCORMACK, 0.3), "confine_unfused": vpt.FluidDetail(vorticity=0.3)}
        t, stats, ends = {v: [] for v in details}, {}, {}
        for r in range(a.discard + a.repeat):
            for v, detail in details.items():
                A.update_volumes(restore)
                os.environ["VPT_FLUID_CONFINE_FUSED"] = "0" if v.endswith("unfused") else ""
                A.fluid_step(step, solver, detail)
                stats[v] = A.update_stats()
                if r >= a.discard:
                    t[v].append(stats[v][2])
                if r == 0 and n == a.small:
                    ends[v] = [A.get_voxels(i).view(np.uint32) for i in ids]
        same = None
        if n == a.small:   # the mirror's step, for the comparison of bits
            same, err, shape, abi = True, C.create_string_buffer(256), np.array(whd, np.int32), step.to_abi()[0]
            for v, detail in details.items():
                g = [np.ascontiguousarray(x, F).copy() for x in start]
                args = [x.ctypes.data for x in g] + [shape.ctypes.data, C.byref(abi), C.byref(solver.to_abi()), C.byref(detail.to_abi()) if detail else None, err, 256]
                assert vpt.host.vpth_fluid_step_detail(*args) == 0, err.value
                same = same and all(np.array_equal(x.view(np.uint32), y) for x, y in zip(g, ends[v]))
        off = float(np.median(t["off"]))
        rec = {"grid": list(whd), "nodes": n ** 3,
               "variants": {v: {"launches": stats[v][0], "bytes": stats[v][1], "device": stat(t[v]), "over_off_ms": float(np.median(t[v]) - off)} for v in details},
               "device_equals_mirror_every_variant": same}
        print(json.dumps(rec), flush=True)
        records.append(rec)
        with open(os.path.join(a.out, "fluid_detail_measure.json"), "w") as out:
            json.dump(records, out, indent=1)
        A.close()


if __name__ == "__main__":
    main()
