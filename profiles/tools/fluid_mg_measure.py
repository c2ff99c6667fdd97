"""vpt_scene_fluid_step_solver measured in fluid_measure.py's protocol and on its scene: one step, closed walls, at --small^3
(96) and --large^3 (256), the pressure by the Jacobi at --iterations (40) sweeps (its default K) and by multigrid V(2,2) with 16 coarsest
sweeps at 1, 2 and 3 cycles, each at VPT_FLUID_MG_BLOCK = 2 and 4, and a step without a pressure solve (0 cycles).

In ONE process, the variants alternating in every round after --discard warm-up rounds, each starting from the same voxels (written back
untimed); median, minimum and maximum over --repeat rounds of the step's device time (events around the launches, vpt_scene_update_stats).

The residual each variant reaches: the pressure lives in the handle's scratch and no call reads it, so it is the host mirror's, which the
device equals bit for bit (tests/test_fluid_mg_gpu.py; here the stepped voxels of every variant are compared with the mirror's step at
--small) - stages 1 to 5 of the mirror give d, its stage 6 by either solver gives p, and the L2 norm of the mean-free part of
-d - (D p - S) is evaluated in float64, as a fraction of p = 0's.  One JSON line per record, and the list in <out>/fluid_mg_measure.json.

  python profiles/tools/fluid_mg_measure.py [--out DIR (default .)] [--repeat 5] [--discard 2] [--small 96] [--large 256] [--iterations 40]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fluid_measure import SCENE, F, start_fields, stat, vpt_loader  # noqa: E402


def residual(p, d):
    """the mean-free L2 norm of -d - (D p - S) behind closed walls, float64: D counts the neighbours inside, S sums them"""
    p, S, D = p.astype(np.float64), np.zeros(p.shape), np.zeros(p.shape)
    for axis in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        S[lo] += p[hi]
        S[hi] += p[lo]
        D[lo] += 1
        D[hi] += 1
    r = -d.astype(np.float64) - (D * p - S)
    return float(np.linalg.norm(r - r.mean()))


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
        raise SystemExit("fluid_mg_measure needs a GPU: a time taken elsewhere says nothing")
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
        step = vpt.FluidStep(ids[0], tuple(ids[1:]), steps=1, iterations=a.iterations, open_faces=0, dt=1.0, lift=(0.0, 0.5, 0.0), keep_density=0.995, keep_velocity=0.99)
        solvers = {"jacobi": None, "mg0": vpt.FluidSolver(cycles=0)}
        solvers.update({f"mg{c}_h{h}": vpt.FluidSolver(cycles=c, smooth=2, coarse_sweeps=16) for c in (1, 2, 3) for h in (2, 4)})
        t, stats, ends = {v: [] for v in solvers}, {}, {}
        for r in range(a.discard + a.repeat):
            for v, solver in solvers.items():
                A.update_volumes(restore)
                os.environ["VPT_FLUID_MG_BLOCK"] = v[-1] if "_h" in v else ""
                A.fluid_step(step, solver)
                stats[v] = A.update_stats()
                if r >= a.discard:
                    t[v].append(stats[v][2])
                if r == 0 and n == a.small:
                    ends[v] = [A.get_voxels(i).view(np.uint32) for i in ids]
        # the mirror: d from stages 1 to 5, p by either solver, and (at --small) the whole step for the comparison of bits
        err, shape, abi = C.create_string_buffer(256), np.array(whd, np.int32), step.to_abi()[0]
        f, d, p = [np.ascontiguousarray(v, F).copy() for v in start], np.zeros((n, n, n), F), np.zeros((n, n, n), F)
        for stage in (0, 1, 2, 1, 3, 4):
            assert vpt.host.vpth_fluid_stage(stage, *[v.ctypes.data for v in f], p.ctypes.data, d.ctypes.data, shape.ctypes.data, C.byref(abi), err, 256) == 0, err.value
        zero = residual(np.zeros_like(p), d)
        reached = {"jacobi": residual(p, d) / zero}
        for c in (1, 2, 3):
            assert vpt.host.vpth_fluid_multigrid_pressure(d.ctypes.data, p.ctypes.data, shape.ctypes.data, 0, C.byref(solvers[f"mg{c}_h2"].to_abi()), err, 256) == 0, err.value
            reached[f"mg{c}"] = residual(p, d) / zero
            print(f"{n}^3: residual after {c} cycles {reached[f'mg{c}']:.4g}, after {a.iterations} Jacobi sweeps {reached['jacobi']:.4g}", flush=True)
        same = None
        if n == a.small:
            same = True
            for v, solver in solvers.items():
                g = [np.ascontiguousarray(x, F).copy() for x in start]
                args = [x.ctypes.data for x in g] + [shape.ctypes.data, C.byref(abi), C.byref(solver.to_abi()) if solver else None, err, 256]
                assert vpt.host.vpth_fluid_step_solver(*args) == 0, err.value
                same = same and all(np.array_equal(x.view(np.uint32), y) for x, y in zip(g, ends[v]))
        rest = float(np.median(t["mg0"]))
        rec = {"grid": list(whd), "nodes": n ** 3, "iterations": a.iterations, "residual_of_p0": zero,
               "variants": {v: {"launches": stats[v][0], "device": stat(t[v]), "pressure_ms": float(np.median(t[v]) - rest),
                                "residual_fraction": reached.get(v.split("_")[0])} for v in solvers},
               "device_equals_mirror_every_variant": same}
        print(json.dumps(rec), flush=True)
        records.append(rec)
        with open(os.path.join(a.out, "fluid_mg_measure.json"), "w") as out:
            json.dump(records, out, indent=1)
        A.close()


if __name__ == "__main__":
    main()
