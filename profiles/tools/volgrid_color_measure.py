"""Coloured extinction in the volgrid shader measured, on §29's two scenes and protocol (profiles/tools/volgrid_measure.py:
dense, sparse; 1280 x 533 x 64 spp, bounces 64, albedo 0.8, g 0.6, the brick walk): three cases alternating in every round after --discard
warm-up rounds, in ONE process - grey; coloured with equal channels, colour chosen so that kmax = 1 (the carrier is the grey medium but for
the rounding of exp and logf); coloured with a = (1, 0.5, 0.2) at kmax = 1.  Median, minimum and maximum of --repeat rounds of
vpt_last_kernel_ms, tracking steps and passes per sample.  Every timed launch follows an edit, so each includes its pilot launch: compare
the cases with each other, not with §29's steady-state figures.  (The committed record holds a fourth case, the alternative design with the
pass decided inside the tracking round, measured by this tool while the kernel had it: same bits, slower, removed - DESIGN.md §33.)  One JSON line per record, and the list in <out>/volgrid_color_measure.json.

  python profiles/tools/volgrid_color_measure.py [--out DIR (default profiles)] [--repeat 5] [--discard 2] [--resolution 1280] [--samples 64]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from volgrid_measure import F, GRIDSDF, ROOT, scene_with, stat  # noqa: E402
import vpt_loader  # noqa: E402

CASES = {"grey": None, "equal_channels": (1.0, 1.0, 1.0), "chromatic": (1.0, 0.5, 0.2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--resolution", type=int, default=1280)
    ap.add_argument("--samples", type=int, default=64)
    args = ap.parse_args()
    vpt = vpt_loader.load()
    os.environ["VPT_VOLGRID_NO_BRICKS"] = "0"
    records = []
    sdf, res = vpt.HostScene(GRIDSDF).volume(0)
    dense = vpt.density_from_sdf(sdf, 2.0 * res)
    sparse = np.zeros((128, 128, 128), F)
    sparse[48:80, 48:80, 48:80] = 1.0
    params = vpt.PathtraceParams(resolution=args.resolution, shader="volgrid", samples=args.samples, bounces=64)
    for name, voxels in (("dense", dense), ("sparse", sparse)):
        scene = scene_with(vpt, voxels, 0.05)
        dev = vpt.DeviceScene(scene, 0)
        ms, steps, passes = ({c: [] for c in CASES} for _ in range(3))
        for r in range(args.discard + args.repeat):
            for case, shares in CASES.items():
                if shares is not None:
                    m = scene.material(0)
                    m.color[:] = [float(np.exp(-a)) for a in shares]
                    scene.set_material(0, m)
                    dev.update(scene.update_bvh())
                dev.set_volgrid_color(shares is not None)
                st = scene.make_state(params)
                before = dev.volgrid_stats()["steps"], dev.volgrid_color_passes()
                dev.pathtrace_samples(st, params, args.samples)
                total = st.width * st.height * args.samples
                if r >= args.discard:
                    ms[case].append(dev.last_kernel_ms())
                    steps[case].append((dev.volgrid_stats()["steps"] - before[0]) / total)
                    passes[case].append((dev.volgrid_color_passes() - before[1]) / total)
        for case in CASES:
            rec = {"what": "render", "scene": name, "grid": list(voxels.shape), "case": case, "a": CASES[case], "width": st.width, "height": st.height,
                   "samples": args.samples, "bounces": 64, "kernel_ms": stat(ms[case]), "tracking_steps_per_sample": stat(steps[case]),
                   "passes_per_sample": stat(passes[case])}
            records.append(rec)
            print(json.dumps(rec), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "volgrid_color_measure.json"), "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
