"""Adaptive sampling against uniform sampling: for each workload, a high-spp uniform reference, a uniform render at
the cap, adaptive renders at a few thresholds and round sizes, and uniform renders with the same number of samples as each adaptive
one.  Times are device events (vpt_last_kernel_ms: the launches of a vpt_render call; for an adaptive call, every round with its
update / compaction kernels and the per-round read-back); RMS is against the reference in sRGB [0, 1].  One JSON line per run,
and the list in <out>/adaptive_measure.json.

  python profiles/tools/adaptive_measure.py [--out DIR (default .)] [--quick] [--workloads headline,config4,frame5]
--quick: the headline frame at one threshold only (the workload of the rocprofv3 --kernel-trace --stats run)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import vpt_loader  # noqa: E402

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
WORKLOADS = {   # name -> (scene, shader, bounces, resolution, cap, reference spp, (threshold, step) of the adaptive runs)
    "headline": (os.path.join(SCENES, "03_volume", "volume.json"), "volpathtrace", 64, 1280, 256, 2048,
                 ((0.1, 16), (0.05, 16), (0.03, 16), (0.02, 16), (0.05, 8), (0.05, 32), (0.05, 64))),
    "config4": (os.path.join(SCENES, "06_gridsdf_full", "gridsdf_full.json"), "implicit", 4, 1280, 256, 1024,
                ((0.1, 16), (0.05, 16), (0.03, 16), (0.02, 16), (0.05, 8), (0.05, 32), (0.05, 64))),
    # BASELINE config 5's frame: 9x the tiles of the headline frame, a launch bound by work rather than by its costliest wave
    "frame5": (os.path.join(SCENES, "03_volume", "volume.json"), "volpathtrace", 64, 3840, 256, 1024, ((0.1, 32), (0.05, 32), (0.05, 16), (0.03, 32))),
}


def srgb(linear):
    x = np.clip(linear[..., :3].astype(np.float64), 0, None)
    return np.clip(np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1 / 2.4) - 0.055), 0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".", help="directory for adaptive_measure.json (default: the current one)")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--workloads", default="headline,config4")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    vpt = vpt_loader.load()
    records = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        records.append(rec)

    for name, (path, shader, bounces, res, cap, ref_spp, runs) in WORKLOADS.items():
        if (args.quick and name != "headline") or (not args.quick and name not in args.workloads.split(",")):
            continue
        scene = vpt.HostScene(path)
        dev = vpt.DeviceScene(scene, 0)
        params = vpt.PathtraceParams(resolution=res, samples=cap, shader=shader, bounces=bounces)

        def uniform(spp, p=params):
            st = scene.make_state(p)
            t0 = time.perf_counter()
            dev.pathtrace_samples(st, p, spp)
            return st, dev.last_kernel_ms(), time.perf_counter() - t0

        def adaptive(threshold, step, min_samples=16):
            st = scene.make_state(params)
            t0 = time.perf_counter()
            rounds, taken = dev.pathtrace_adaptive(st, params, threshold, min(min_samples, cap), step)
            return st, rounds, taken, dev.last_kernel_ms(), time.perf_counter() - t0

        uniform(16)   # code objects, launch schedule
        adaptive(0.05, 16)
        if args.quick:
            st, rounds, taken, ms, wall = adaptive(0.05, 16)
            emit({"workload": name, "run": "adaptive", "threshold": 0.05, "step": 16, "rounds": rounds, "samples": taken, "ms": round(ms, 2)})
            continue
        ref_params = vpt.PathtraceParams(resolution=res, samples=ref_spp, shader=shader, bounces=bounces)
        ref = srgb(vpt.get_render(uniform(ref_spp, ref_params)[0]))
        pixels = ref.shape[0] * ref.shape[1]
        rms = lambda img: float(np.sqrt(np.mean((srgb(img) - ref) ** 2)))
        st, ms, wall = uniform(cap)
        full_ms = ms
        emit({"workload": name, "run": "uniform", "spp": cap, "samples": pixels * cap, "ms": round(ms, 2), "wall_s": round(wall, 3),
              "rms": rms(vpt.get_render(st)), "frame": f"{st.width}x{st.height}"})
        for threshold, step in runs:
            st, rounds, taken, ms, wall = adaptive(threshold, step)
            spp = max(1, taken // pixels)
            us, ums, uwall = uniform(spp)
            emit({"workload": name, "run": "adaptive", "threshold": threshold, "step": step, "rounds": rounds, "samples": taken,
                  "sample_share": round(taken / (pixels * cap), 4), "ms": round(ms, 2), "ms_per_round": round(ms / max(rounds, 1), 2),
                  "time_share": round(ms / full_ms, 4), "wall_s": round(wall, 3), "rms": rms(vpt.get_render_hits(st)),
                  "uniform_same_samples": {"spp": spp, "ms": round(ums, 2), "rms": rms(vpt.get_render(us))}})
        dev.close()
    with open(os.path.join(args.out, "adaptive_measure.json"), "w") as f:
        json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
