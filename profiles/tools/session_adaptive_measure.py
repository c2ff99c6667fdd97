"""Adaptive sampling inside a render session against the uniform session, on §10's three workloads.  A session is cut
into rounds whether it is adaptive or not: the uniform side advances `step` samples at a time to the cap, the adaptive side runs
rounds of `step` samples over the pixels still rendering until none is left.  For each workload, step (16, 32) and, on the adaptive
side, threshold (0.05, 0.1): the samples taken, the wall time from the first advance to the fetched last display frame, the device
time of the render launches (vpt_last_kernel_ms summed over the advances: for an adaptive advance every round with its update /
compaction kernels and read-back), and the RMS in sRGB [0, 1] against the high-spp uniform render §10 used.  Then the same with
denoise = 1, the RMS being that of the filtered image: the adaptive side hands the filter box3 of its Welford estimate, the uniform
side the half variance.  One JSON line per run, and the list in <out>/session_adaptive_measure.json.

  python profiles/tools/session_adaptive_measure.py [--out DIR (default .)] [--workloads headline,config4,frame5]"""
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
WORKLOADS = {   # name -> (scene, shader, bounces, resolution, cap, reference spp): those of profiles/tools/adaptive_measure.py
    "headline": (os.path.join(SCENES, "03_volume", "volume.json"), "volpathtrace", 64, 1280, 256, 2048),
    "config4": (os.path.join(SCENES, "06_gridsdf_full", "gridsdf_full.json"), "implicit", 4, 1280, 256, 1024),
    "frame5": (os.path.join(SCENES, "03_volume", "volume.json"), "volpathtrace", 64, 3840, 256, 1024),
}
STEPS = (16, 32)
THRESHOLDS = (0.05, 0.1)
MIN_SAMPLES = 16


def srgb(linear):
    x = np.clip(linear[..., :3].astype(np.float64), 0, None)
    return np.clip(np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1 / 2.4) - 0.055), 0, 1)


def run_session(vpt, dev, params, step, threshold, denoise):
    """one session to its last frame: threshold None is the uniform side"""
    s = vpt.RenderSession(dev, params, denoise=denoise, adaptive=None if threshold is None else (threshold, min(MIN_SAMPLES, params.samples), step))
    s.display()   # the reset has finished
    frames, device_ms = 0, 0.0
    t0 = time.perf_counter()
    while s.samples < params.samples and (threshold is None or not s.converged()):
        s.advance(step)
        device_ms += dev.last_kernel_ms()
        frames += 1
    s.display()
    wall = time.perf_counter() - t0
    w, h = s.size
    taken = s.progress()[1] if threshold is not None else w * h * s.samples
    image = s.image(denoised=denoise)
    s.close()
    return {"frames": frames, "samples": int(taken), "wall_s": round(wall, 4), "device_ms": round(device_ms, 2)}, image


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".", help="directory for session_adaptive_measure.json (default: the current one)")
    ap.add_argument("--workloads", default="headline,config4,frame5")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    vpt = vpt_loader.load()
    records = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        records.append(rec)

    for name, (path, shader, bounces, res, cap, ref_spp) in WORKLOADS.items():
        if name not in args.workloads.split(","):
            continue
        scene = vpt.HostScene(path)
        dev = vpt.DeviceScene(scene, 0)
        params = vpt.PathtraceParams(resolution=res, samples=cap, shader=shader, bounces=bounces)
        ref_params = vpt.PathtraceParams(resolution=res, samples=ref_spp, shader=shader, bounces=bounces)
        st = scene.make_state(ref_params)
        dev.pathtrace_samples(st, ref_params, ref_spp)
        ref = srgb(vpt.get_render(st))
        pixels = ref.shape[0] * ref.shape[1]
        rms = lambda img: float(np.sqrt(np.mean((srgb(img) - ref) ** 2)))
        warm = vpt.PathtraceParams(resolution=res, samples=32, shader=shader, bounces=bounces)
        run_session(vpt, dev, warm, 16, None, True)   # code objects, launch schedule, the filter's kernels
        run_session(vpt, dev, warm, 16, 0.05, True)
        for denoise in (False, True):
            for step in STEPS:
                base, image = run_session(vpt, dev, params, step, None, denoise)
                emit({"workload": name, "frame": f"{st.width}x{st.height}", "run": "uniform", "denoise": int(denoise), "step": step, **base,
                      "rms": rms(image)})
                for threshold in THRESHOLDS:
                    rec, image = run_session(vpt, dev, params, step, threshold, denoise)
                    emit({"workload": name, "run": "adaptive", "denoise": int(denoise), "step": step, "threshold": threshold, **rec,
                          "sample_share": round(rec["samples"] / (pixels * cap), 4), "wall_share": round(rec["wall_s"] / base["wall_s"], 4),
                          "device_share": round(rec["device_ms"] / base["device_ms"], 4), "rms": rms(image)})
        dev.close()
    with open(os.path.join(args.out, "session_adaptive_measure.json"), "w") as f:
        json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
