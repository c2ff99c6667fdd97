"""The denoising filter measured.

--quality: for each workload a high-spp reference (the one §10 used), uniform renders at 16 / 64 / 256 spp, each filtered with the
  spatial seed and with the half variance of its own sample chain; RMS against the reference in sRGB [0, 1]; the render's, the guides'
  and the filter's time (vpt_last_kernel_ms for the launches of a render; device events around vpt_denoise_device; for the guides also
  the wall clock of pathtrace_guides, which moves the state through the host).
--speed: device-event time of vpt_denoise_device (warm calls, median of --repeat) at the three BASELINE frame sizes, for the tiled and
  the plain form (VPT_DENOISE_PLAIN, read per call) taken in turns, by iteration count (pass k has stride 2^k, so the differences are the
  passes' own times), beside the bound it is read against: 72 B per pixel and pass over the HBM figure bench.py uses.
One JSON line per record, and the list in <out>/denoise_measure_<mode>.json.

  python profiles/tools/denoise_measure.py --speed | --quality [--out DIR (default .)] [--workloads headline,config4,frame5] [--repeat 20]"""
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
WORKLOADS = {   # name -> (scene, shader, bounces, resolution, reference spp): the workloads and references of adaptive_measure.py
    "headline": (os.path.join(SCENES, "03_volume", "volume.json"), "volpathtrace", 64, 1280, 2048),
    "config4": (os.path.join(SCENES, "06_gridsdf_full", "gridsdf_full.json"), "implicit", 4, 1280, 1024),
    "frame5": (os.path.join(SCENES, "03_volume", "volume.json"), "volpathtrace", 64, 3840, 1024),
}
SIZES = ((1280, 533), (1280, 1280), (3840, 1600))
HBM_BYTES_PER_S = 8.0e12   # bench.py's roofline figure
GUIDE_SPP = 16


def srgb(linear):
    x = np.clip(linear[..., :3].astype(np.float64), 0, 1)
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1 / 2.4) - 0.055)


class DeviceFilter:
    """vpt_denoise_device on torch buffers, timed with device events"""

    def __init__(self, vpt, color, albedo, normal, variance):
        import torch
        self.torch, self.vpt = torch, vpt
        self.h, self.w, _ = color.shape
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
        self.bufs = [up(color), up(normal), up(albedo), up(variance)]
        self.out = torch.zeros((self.h, self.w, 4), dtype=torch.float32, device="cuda")
        self.scratch = torch.zeros(vpt.denoise_scratch_bytes(self.w, self.h), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def run(self, use_variance=True, **kw):
        """one call on the current stream; returns its device time in ms"""
        torch = self.torch
        ptr = [None if t is None else t.data_ptr() for t in self.bufs]
        if not use_variance:
            ptr[3] = None
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream = torch.cuda.current_stream()
        t0.record(stream)
        self.vpt.denoise_device(self.w, self.h, ptr[0], ptr[1], ptr[2], ptr[3], self.out.data_ptr(), self.scratch.data_ptr(),
                                stream=stream.cuda_stream, **kw)
        t1.record(stream)
        t1.synchronize()
        return t0.elapsed_time(t1)

    def result(self):
        return self.out.cpu().numpy()


def speed(vpt, emit, repeat):
    rng = np.random.default_rng(0)
    for w, h in SIZES:
        color = rng.gamma(2.0, 0.3, (h, w, 4)).astype(np.float32)
        albedo = (np.round(rng.random((h, w, 4)) * 8) / 8).astype(np.float32)
        normal = rng.random((h, w, 4)).astype(np.float32)
        variance = (rng.random((h, w)) * 0.05).astype(np.float32)
        bound_ms = 72.0 * w * h / HBM_BYTES_PER_S * 1e3
        for guides in ("both", "none"):
            f = DeviceFilter(vpt, color, albedo if guides == "both" else None, normal if guides == "both" else None, variance)
            for iterations in (1, 2, 3, 5):
                times = {"tiled": [], "plain": []}
                for i in range(repeat + 3):   # the forms in turns, three warm calls of each first
                    for form in ("tiled", "plain"):
                        os.environ["VPT_DENOISE_PLAIN"] = "1" if form == "plain" else "0"
                        ms = f.run(iterations=iterations)
                        if i >= 3:
                            times[form].append(ms)
                os.environ["VPT_DENOISE_PLAIN"] = "0"
                seed_ms = float(np.median([f.run(use_variance=False, iterations=iterations) for _ in range(repeat + 3)][3:]))
                emit({"mode": "speed", "frame": f"{w}x{h}", "guides": guides, "iterations": iterations,
                      "tiled_ms": round(float(np.median(times["tiled"])), 4), "plain_ms": round(float(np.median(times["plain"])), 4),
                      "tiled_min_ms": round(min(times["tiled"]), 4), "plain_min_ms": round(min(times["plain"]), 4),
                      "tiled_with_spatial_seed_ms": round(seed_ms, 4), "hbm_bound_ms": round(bound_ms * iterations, 4)})
    os.environ.pop("VPT_DENOISE_PLAIN", None)


def quality(vpt, emit, names):
    for name in names:
        path, shader, bounces, res, ref_spp = WORKLOADS[name]
        scene = vpt.HostScene(path)
        dev = vpt.DeviceScene(scene, 0)
        params = vpt.PathtraceParams(resolution=res, samples=ref_spp, shader=shader, bounces=bounces)

        def chain(n):
            """the n-spp render with the sums at n // 2, and the device time of its launches"""
            st = scene.make_state(params)
            dev.pathtrace_samples(st, params, n // 2)
            ms, sum_a = dev.last_kernel_ms(), st.image.copy()
            dev.pathtrace_samples(st, params, n - n // 2)
            return st, sum_a, ms + dev.last_kernel_ms()

        chain(16)   # code objects, launch schedule
        st, _, ref_ms = chain(ref_spp)
        ref = srgb(vpt.get_render(st))
        rms = lambda img: float(np.sqrt(np.mean((srgb(img) - ref) ** 2)))
        vpt.pathtrace_guides(scene, dev, params, GUIDE_SPP)
        t0 = time.perf_counter()
        normal, albedo = vpt.pathtrace_guides(scene, dev, params, GUIDE_SPP)
        guide_wall_ms = (time.perf_counter() - t0) * 1e3   # host clock: the renders with their state uploads and downloads
        guide_ms = 0.0                                      # device events: the launches of the same renders alone
        for guide in (("implicit_normal",) if albedo is None else ("normal", "color")):
            p = vpt.PathtraceParams(resolution=res, samples=GUIDE_SPP, shader=guide, bounces=bounces)
            dev.pathtrace_samples(scene.make_state(p), p, GUIDE_SPP)
            guide_ms += dev.last_kernel_ms()
        emit({"mode": "quality", "workload": name, "run": "reference", "spp": ref_spp, "ms": round(ref_ms, 2), "frame": f"{st.width}x{st.height}",
              "guide_spp": GUIDE_SPP, "guides_ms": round(guide_ms, 2), "guides_wall_ms": round(guide_wall_ms, 2)})
        for n in (16, 64, 256):
            st, sum_a, ms = chain(n)
            color = vpt.get_render(st)
            variance = vpt.half_variance(sum_a, n // 2, st.image, n, device=0)
            f = DeviceFilter(vpt, color, albedo, normal, variance)
            rec = {"mode": "quality", "workload": name, "run": "uniform", "spp": n, "render_ms": round(ms, 2), "rms": rms(color)}
            for seed in ("spatial", "half"):
                for _ in range(3):
                    f.run(use_variance=seed == "half")
                rec[f"filter_{seed}_ms"] = round(float(np.median([f.run(use_variance=seed == "half") for _ in range(9)])), 4)
                rec[f"rms_{seed}"] = rms(f.result())
            for seed, kw in (("half_3_iterations", dict(iterations=3)), ("half_sigma_luminance_2", dict(sigma_luminance=2.0))):
                f.run(**kw)
                rec[f"rms_{seed}"] = rms(f.result())
            f = DeviceFilter(vpt, color, None, None, variance)
            f.run()
            rec["rms_half_no_guides"] = rms(f.result())
            emit(rec)
        dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--speed", action="store_true")
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--workloads", default="headline,config4,frame5")
    ap.add_argument("--repeat", type=int, default=20)
    args = ap.parse_args()
    if args.speed == args.quality:
        ap.error("one of --speed and --quality")
    os.makedirs(args.out, exist_ok=True)
    vpt = vpt_loader.load()
    if vpt.device_count() < 1:
        raise SystemExit("denoise_measure needs a GPU: nothing here is measured on a CPU")
    records = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        records.append(rec)
        with open(os.path.join(args.out, f"denoise_measure_{'speed' if args.speed else 'quality'}.json"), "w") as f:
            json.dump(records, f, indent=1)

    if args.speed:
        speed(vpt, emit, args.repeat)
    else:
        quality(vpt, emit, args.workloads.split(","))


if __name__ == "__main__":
    main()
