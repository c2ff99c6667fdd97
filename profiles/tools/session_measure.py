"""vpt_session measured against the path the library offered for a frame loop before it, on 03_volume, volpathtrace,
64 bounces, at each --resolutions width.  Both paths run in ONE process in interleaved rounds after --discard warm-up rounds; times are
a host clock around a device synchronise; median and minimum of --repeat rounds.

 (a) restart   vpt_session_reset (+ synchronise)  against  host make_state, vpt_state_upload, a preview through vpt_render on a host
               state, the host upscale and the host tone map to bytes
 (b) frame     advance(n) + display() as bytes, n = 1, 4, 16  against  vpt_render on host arrays, get_render, the host tone map to
               bytes; the render kernels' own time (vpt_last_kernel_ms) is subtracted on both sides: what is left is the frame's overhead
 (c) guides    normal + color guides of --guides samples rendered into device buffers (vpt_state_init_device, vpt_render_device,
               vpt_resolve_device)  against  pathtrace_guides through host states
 One JSON line per record, and the list in <out>/session_measure.json.

 (d) --kernels: launches the three new kernels --repeat times at each size and nothing else, to be run under
     rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 profiles/tools/session_measure.py --kernels
     and --summarize DIR turns that run's kernel trace into records (per kernel and grid: median and minimum duration, bytes moved per
     pixel, the time those bytes take at bench.py's HBM figure) appended to <out>/session_measure.json.

  python profiles/tools/session_measure.py [--out DIR (default .)] [--repeat 8] [--discard 2] [--resolutions 1280,3840] [--guides 16]"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import vpt_loader  # noqa: E402

SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "03_volume", "volume.json")
HBM_BYTES_PER_S = 8.0e12   # bench.py's roofline figure
PRATIO = 8
# bytes per pixel (slot) a kernel has to move: state init writes 16 + 4 + 16; the tone map reads 16 and writes 16 + 4 (both displays, as
# the session runs it); the upscale writes 16 and reads 16 from a preview 64 times smaller (counted in full, as an upper bound)
KERNEL_BYTES = {"vpt_state_init_kernel": 36, "vpt_tonemap_kernel": 36, "vpt_upscale_kernel": 32}


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "n": len(xs)}


def measure(vpt, torch, scene, dev, resolution, repeat, discard, guide_samples):
    out = []
    sync = torch.cuda.synchronize
    params = vpt.PathtraceParams(resolution=resolution, samples=4096, shader="volpathtrace", bounces=64)
    pp = vpt.PathtraceParams(resolution=resolution // PRATIO, samples=1, shader="volpathtrace", bounces=64)
    s = vpt.RenderSession(dev, params, pratio=PRATIO)
    w, h = s.size
    layout = vpt.VptLayout(w, h, 8, 8, 0, 1)
    slots = vpt.layout_slots(layout)
    d_img = torch.zeros((slots, 4), dtype=torch.float32, device="cuda")
    d_hits = torch.zeros((slots,), dtype=torch.int32, device="cuda")
    d_rng = torch.zeros((slots, 2), dtype=torch.int64, device="cuda")
    d_rows = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    size = f"{w}x{h}"

    # (a) restart
    new, old, new_shown = [], [], []
    for r in range(repeat + discard):
        sync()
        t0 = time.perf_counter()
        s.reset()
        sync()
        t1 = time.perf_counter()
        s.display()
        t2 = time.perf_counter()
        st = scene.make_state(params)
        vpt.state_upload(layout, st, d_img.data_ptr(), d_hits.data_ptr(), d_rng.data_ptr())
        pst = scene.make_state(pp)
        dev.pathtrace_samples(pst, pp, 1)
        vpt.tonemap_image(vpt.upscale_preview(vpt.get_render(pst), PRATIO, w, h), as_bytes=True)
        t3 = time.perf_counter()
        if r >= discard:
            new.append((t1 - t0) * 1e3), new_shown.append((t2 - t0) * 1e3), old.append((t3 - t2) * 1e3)
    rec = {"measure": "restart", "size": size, "session_reset": stat(new), "session_reset_and_display_bytes": stat(new_shown),
           "host_make_state_upload_preview_tonemap": stat(old)}
    rec["speedup_median"] = rec["host_make_state_upload_preview_tonemap"]["median_ms"] / rec["session_reset"]["median_ms"]
    print(json.dumps(rec), flush=True)
    out.append(rec)

    # (b) a display frame every n samples
    for n in (1, 4, 16):
        s.reset()
        st = scene.make_state(params)
        new, old, new_k, old_k = [], [], [], []
        for r in range(repeat + discard):
            sync()
            t0 = time.perf_counter()
            s.advance(n)
            s.display()
            t1 = time.perf_counter()
            k1 = dev.last_kernel_ms()
            t2 = time.perf_counter()
            dev.pathtrace_samples(st, params, n)
            vpt.tonemap_image(vpt.get_render(st), as_bytes=True)
            t3 = time.perf_counter()
            k2 = dev.last_kernel_ms()
            if r >= discard:
                new.append((t1 - t0) * 1e3 - k1), old.append((t3 - t2) * 1e3 - k2), new_k.append(k1), old_k.append(k2)
        rec = {"measure": "frame_overhead", "size": size, "spp_per_frame": n, "session_advance_display_minus_kernel": stat(new),
               "host_render_get_render_tonemap_minus_kernel": stat(old), "render_kernel_session": stat(new_k), "render_kernel_host_path": stat(old_k)}
        rec["overhead_ratio_median"] = rec["host_render_get_render_tonemap_minus_kernel"]["median_ms"] / rec["session_advance_display_minus_kernel"]["median_ms"]
        print(json.dumps(rec), flush=True)
        out.append(rec)
    s.close()

    # (c) the guides
    new, old = [], []
    for r in range(repeat + discard):
        sync()
        t0 = time.perf_counter()
        for shader in ("normal", "color"):
            p = vpt.PathtraceParams(resolution=resolution, samples=guide_samples, shader=shader, bounces=64)
            vpt.state_init_device(layout, d_img.data_ptr(), d_hits.data_ptr(), d_rng.data_ptr())
            dev.render_device(p, layout, guide_samples, d_img.data_ptr(), d_hits.data_ptr(), d_rng.data_ptr())
            vpt.resolve_device(layout, d_img.data_ptr(), guide_samples, d_rows.data_ptr())
        sync()
        t1 = time.perf_counter()
        vpt.pathtrace_guides(scene, dev, params, guide_samples)
        t2 = time.perf_counter()
        if r >= discard:
            new.append((t1 - t0) * 1e3), old.append((t2 - t1) * 1e3)
    rec = {"measure": "guides", "size": size, "samples": guide_samples, "device_resident": stat(new), "pathtrace_guides_host_states": stat(old)}
    rec["speedup_median"] = rec["pathtrace_guides_host_states"]["median_ms"] / rec["device_resident"]["median_ms"]
    print(json.dumps(rec), flush=True)
    out.append(rec)
    return out


def kernels(vpt, torch, scene, resolutions, repeat):
    """the three new kernels alone, `repeat` launches per size (for a rocprofv3 --kernel-trace run)"""
    for resolution in resolutions:
        st = scene.make_state(vpt.PathtraceParams(resolution=resolution))
        w, h = st.width, st.height
        pw, ph = max(1, w // PRATIO), max(1, h // PRATIO)
        layout = vpt.VptLayout(w, h, 8, 8, 0, 1)
        slots = vpt.layout_slots(layout)
        d_img = torch.zeros((slots, 4), dtype=torch.float32, device="cuda")
        d_hits = torch.zeros((slots,), dtype=torch.int32, device="cuda")
        d_rng = torch.zeros((slots, 2), dtype=torch.int64, device="cuda")
        d_rows = torch.rand((h, w, 4), dtype=torch.float32, device="cuda")
        d_f = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        d_b = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        d_prev = torch.rand((ph, pw, 4), dtype=torch.float32, device="cuda")
        for _ in range(repeat):
            vpt.state_init_device(layout, d_img.data_ptr(), d_hits.data_ptr(), d_rng.data_ptr())
            vpt.tonemap_device(w, h, d_rows.data_ptr(), d_f.data_ptr(), d_b.data_ptr(), vpt.DisplayParams(1.25, True, True))
            vpt.upscale_device(PRATIO, pw, ph, d_prev.data_ptr(), w, h, d_f.data_ptr())
            torch.cuda.synchronize()
        print(json.dumps({"kernels": f"{w}x{h}", "slots": slots, "launches_each": repeat}), flush=True)


def summarize(directory, vpt, scene, resolutions):
    """records from the kernel trace rocprofv3 wrote under `directory` for a --kernels run"""
    rows = []
    for f in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    pixels = {}
    for resolution in resolutions:
        st = scene.make_state(vpt.PathtraceParams(resolution=resolution))
        pixels[f"{st.width}x{st.height}"] = (st.width * st.height, vpt.layout_slots(vpt.VptLayout(st.width, st.height, 8, 8, 0, 1)))
    out = []
    for name, per_pixel in KERNEL_BYTES.items():
        groups = {}
        for r in rows:
            if name in r["Kernel_Name"]:
                grid = int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0) * max(1, int(r.get("Grid_Size_Y", 1) or 1))
                groups.setdefault(grid, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
        # the sizes in ascending order of their grids
        for (size, (npix, slots)), grid in zip(sorted(pixels.items(), key=lambda kv: kv[1][0]), sorted(groups)):
            ms = groups[grid][1:] or groups[grid]   # the first launch of a kernel loads its code object
            count = slots if name == "vpt_state_init_kernel" else npix
            bound = count * per_pixel / HBM_BYTES_PER_S * 1e3
            out.append({"measure": "kernel", "kernel": name, "size": size, "grid_threads": grid, "duration": stat(ms), "bytes_per_pixel": per_pixel,
                        "hbm_bound_ms": bound, "median_over_bound": float(np.median(ms)) / bound})
            print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--resolutions", default="1280,3840")
    ap.add_argument("--guides", type=int, default=16)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--summarize", default=None, metavar="DIR")
    a = ap.parse_args()
    vpt = vpt_loader.load()
    scene = vpt.HostScene(SCENE)
    resolutions = [int(r) for r in a.resolutions.split(",")]
    target = os.path.join(a.out, "session_measure.json")
    if a.summarize:
        records = json.load(open(target)) if os.path.exists(target) else []
        records = [r for r in records if r.get("measure") != "kernel"] + summarize(a.summarize, vpt, scene, resolutions)
    else:
        import torch
        if a.kernels:
            return kernels(vpt, torch, scene, resolutions, a.repeat)
        dev = vpt.DeviceScene(scene, 0)
        records = []
        for resolution in resolutions:
            records += measure(vpt, torch, scene, dev, resolution, a.repeat, a.discard, a.guides)
    os.makedirs(a.out, exist_ok=True)
    json.dump(records, open(target, "w"), indent=1)


if __name__ == "__main__":
    main()
