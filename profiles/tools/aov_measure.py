"""The first-hit pass (include/vpt.h: vpt_render_aov_device) measured against what it replaces, on 03_volume at each
--resolutions width with --guides samples.  Everything runs in ONE process, the two sides of a comparison alternating round by round
after --discard warm-up rounds; every figure is the median (and minimum) of --repeat rounds.

 (a) guides   device time (events around the enqueued work) of the guides of a session reset:
              separate  2 x (vpt_state_init_device, vpt_render_device of `normal` / `color`, vpt_resolve_device) - the parent's reset
              fused     vpt_state_init_device, a memset, ONE vpt_render_aov_device (normal + albedo), 2 x vpt_resolve_device
              The `separate` row is taken --spread (5) times: the spread of its medians is what a difference has to exceed, and the bar
              for the session is  fused median <= separate median + spread.  The resolved guides of both sides are compared bit for bit.
 (b) offline  wall time of pathtrace_guides: two renders through host states (the parent's)  against  one vpt_render_aov
 (c) pick     wall time of the first pick after a reset (it makes the id frame) and of the next one (24 bytes)
 One JSON line per record, and the list in <out>/aov_measure.json.

  python profiles/tools/aov_measure.py [--out DIR (default profiles)] [--repeat 8] [--discard 2] [--resolutions 1280,3840] [--guides 16]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import vpt_loader  # noqa: E402

SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "03_volume", "volume.json")


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "max_ms": float(np.max(xs)), "n": len(xs)}


def measure(vpt, torch, scene, dev, resolution, repeat, discard, guide_samples, spread_rows):
    out = []
    sync = torch.cuda.synchronize
    params = vpt.PathtraceParams(resolution=resolution, samples=4096, shader="volpathtrace", bounces=64)
    st = scene.make_state(params)
    w, h = st.width, st.height
    layout = vpt.VptLayout(w, h, 8, 8, 0, 1)
    slots = vpt.layout_slots(layout)
    d_img = torch.zeros((slots, 4), dtype=torch.float32, device="cuda")
    d_alb = torch.zeros((slots, 4), dtype=torch.float32, device="cuda")
    d_hits = torch.zeros((slots,), dtype=torch.int32, device="cuda")
    d_rng = torch.zeros((slots, 2), dtype=torch.int64, device="cuda")
    rows = {k: torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for k in ("sep_normal", "sep_albedo", "fused_normal", "fused_albedo")}
    size = f"{w}x{h}"
    state = (d_img.data_ptr(), d_hits.data_ptr(), d_rng.data_ptr())

    def separate():
        for shader, row in (("normal", "sep_normal"), ("color", "sep_albedo")):
            p = vpt.PathtraceParams(resolution=resolution, samples=guide_samples, shader=shader, bounces=64)
            vpt.state_init_device(layout, *state)
            dev.render_device(p, layout, guide_samples, *state)
            vpt.resolve_device(layout, d_img.data_ptr(), guide_samples, rows[row].data_ptr())

    def fused():
        p = vpt.PathtraceParams(resolution=resolution, samples=guide_samples, shader="normal", bounces=64)
        vpt.state_init_device(layout, *state)
        d_alb.zero_()
        dev.render_aov_device(p, layout, guide_samples, {"normal": d_img.data_ptr(), "albedo": d_alb.data_ptr()}, d_hits.data_ptr(), d_rng.data_ptr())
        vpt.resolve_device(layout, d_img.data_ptr(), guide_samples, rows["fused_normal"].data_ptr())
        vpt.resolve_device(layout, d_alb.data_ptr(), guide_samples, rows["fused_albedo"].data_ptr())

    def device_ms(work):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        a.record()
        work()
        b.record()
        sync()
        return a.elapsed_time(b)

    # (a) the guides of a reset
    sep_rows, fus = [[] for _ in range(spread_rows)], []
    for row in range(spread_rows):
        for r in range(repeat + discard):
            t_sep, t_fus = device_ms(separate), device_ms(fused)
            if r >= discard:
                sep_rows[row].append(t_sep), fus.append(t_fus)
    same = all(torch.equal(rows["sep_" + k].view(torch.int32), rows["fused_" + k].view(torch.int32)) for k in ("normal", "albedo"))
    medians = [float(np.median(x)) for x in sep_rows]
    spread = max(medians) - min(medians)
    rec = {"measure": "reset_guides_device_ms", "size": size, "samples": guide_samples, "separate_renders": stat([t for x in sep_rows for t in x]),
           "separate_row_medians_ms": medians, "separate_spread_ms": spread, "fused_pass": stat(fus), "same_bits": bool(same)}
    rec["fused_over_separate_median"] = rec["fused_pass"]["median_ms"] / rec["separate_renders"]["median_ms"]
    rec["bar_met"] = bool(rec["fused_pass"]["median_ms"] <= rec["separate_renders"]["median_ms"] + spread)
    print(json.dumps(rec), flush=True)
    out.append(rec)

    # (b) pathtrace_guides
    def two_renders():
        for shader in ("normal", "color"):
            p = vpt.PathtraceParams(resolution=resolution, samples=guide_samples, shader=shader, bounces=64)
            s = scene.make_state(p)
            dev.pathtrace_samples(s, p, guide_samples)
            vpt.get_render(s)

    old, new = [], []
    for r in range(repeat + discard):
        sync()
        t0 = time.perf_counter()
        two_renders()
        t1 = time.perf_counter()
        vpt.pathtrace_guides(scene, dev, params, guide_samples)
        t2 = time.perf_counter()
        if r >= discard:
            old.append((t1 - t0) * 1e3), new.append((t2 - t1) * 1e3)
    rec = {"measure": "pathtrace_guides_wall_ms", "size": size, "samples": guide_samples, "two_host_state_renders": stat(old), "one_aov_pass": stat(new)}
    rec["speedup_median"] = rec["two_host_state_renders"]["median_ms"] / rec["one_aov_pass"]["median_ms"]
    print(json.dumps(rec), flush=True)
    out.append(rec)

    # (c) a pick
    s = vpt.RenderSession(dev, params, pratio=8)
    first, again = [], []
    for r in range(repeat + discard):
        s.reset()
        sync()
        t0 = time.perf_counter()
        s.pick(w // 2, h // 2)
        t1 = time.perf_counter()
        s.pick(w // 3, h // 3)
        t2 = time.perf_counter()
        if r >= discard:
            first.append((t1 - t0) * 1e3), again.append((t2 - t1) * 1e3)
    rec = {"measure": "pick_wall_ms", "size": size, "first_pick_after_reset": stat(first), "next_pick": stat(again), "next_pick_stats": list(s.stats())}
    s.close()
    print(json.dumps(rec), flush=True)
    out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--spread", type=int, default=5)
    ap.add_argument("--resolutions", default="1280,3840")
    ap.add_argument("--guides", type=int, default=16)
    a = ap.parse_args()
    vpt = vpt_loader.load()
    import torch
    if vpt.device_count() < 1:
        raise SystemExit("aov_measure needs a GPU: nothing here is measured without one")
    scene = vpt.HostScene(SCENE)
    dev = vpt.DeviceScene(scene, 0)
    records = []
    for resolution in (int(r) for r in a.resolutions.split(",")):
        records += measure(vpt, torch, scene, dev, resolution, a.repeat, a.discard, a.guides, a.spread)
    os.makedirs(a.out, exist_ok=True)
    json.dump(records, open(os.path.join(a.out, "aov_measure.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
