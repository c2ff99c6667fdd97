"""The sphere-traced first-hit pass (include/vpt.h: vpt_render_sdf_aov_device) measured against the routes a caller had
before it, on 06_gridsdf_full and 07_sdfunction_synth at --resolution (1280: 1280 x 533).  Everything runs in ONE process, the two sides
of a comparison alternating round by round after --discard warm-up rounds; every figure is the median (minimum, maximum) of --repeat rounds.

 (a) normal   device time (events around the enqueued work) of the normal plane at --samples samples:
              k2     vpt_state_init_device, vpt_render_device with `implicit_normal` - K2, the regenerating state machine with its launch
                     schedule and tile splitting: the only way to this plane before the pass
              pass   vpt_state_init_device, a memset, ONE vpt_render_sdf_aov_device (normal alone); and the same with all five planes
              The k2 row is taken --spread times: the spread of its medians is what a difference has to exceed.  Bits are compared.
 (b) groups   the pass of (a) on a second handle of the same scene made under VPT_NO_GROUP_FORMS=1 (every ray marches in its own lane),
              alternating with the first handle's (the four-lanes-per-ray round on).  Bits are compared.
 (c) pick     wall time of the first pick_sdf after a reset of an implicit session (it makes the id frame: 3 launches) and of the next one
              (48 bytes), against the only route before: the rays through the pixel centres handed to vpt_spheretrace - timed with the rays
              already made (a lower bound of that route: w * h rays up, ids and t down) and with the rays made by VPT_KAT_CAMERA first.
 One JSON line per record, and the list in <out>/sdf_aov_measure.json.

  python profiles/tools/sdf_aov_measure.py [--out DIR (default profiles)] [--repeat 8] [--discard 2] [--resolution 1280] [--samples 16]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import vpt_loader  # noqa: E402

SCENES = {"06_gridsdf_full": os.path.join(ROOT, "tests", "golden", "scenes", "06_gridsdf_full", "gridsdf_full.json"),
          "07_sdfunction_synth": os.path.join(ROOT, "tests", "golden", "scenes", "07_sdfunction_synth", "sdfunction_synth.json")}
PLANES = ("normal", "albedo", "depth", "ids", "hit")


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "max_ms": float(np.max(xs)), "n": len(xs)}


def measure(vpt, torch, name, a):
    out = []
    sync = torch.cuda.synchronize
    scene = vpt.HostScene(SCENES[name])
    dev = vpt.DeviceScene(scene, 0)
    os.environ["VPT_NO_GROUP_FORMS"] = "1"   # read when a handle is created
    dev_own = vpt.DeviceScene(scene, 0)
    del os.environ["VPT_NO_GROUP_FORMS"]
    params = vpt.PathtraceParams(resolution=a.resolution, samples=a.samples, shader="implicit_normal", bounces=4)
    st = scene.make_state(params)
    w, h = st.width, st.height
    layout = vpt.VptLayout(w, h, 8, 8, 0, 1)
    slots = vpt.layout_slots(layout)
    size = f"{w}x{h}"
    d_img = torch.zeros((slots, 4), dtype=torch.float32, device="cuda")
    d_hits = torch.zeros((slots,), dtype=torch.int32, device="cuda")
    d_rng = torch.zeros((slots, 2), dtype=torch.int64, device="cuda")
    planes = {k: torch.zeros((slots, 2), dtype=torch.int32, device="cuda") if k == "ids" else torch.zeros((slots, 4), dtype=torch.float32, device="cuda")
              for k in PLANES}
    state = (d_img.data_ptr(), d_hits.data_ptr(), d_rng.data_ptr())
    kept = {}

    def k2():
        vpt.state_init_device(layout, *state)
        dev.render_device(params, layout, a.samples, *state)

    def the_pass(device, names):
        def work():
            vpt.state_init_device(layout, *state)   # its image plane is not used: the pass has planes of its own
            for k in names:
                if k not in ("ids", "hit"):
                    planes[k].zero_()
            device.render_sdf_aov_device(params, layout, a.samples, {k: planes[k].data_ptr() for k in names}, d_hits.data_ptr(), d_rng.data_ptr())
        return work

    def device_ms(work, keep=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        e0.record()
        work()
        e1.record()
        sync()
        if keep:
            kept[keep] = (d_img if keep == "k2" else planes["normal"]).clone()
        return e0.elapsed_time(e1)

    # (a) the normal plane
    k2_rows, one, five = [[] for _ in range(a.spread)], [], []
    for row in range(a.spread):
        for r in range(a.repeat + a.discard):
            t = device_ms(k2, "k2"), device_ms(the_pass(dev, ("normal",)), "pass"), device_ms(the_pass(dev, PLANES))
            if r >= a.discard:
                k2_rows[row].append(t[0]), one.append(t[1]), five.append(t[2])
    medians = [float(np.median(x)) for x in k2_rows]
    rec = {"measure": "normal_plane_device_ms", "scene": name, "size": size, "samples": a.samples, "k2_implicit_normal": stat([t for x in k2_rows for t in x]),
           "k2_row_medians_ms": medians, "k2_spread_ms": max(medians) - min(medians), "pass_normal_only": stat(one), "pass_all_five_planes": stat(five),
           "same_bits": bool(torch.equal(kept["k2"].view(torch.int32), kept["pass"].view(torch.int32)))}
    rec["pass_over_k2_median"] = rec["pass_normal_only"]["median_ms"] / rec["k2_implicit_normal"]["median_ms"]
    print(json.dumps(rec), flush=True)
    out.append(rec)

    # (b) the group round on against off
    on, off = [], []
    for r in range(a.repeat + a.discard):
        t = device_ms(the_pass(dev, ("normal",)), "on"), device_ms(the_pass(dev_own, ("normal",)), "off")
        if r >= a.discard:
            on.append(t[0]), off.append(t[1])
    rec = {"measure": "group_round_device_ms", "scene": name, "size": size, "samples": a.samples, "group_round_on": stat(on), "group_round_off": stat(off),
           "same_bits": bool(torch.equal(kept["on"].view(torch.int32), kept["off"].view(torch.int32)))}
    rec["on_over_off_median"] = rec["group_round_on"]["median_ms"] / rec["group_round_off"]["median_ms"]
    print(json.dumps(rec), flush=True)
    out.append(rec)

    # (c) the id frame and a later pick
    s = vpt.RenderSession(dev, vpt.PathtraceParams(resolution=a.resolution, samples=64, shader="implicit", bounces=4), pratio=8)
    rec5 = np.zeros((h, w, 5), np.float32)
    rec5[..., 1] = ((np.arange(w, dtype=np.float32) + np.float32(0.5)) / np.float32(w))[None, :]
    rec5[..., 2] = ((np.arange(h, dtype=np.float32) + np.float32(0.5)) / np.float32(h))[:, None]
    rec5 = rec5.reshape(-1, 5)
    rays = dev.kat(3, rec5)
    first, again, traced, made_and_traced = [], [], [], []
    for r in range(a.repeat + a.discard):
        s.reset()
        sync()
        t0 = time.perf_counter()
        s.pick_sdf(w // 2, h // 2)
        t1 = time.perf_counter()
        s.pick_sdf(w // 3, h // 3)
        t2 = time.perf_counter()
        ids, t = dev.spheretrace(rays, -1, 450)
        t3 = time.perf_counter()
        dev.spheretrace(dev.kat(3, rec5), -1, 450)
        t4 = time.perf_counter()
        if r >= a.discard:
            first.append((t1 - t0) * 1e3), again.append((t2 - t1) * 1e3), traced.append((t3 - t2) * 1e3), made_and_traced.append((t4 - t3) * 1e3)
    frame_ids, frame_hit = s.sdf_ids()
    hit = ids[:, 0] == 1
    same = np.array_equal(frame_ids.reshape(-1, 2)[hit], ids[hit, 1:3]) and np.array_equal(frame_hit.reshape(-1, 4)[hit, 3].view(np.uint32), t[hit].view(np.uint32))
    s.pick_sdf(w // 3, h // 3)
    rec = {"measure": "pick_wall_ms", "scene": name, "size": size, "first_pick_sdf_after_reset": stat(first), "next_pick_sdf": stat(again),
           "next_pick_stats": list(s.stats()), "spheretrace_of_ready_rays": stat(traced),
           "kat_camera_then_spheretrace": stat(made_and_traced), "same_ids_and_t": bool(same), "hits": int(hit.sum()), "pixels": int(w * h)}
    rec["frame_speedup_median"] = rec["spheretrace_of_ready_rays"]["median_ms"] / rec["first_pick_sdf_after_reset"]["median_ms"]
    s.close()
    print(json.dumps(rec), flush=True)
    out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--spread", type=int, default=3)
    ap.add_argument("--resolution", type=int, default=1280)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--scenes", default=",".join(SCENES))
    a = ap.parse_args()
    vpt = vpt_loader.load()
    import torch
    if vpt.device_count() < 1:
        raise SystemExit("sdf_aov_measure needs a GPU: nothing here is measured without one")
    records = []
    for name in a.scenes.split(","):
        records += measure(vpt, torch, name, a)
    os.makedirs(a.out, exist_ok=True)
    json.dump(records, open(os.path.join(a.out, "sdf_aov_measure.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
