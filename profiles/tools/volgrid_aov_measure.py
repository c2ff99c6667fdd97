"""The first-collision pass of the volgrid shader measured on §29's dense and sparse scenes at 1280 x 533 x 64 samples:
the opacity-only pass and the all-planes pass (vpt_render_volgrid_aov_device) against the only comparable thing K3 can do, a volgrid
render with bounces = 1 (vpt_render_device), all three on device-resident state, alternating in every round after --discard warm-up
rounds in ONE process, timed by events on the launch stream; median, minimum and maximum of --repeat rounds.  Then, on the dense
scene's session: the latency of a pick after a reset (the id frame is made: guide_samples flights per pixel) and of the next pick,
the bytes either moves to the host, and sculpt_at end to end against the same pick + get_voxels + a host sculpt + set_volume
through edit_volumes.
One JSON line per record, and the list in <out>/volgrid_aov_measure.json.

  python profiles/tools/volgrid_aov_measure.py [--out DIR (default profiles)] [--repeat 5] [--discard 2] [--resolution 1280] [--samples 64]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vpt_loader  # noqa: E402
from volgrid_measure import F, GRIDSDF, scene_with, stat  # noqa: E402

ALL = ("opacity", "albedo", "depth", "normal", "ids", "hit")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--resolution", type=int, default=1280)
    ap.add_argument("--samples", type=int, default=64)
    args = ap.parse_args()
    vpt = vpt_loader.load()
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    sdf, res = vpt.HostScene(GRIDSDF).volume(0)
    dense = vpt.density_from_sdf(sdf, 2.0 * res)
    sparse = np.zeros((128, 128, 128), F)
    sparse[48:80, 48:80, 48:80] = 1.0
    params = vpt.PathtraceParams(resolution=args.resolution, shader="volgrid", samples=args.samples, bounces=1)
    for name, voxels in (("dense", dense), ("sparse", sparse)):
        scene = scene_with(vpt, voxels, 0.05)
        dev = vpt.DeviceScene(scene, 0)
        st = scene.make_state(params)
        lay = vpt.VptLayout(st.width, st.height, 8, 8, 0, 1)
        slots, pixels = vpt.layout_slots(lay), st.width * st.height
        image = torch.zeros((slots, 4), device="cuda")
        hits, rng = torch.zeros(slots, dtype=torch.int32, device="cuda"), torch.zeros((slots, 2), dtype=torch.int64, device="cuda")
        planes = {k: torch.zeros((slots, 2 if k == "ids" else 4), dtype=torch.int32 if k == "ids" else torch.float32, device="cuda") for k in ALL}
        ptr = lambda names: {k: planes[k].data_ptr() for k in names}
        runs = {"k3_bounces_1": lambda: dev.render_device(params, lay, args.samples, image.data_ptr(), hits.data_ptr(), rng.data_ptr()),
                "aov_opacity": lambda: dev.render_volgrid_aov_device(params, lay, args.samples, ptr(("opacity",)), hits.data_ptr(), rng.data_ptr()),
                "aov_all_planes": lambda: dev.render_volgrid_aov_device(params, lay, args.samples, ptr(ALL), hits.data_ptr(), rng.data_ptr())}
        ms = {k: [] for k in runs}
        for r in range(args.discard + args.repeat):
            for k, run in runs.items():
                vpt.state_init_device(lay, image.data_ptr(), hits.data_ptr(), rng.data_ptr())   # every run flies the same streams
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run()
                b.record()
                torch.cuda.synchronize()
                if r >= args.discard:
                    ms[k].append(a.elapsed_time(b))
        for k in runs:
            emit({"what": "pass", "scene": name, "grid": list(voxels.shape), "run": k, "width": st.width, "height": st.height, "samples": args.samples,
                  "stream_ms": stat(ms[k]), "msamples_per_s": stat([pixels * args.samples / t / 1e3 for t in ms[k]])})
        if name != "dense":
            continue
        s = vpt.RenderSession(dev, vpt.PathtraceParams(resolution=args.resolution, shader="volgrid", samples=args.samples, bounces=8), pratio=8,
                              guide_samples=16)
        first, again, down = [], [], []
        for r in range(args.discard + args.repeat):
            s.reset()
            t0 = time.perf_counter()
            pick = s.pick_volgrid(st.width // 2, st.height // 2)
            t1 = time.perf_counter()
            d0 = s.stats()[2]
            s.pick_volgrid(st.width // 2 + 3, st.height // 2)
            t2 = time.perf_counter()
            if r >= args.discard:
                first.append((t1 - t0) * 1e3), again.append((t2 - t1) * 1e3), down.append((d0, s.stats()[2]))
        emit({"what": "pick", "width": st.width, "height": st.height, "guide_samples": 16, "hit": pick is not None, "first_pick_after_reset_wall_ms": stat(first),
              "next_pick_wall_ms": stat(again), "bytes_to_host_first_and_next": list(down[-1])})
        # sculpt_at end to end (pick, host mirror, the sculpt kernel over the region, reset) against the way round it: the same pick, then
        # get_voxels (the whole volume comes back), the host mirror of the stamp, set_volume of the whole volume through edit_volumes.
        # A pixel of its own per round, 50 apart for a brush 20 pixels wide: a stroke repeated in place would drill through the cloud
        brush = vpt.VptSdf(type=vpt.SDF_TYPES.index("sphere"))
        brush.frame.x[:], brush.frame.y[:], brush.frame.z[:] = (1, 0, 0), (0, 1, 0), (0, 0, 1)
        brush.p[0] = 0.02
        at, by_hand, parts = [], [], []
        for r in range(args.discard + args.repeat):
            x, y = st.width // 2 - 150 + 50 * r, st.height // 2
            t0 = time.perf_counter()
            entry = s.sculpt_at(scene, x, y, brush, vpt.SCULPT_UNION)
            t1 = time.perf_counter()
            s.pick_volgrid(x + 25, y)
            t2 = time.perf_counter()
            vox = dev.get_voxels(0)
            t3 = time.perf_counter()
            scene.sculpt_volume(0, entry.stamps, region=(entry.region_lo, entry.region_whd))
            scene.update_sculpts()
            t4 = time.perf_counter()
            scene.set_volume(0, scene.volume(0)[0], res=1.0 / vox.shape[2])
            s.edit_volumes(scene.update_volumes())
            t5 = time.perf_counter()
            if r >= args.discard:
                at.append((t1 - t0) * 1e3), by_hand.append((t5 - t1) * 1e3)
                parts.append([(b - a) * 1e3 for a, b in ((t1, t2), (t2, t3), (t3, t4), (t4, t5))])
        emit({"what": "sculpt_at end to end against pick + get_voxels + host sculpt + set_volume", "grid": list(dense.shape), "region": list(entry.region_whd),
              "sculpt_at_wall_ms": stat(at), "by_hand_wall_ms": stat(by_hand),
              "by_hand_parts_median_ms": dict(zip(("pick", "get_voxels", "host_sculpt", "set_volume_and_edit"), np.median(parts, axis=0).tolist())),
              "ratio": float(np.median(by_hand) / np.median(at))})
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "volgrid_aov_measure.json"), "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
