#!/usr/bin/env python3
"""Wall time of the entry points that are mostly copies between row-major pixels and tile-major slots (csrc/vpt_layout.hip), on
03_volume at the benchmark's 1280 x 533 frame.  Every timed call ends in a synchronise of its own; a host clock around it, after a warm-up:
  state_pair      vpt_state_upload + vpt_state_download of one rank's state
  render_aov      one vpt_render_aov with all six planes at 1 sample
  session_state   vpt_session_get_state
One process measures one build of the library:
  layout_copy_measure.py [--root TREE] [--calls 20] [--warmup 3]          -> one JSON line: per measure the median / min / max ms of the calls
Two builds against each other (each repetition a fresh process, the two trees alternating; the tree this file is in is the branch):
  layout_copy_measure.py --parent TREE [--repeat 5] [--out profiles/layout_copy_measure.json]
The verdict per measure: the branch's median over its repetitions lies within the spread (min .. max) of the parent's repetitions."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MEASURES = ("state_pair", "render_aov", "session_state")


def measure(root, calls, warmup):
    sys.path.insert(0, root)
    import vpt_loader
    vpt = vpt_loader.load()
    import torch
    if vpt.device_count() < 1:
        raise SystemExit("layout_copy_measure needs a GPU: nothing here is measured without one")
    scene = vpt.HostScene(os.path.join(root, "tests", "golden", "scenes", "03_volume", "volume.json"))
    dev = vpt.DeviceScene(scene, 0)
    params = vpt.PathtraceParams(resolution=1280, samples=1 << 20, shader="volpathtrace", bounces=64)
    host = scene.make_state(params)
    w, h = host.width, host.height
    lay = vpt.VptLayout(w, h, 8, 8, 0, 1)
    slots = vpt.layout_slots(lay)
    d = torch.device("cuda", 0)
    img = torch.zeros((slots, 4), dtype=torch.float32, device=d)
    hit = torch.zeros((slots,), dtype=torch.int32, device=d)
    rng = torch.zeros((slots, 2), dtype=torch.int64, device=d)
    back = host.copy()

    def state_pair():
        vpt.state_upload(lay, host, img.data_ptr(), hit.data_ptr(), rng.data_ptr())
        vpt.state_download(lay, img.data_ptr(), hit.data_ptr(), rng.data_ptr(), back)

    shapes = {"ids": ((2,), np.int32), "uvt": ((3,), np.float32)}
    planes = {}
    for name in vpt.AOV_PLANES:
        tail, dtype = shapes.get(name, ((4,), np.float32))
        planes[name] = np.zeros((h, w) + tail, dtype)
    abi, pl = params.to_abi(), vpt.VptAovPlanes(**{k: a.ctypes.data for k, a in planes.items()})
    aov_state = host.copy()

    def render_aov():
        samples = C.c_int(0)
        rc = vpt.hip.vpt_render_aov(dev.handle, C.byref(abi), 1, w, h, C.byref(pl), aov_state.hits.ctypes.data, aov_state.rngs.ctypes.data,
                                    C.byref(samples))
        assert rc == 0 and samples.value == 1, vpt.hip.vpt_last_error().decode()

    session = vpt.RenderSession(dev, params, pratio=8)
    session.reset()
    session.advance(1)
    got = host.copy()

    def session_state():
        n = C.c_int(0)
        rc = vpt.hip.vpt_session_get_state(session.handle, got.image.ctypes.data, got.hits.ctypes.data, got.rngs.ctypes.data, C.byref(n))
        assert rc == 0, vpt.hip.vpt_last_error().decode()

    rec = {"root": os.path.relpath(root, HERE), "size": f"{w}x{h}", "calls": calls}
    for name, work in zip(MEASURES, (state_pair, render_aov, session_state)):
        for _ in range(warmup):
            work()
        torch.cuda.synchronize()
        ms = []
        for _ in range(calls):
            t0 = time.perf_counter()
            work()
            ms.append((time.perf_counter() - t0) * 1e3)
        rec[name] = {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
    session.close()
    print(json.dumps(rec), flush=True)


def compare(parent, repeat, calls, warmup, out):
    runs = {"parent": [], "branch": []}
    for _ in range(repeat):
        for side, root in (("parent", os.path.abspath(parent)), ("branch", HERE)):
            line = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--calls", str(calls), "--warmup", str(warmup)],
                                  check=True, stdout=subprocess.PIPE, text=True, timeout=300).stdout.strip().splitlines()[-1]
            print(side, line, flush=True)
            runs[side].append(json.loads(line))
    verdict = {}
    for name in MEASURES:
        p = [r[name]["median_ms"] for r in runs["parent"]]
        b = [r[name]["median_ms"] for r in runs["branch"]]
        verdict[name] = {"parent_medians_ms": p, "branch_medians_ms": b, "parent_spread_ms": [min(p), max(p)],
                         "branch_median_ms": float(np.median(b)), "within_parent_spread": bool(min(p) <= float(np.median(b)) <= max(p)),
                         "not_above_parent_spread": bool(float(np.median(b)) <= max(p))}
    json.dump({"repetitions": runs, "verdict": verdict}, open(out, "w"), indent=1)
    print(json.dumps(verdict), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--parent")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "layout_copy_measure.json"))
    a = ap.parse_args()
    if a.parent:
        compare(a.parent, a.repeat, a.calls, a.warmup, a.out)
    else:
        measure(os.path.abspath(a.root), a.calls, a.warmup)


if __name__ == "__main__":
    main()
