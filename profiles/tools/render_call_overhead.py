#!/usr/bin/env python3
"""Host-side cost of a vpt_render_device call: wall time of N consecutive calls of 1 sample each, ended by a synchronise.
  render_call_overhead.py [calls [scene file [resolution]]]   -> one JSON line: calls, wall ms, microseconds per call
The calls are short launches in a row on one layout (wave order, cost average and sort every time), so what the host does
around a launch - the launch schedule's bookkeeping - shows up here and not in the throughput of a long render."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vpt_loader

vpt = vpt_loader.load()
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200
scene_file = sys.argv[2] if len(sys.argv) > 2 else "03_volume/volume.json"
res = int(sys.argv[3]) if len(sys.argv) > 3 else 320
scene = vpt.HostScene(os.path.join(ROOT, "tests", "golden", "scenes", scene_file))
dev = vpt.DeviceScene(scene, 0)
p = vpt.PathtraceParams(resolution=res, samples=1 << 20, shader="volpathtrace", bounces=64)
host = scene.make_state(p)
lay = vpt.VptLayout(host.width, host.height, 8, 8, 0, 1)
slots = vpt.layout_slots(lay)
d = torch.device("cuda", 0)
img = torch.zeros((slots, 4), dtype=torch.float32, device=d)
hit = torch.zeros((slots,), dtype=torch.int32, device=d)
rng = torch.zeros((slots, 2), dtype=torch.int64, device=d)
vpt.state_upload(lay, host, img.data_ptr(), hit.data_ptr(), rng.data_ptr())
for _ in range(20):   # warm-up: the schedule's buffers and the costs of this layout are in place
    dev.render_device(p, lay, 1, img.data_ptr(), hit.data_ptr(), rng.data_ptr(), 0)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(calls):
    dev.render_device(p, lay, 1, img.data_ptr(), hit.data_ptr(), rng.data_ptr(), 0)
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) * 1e3
print(json.dumps({"calls": calls, "scene": scene_file, "resolution": res, "wall_ms": round(ms, 3), "us_per_call": round(ms * 1e3 / calls, 2)}))
