"""The SAH build against the middle build ON THE SAME COMMIT: what the trees cost to build and what they do to rendering.

Per workload - the headline frame (03_volume, 1280 wide, 256 spp), BASELINE config 3's substitute (05_head1ss_sub, 1280 wide, 1024 spp),
config 5's frame (03_volume, 3840 wide, 256 spp), all volpathtrace at 64 bounces as bench.py runs them, and one uneven synthetic shape
(tests/bvh_sah_shapes.py: uneven_scene, 1280 wide, 64 spp) - and per quality:
  Msamples/s of volpathtrace through vpt_render (host state in and out), two resident handles in ONE process in interleaved rounds,
  the first --discard rounds dropped, medians;
  the wall time of vpt_scene_rebuild_bvh_quality over every shape and its device span (vpt_scene_update_stats), interleaved likewise;
  the host mirror's rebuild_bvh of the same trees (the plain 45-pass form for SAH; with the flatten);
  node count, depth and the area-weighted cost sum over nodes of (internal ? 1 : num) * area(node) / area(root) of the largest shape's tree.
No threshold is set for any figure.  One JSON line per record, and the list in <out>/bvh_sah_measure.json.

  python profiles/tools/bvh_sah_measure.py [--out DIR (default .)] [--repeat 5] [--discard 2] [--workloads a,b]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vpt_loader  # noqa: E402

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
# name: (scene file or None for the synthetic one, resolution, samples per frame)
WORKLOADS = {"headline": ("03_volume/volume.json", 1280, 256), "config3": ("05_head1ss_sub/head1ss_sub.json", 1280, 1024),
             "config5_frame": ("03_volume/volume.json", 3840, 256), "uneven_synth": (None, 1280, 64)}


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs)}


def tree_figures(nodes):
    size = np.maximum(nodes["bbox_max"].astype(np.float64) - nodes["bbox_min"].astype(np.float64), 0)
    area = 2 * (size[:, 0] * size[:, 1] + size[:, 0] * size[:, 2] + size[:, 1] * size[:, 2])
    weight = np.where(nodes["internal"] != 0, 1, nodes["num"])
    depth, todo = 0, [(0, 0)]
    while todo:
        i, d = todo.pop()
        depth = max(depth, d)
        if nodes[i]["internal"]:
            todo += [(int(nodes[i]["start"]), d + 1), (int(nodes[i]["start"]) + 1, d + 1)]
    return {"nodes": int(len(nodes)), "depth": depth, "cost_sum": float((weight * area).sum() / area[0])}


def largest_tree(h):
    _, shape_nodes = h.bvh_nodes()
    counts = [s["bvh_nodes"] for s in json.loads(h.stats())["shapes"]]
    s = int(np.argmax(counts))
    at = int(np.sum(counts[:s]))
    return shape_nodes[at:at + counts[s]]


def measure(vpt, name, path, resolution, spp, repeat, discard):
    hosts = [vpt.HostScene(path), vpt.HostScene(path)]
    host_ms = [[], []]
    for r in range(repeat + discard):
        for q in (0, 1):
            t0 = time.perf_counter()
            hosts[q].rebuild_bvh("all", quality=q)
            if r >= discard:
                host_ms[q].append((time.perf_counter() - t0) * 1e3)
    devs = [vpt.DeviceScene(hosts[q], 0) for q in (0, 1)]
    p = vpt.PathtraceParams(resolution=resolution, samples=spp, shader="volpathtrace", bounces=64)
    rate, wall, span, launches = [[], []], [[], []], [[], []], [0, 0]
    states = [None, None]
    for r in range(repeat + discard):
        for q in (0, 1):
            st = hosts[q].make_state(p)
            t0 = time.perf_counter()
            devs[q].pathtrace_samples(st, p, spp)
            dt = time.perf_counter() - t0
            states[q] = st
            if r >= discard:
                rate[q].append(st.width * st.height * spp / dt * 1e-6)
    builder = vpt.DeviceScene(vpt.HostScene(path), 0)   # a third handle takes the rebuilds: the rendering handles keep their trees
    abi, keep = vpt.BvhRebuild(range(hosts[0].count("shapes")), True).to_abi()
    for r in range(repeat + discard):
        for q in (0, 1):
            t0 = time.perf_counter()
            vpt._check(vpt.hip.vpt_scene_rebuild_bvh_quality(builder.handle, C.byref(abi), q), "vpt_scene_rebuild_bvh_quality")
            dt = time.perf_counter() - t0
            if r >= discard:
                wall[q].append(dt * 1e3), span[q].append(builder.update_stats()[2])
            launches[q] = builder.update_stats()[0]
    same = builder.get_bvh()[1].tobytes() == hosts[1].bvh_nodes()[1].tobytes()
    rec = {"workload": name, "frame": f"{states[0].width}x{states[0].height} x {spp} spp volpathtrace, 64 bounces, host state in and out",
           "the_device_rebuild_equals_the_mirror": bool(same),
           "hit_pixels_equal": bool(np.array_equal(states[0].hits, states[1].hits))}
    for q, key in ((0, "middle"), (1, "sah")):
        rec[key] = {"msamples_per_s": stat(rate[q]), "rebuild_all_shapes_wall_ms": stat(wall[q]), "rebuild_all_shapes_device_span_ms": stat(span[q]),
                    "launches": launches[q], "host_mirror_rebuild_ms": stat(host_ms[q]), "largest_shape_tree": tree_figures(largest_tree(hosts[q]))}
    rec["sah_over_middle_msamples"] = rec["sah"]["msamples_per_s"]["median"] / rec["middle"]["msamples_per_s"]["median"]
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    a = ap.parse_args()
    vpt = vpt_loader.load()
    records = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.workloads.split(","):
            file, resolution, spp = WORKLOADS[name]
            if file is None:
                import bvh_sah_shapes
                path = bvh_sah_shapes.uneven_scene(tmp)
            else:
                path = os.path.join(SCENES, file)
            records.append(measure(vpt, name, path, resolution, spp, a.repeat, a.discard))
            os.makedirs(a.out, exist_ok=True)
            json.dump(records, open(os.path.join(a.out, "bvh_sah_measure.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
