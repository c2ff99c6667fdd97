"""vpt_scene_rebuild_bvh measured against what the library offered for the same change before it: the host's make_bvh of the same
BVHs, vpt_scene_destroy and vpt_scene_create on the rebuilt descriptor.

Per workload (03_volume, 05_head1ss_sub, 09_curves_synth/dense.json) and kind (the scene BVH only; the largest shape + the scene BVH):
wall-clock time of the vpt_scene_rebuild_bvh call and of the old way (HostScene.rebuild_bvh - make_bvh of the same BVHs and the
flatten - then destroy + create), both in ONE process in interleaved rounds, median and minimum of --repeat rounds after --discard
warm-up rounds; the launches, the bytes of both directions and the device time of the call (vpt_scene_update_stats).  Every round
rebuilds from a changed scene: an instance moves there and back, so neither way meets a tree it has already built.
--frame: the headline frame (03_volume, 1280 wide, volpathtrace, 16 spp through vpt_render) on a deliberately degraded scene - all
instances' frames permuted, then refitted - before and after a rebuild of the scene BVH.  No threshold is set for any time.
One JSON line per record, and the list in <out>/bvh_rebuild_measure.json.

  python profiles/tools/bvh_rebuild_measure.py [--out DIR (default .)] [--repeat 12] [--discard 2] [--workloads a,b] [--frame]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vpt_loader  # noqa: E402

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
WORKLOADS = {"03_volume": "03_volume/volume.json", "05_head1ss_sub": "05_head1ss_sub/head1ss_sub.json", "09_curves_dense": "09_curves_synth/dense.json"}


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "n": len(xs)}


def largest_shape(h):
    return max(range(h.count("shapes")), key=lambda s: len(h.shape_positions(s)))


def measure(vpt, name, scene_file, repeat, discard):
    out = []
    path = os.path.join(SCENES, scene_file)
    for kind in ("scene_only", "largest_shape_and_scene"):
        h = vpt.HostScene(path)
        shapes = [largest_shape(h)] if kind == "largest_shape_and_scene" else []
        A, B = vpt.DeviceScene(vpt.HostScene(path), 0), vpt.DeviceScene(h, 0)
        last = h.count("instances") - 1
        frame0 = h.instance_frame(last)
        new, host_ms, rec, dev_ms = [], [], [], []
        for r in range(repeat + discard):
            f = frame0.copy()
            f[10] += np.float32(0.05 if r % 2 == 0 else 0.0)
            h.set_instance_frame(last, f)
            A.update(h.update_bvh())
            abi, keep = vpt.BvhRebuild(shapes, True).to_abi()
            t0 = time.perf_counter()
            vpt._check(vpt.hip.vpt_scene_rebuild_bvh(A.handle, C.byref(abi)), "vpt_scene_rebuild_bvh")
            t1 = time.perf_counter()
            h.rebuild_bvh(shapes, True)   # make_bvh of the same BVHs on the host, and the flatten
            desc, curves = h.desc, h.curves
            t2 = time.perf_counter()
            vpt.hip.vpt_scene_destroy(B.handle)
            B.handle = vpt._p()
            vpt._check(vpt.hip.vpt_scene_create_curves(desc, curves, 0, C.byref(B.handle)), "vpt_scene_create")
            t3 = time.perf_counter()
            if r >= discard:
                new.append((t1 - t0) * 1e3), host_ms.append((t2 - t1) * 1e3), rec.append((t3 - t2) * 1e3), dev_ms.append(A.update_stats()[2])
        launches, moved, _ = A.update_stats()
        a, b = A.get_bvh()
        c, d = h.bvh_nodes()
        rec_ = {"workload": name, "kind": kind, "shapes": shapes, "rebuild": stat(new), "rebuild_device_span": stat(dev_ms), "launches": launches,
                "bytes_both_directions": moved, "old_host_make_bvh_and_flatten": stat(host_ms), "old_destroy_create": stat(rec),
                "old_sum_median_ms": float(np.median(np.array(host_ms) + np.array(rec))), "same_bytes_as_the_mirror": a.tobytes() == c.tobytes() and b.tobytes() == d.tobytes()}
        rec_["old_over_new_median"] = rec_["old_sum_median_ms"] / rec_["rebuild"]["median_ms"]
        print(json.dumps(rec_), flush=True)
        out.append(rec_)
    return out


def frame(vpt, repeat, discard):
    path = os.path.join(SCENES, WORKLOADS["03_volume"])
    h = vpt.HostScene(path)
    A = vpt.DeviceScene(vpt.HostScene(path), 0)
    n = h.count("instances")
    frames = [h.instance_frame(i) for i in range(n)]
    for i in range(n):   # every instance takes the origin of the next one: the tree keeps the topology made for the old places
        f = frames[i].copy()
        f[9:12] = frames[(i + 1) % n][9:12]
        h.set_instance_frame(i, f)
    A.update_lights(h.update_lights())
    p = vpt.PathtraceParams(resolution=1280, samples=16, shader="volpathtrace", bounces=64)

    def frames_ms():
        ms = []
        for r in range(repeat + discard):
            st = h.make_state(p)
            t0 = time.perf_counter()
            A.pathtrace_samples(st, p, 16)
            t1 = time.perf_counter()
            if r >= discard:
                ms.append((t1 - t0) * 1e3)
        return st, ms

    before_state, before = frames_ms()
    A.rebuild_bvh(h.rebuild_bvh((), True))
    after_state, after = frames_ms()
    rec_ = {"workload": "headline frame 1280x533 x 16 spp, all instance origins permuted then refitted (host state in and out)",
            "refitted_tree": stat(before), "rebuilt_tree": stat(after),
            "same_picture": bool(np.array_equal(before_state.image.view(np.uint32), after_state.image.view(np.uint32)))}
    print(json.dumps(rec_), flush=True)
    return [rec_]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--repeat", type=int, default=12)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--frame", action="store_true")
    a = ap.parse_args()
    vpt = vpt_loader.load()
    records = []
    for name in a.workloads.split(","):
        records += measure(vpt, name, WORKLOADS[name], a.repeat, a.discard)
    if a.frame:
        records += frame(vpt, a.repeat, a.discard)
    os.makedirs(a.out, exist_ok=True)
    json.dump(records, open(os.path.join(a.out, "bvh_rebuild_measure.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
