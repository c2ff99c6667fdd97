"""vpt_bake_sdf measured: tests/golden/scenes/03_volume/shapes/bunny.ply baked into 64^3 and 128^3 grids fitted around it.

Per grid size, in ONE process: the device time of the bake kernel (vpt_bake_stats.device_ms: HIP events around the launch) and the
wall-clock time of the whole vpt_bake_sdf call (host clock; the call is synchronous: validation, feature normals, BVH build, uploads,
kernel, download), for the BVH form and for the brute form (VPT_BAKE_BRUTE=1, read per call) in interleaved rounds: median and minimum
of --repeat rounds after --discard warm-up rounds.  The two forms' voxels are compared bit for bit at the measured size.  The host
mirror (bake_sdf with device None: 16 CPU threads, every triangle per voxel) is the baseline - the capability is new, so there is no
earlier time to compare with; it is timed once per size in --mirror-res (default: 64 only; it takes minutes) and compared bit for bit
too.  One JSON line per record, and the list in <out>/bake_sdf_measure.json.

  python profiles/tools/bake_sdf_measure.py [--out DIR (default .)] [--res 64,128] [--mirror-res 64] [--repeat 5] [--discard 1] [--brute-repeat 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import vpt_loader  # noqa: E402

SHAPE = os.path.join(ROOT, "tests", "golden", "scenes", "03_volume", "shapes", "bunny.ply")


def load_shape(vpt, out_dir):
    """the shape through the host loader: a one-shape scene written beside the results"""
    path = os.path.join(out_dir, "bake_sdf_measure_scene.json")
    with open(path, "w") as f:
        json.dump({"asset": {"version": "4.2"}, "cameras": [{"name": "default", "frame": [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1]}],
                   "materials": [{"name": "m"}], "shapes": [{"name": "bunny", "uri": os.path.relpath(SHAPE, out_dir)}],
                   "instances": [{"name": "bunny", "shape": 0, "material": 0}]}, f)
    arrays = vpt.HostScene(path).shape_arrays(0)
    return arrays["positions"], vpt.bake_triangles(arrays["quads"] if len(arrays["quads"]) else arrays["triangles"])


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--res", default="64,128")
    ap.add_argument("--mirror-res", default="64")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--discard", type=int, default=1)
    ap.add_argument("--brute-repeat", type=int, default=3)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    vpt = vpt_loader.load()
    if vpt.device_count() < 1:
        raise SystemExit("bake_sdf_measure needs a GPU: a time taken elsewhere says nothing")
    positions, triangles = load_shape(vpt, a.out)
    mirror_res = [int(r) for r in a.mirror_res.split(",") if r]
    records = []
    for res in [int(r) for r in a.res.split(",")]:
        times = {"bvh": {"device": [], "wall": []}, "brute": {"device": [], "wall": []}}
        voxels, stats = {}, {}
        for r in range(a.discard + a.repeat):
            for form in ("bvh", "brute"):
                if form == "brute" and r >= a.discard + a.brute_repeat:
                    continue
                os.environ.pop("VPT_BAKE_BRUTE", None)
                if form == "brute":
                    os.environ["VPT_BAKE_BRUTE"] = "1"
                t0 = time.perf_counter()
                baked = vpt.bake_sdf(positions, triangles, res, device=0)
                wall = (time.perf_counter() - t0) * 1e3
                voxels[form], stats[form] = baked.voxels, baked.stats
                if r >= a.discard:
                    times[form]["device"].append(baked.stats["device_ms"]), times[form]["wall"].append(wall)
        os.environ.pop("VPT_BAKE_BRUTE", None)
        rec = {"shape": "bunny.ply", "triangles": int(len(triangles)), "dropped": stats["bvh"]["dropped_triangles"], "res": res,
               "bvh_nodes": stats["bvh"]["bvh_nodes"], "bvh_depth": stats["bvh"]["bvh_depth"],
               "bvh_device": stat(times["bvh"]["device"]), "bvh_wall": stat(times["bvh"]["wall"]),
               "brute_device": stat(times["brute"]["device"]), "brute_wall": stat(times["brute"]["wall"]),
               "bvh_equals_brute": bool(np.array_equal(voxels["bvh"].view(np.uint32), voxels["brute"].view(np.uint32))),
               "inside_voxels": int((voxels["bvh"] < 0).sum())}
        if res in mirror_res:
            print(f"res {res}: device done, host mirror running ...", flush=True)
            t0 = time.perf_counter()
            mirror = vpt.bake_sdf(positions, triangles, res, device=None)
            rec["mirror_wall_ms_16_threads"] = (time.perf_counter() - t0) * 1e3
            rec["device_equals_mirror"] = bool(np.array_equal(voxels["bvh"].view(np.uint32), mirror.voxels.view(np.uint32)))
        print(json.dumps(rec), flush=True)
        records.append(rec)
        with open(os.path.join(a.out, "bake_sdf_measure.json"), "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
