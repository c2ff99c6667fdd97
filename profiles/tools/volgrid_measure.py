"""The volgrid shader (K3) measured: Msamples/s and vpt_last_kernel_ms at 1280 x 533 x 64 spp, bounces 64, albedo 0.8,
g 0.6, on
 - dense:  the 96^3 grid of 06_gridsdf_full (volume 0) turned into a cloud by density_from_sdf, in the fixture scene's box;
 - sparse: the fixture's sparse grid scaled to 128^3 (the central 32-node block 1, everything else 0);
each with the brick walk and with one majorant per volume (VPT_VOLGRID_NO_BRICKS=1, read per launch), the two alternating in every round
after --discard warm-up rounds, in ONE process; median, minimum and maximum of --repeat rounds, and the mean tracking steps per sample
(vpt_scene_volgrid_stats).  Then the cost of a majorant rebuild after a one-stamp sculpt of the 96^3 grid - the wall-clock time of the
query that rebuilds the tables (vpt_scene_get_volgrid_majorants: the reduction and 7 KiB back) - against the render launch that follows.
One JSON line per record, and the list in <out>/volgrid_measure.json.

  python profiles/tools/volgrid_measure.py [--out DIR (default profiles)] [--repeat 5] [--discard 2] [--resolution 1280] [--samples 64]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import vpt_loader  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "scenes", "10_volgrid_synth", "volgrid.json")
GRIDSDF = os.path.join(ROOT, "tests", "golden", "scenes", "06_gridsdf_full", "gridsdf_full.json")
F = np.float32


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs)}


def scene_with(vpt, voxels, trdepth):
    scene = vpt.HostScene(FIXTURE)
    cam = scene.camera(0)
    cam.aspect = 2.4
    scene.set_camera(0, cam)
    m = scene.material(0)
    m.scattering[:], m.scanisotropy, m.trdepth = (0.8, 0.8, 0.8), 0.6, trdepth
    scene.set_material(0, m)
    scene.update_bvh()
    w = voxels.shape[2]
    scene.set_volume(0, voxels, res=1.0 / w)
    scene.update_volumes()
    return scene


def main():
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
    dense = vpt.density_from_sdf(sdf, 2.0 * res)   # the grid's distances are in its voxel space, a voxel about res wide: a soft edge two voxels wide
    sparse = np.zeros((128, 128, 128), F)
    sparse[48:80, 48:80, 48:80] = 1.0
    params = vpt.PathtraceParams(resolution=args.resolution, shader="volgrid", samples=args.samples, bounces=64)
    for name, voxels, trdepth in (("dense", dense, 0.05), ("sparse", sparse, 0.05)):
        scene = scene_with(vpt, voxels, trdepth)
        dev = vpt.DeviceScene(scene, 0)
        ms = {"bricks": [], "one_majorant": []}
        steps = {"bricks": [], "one_majorant": []}
        pixels = 0
        for r in range(args.discard + args.repeat):
            for mode in ("bricks", "one_majorant"):
                os.environ["VPT_VOLGRID_NO_BRICKS"] = "1" if mode == "one_majorant" else "0"
                st = scene.make_state(params)
                before = dev.volgrid_stats()["steps"]
                dev.pathtrace_samples(st, params, args.samples)
                pixels = st.width * st.height
                if r >= args.discard:
                    ms[mode].append(dev.last_kernel_ms())
                    steps[mode].append((dev.volgrid_stats()["steps"] - before) / (pixels * args.samples))
        os.environ["VPT_VOLGRID_NO_BRICKS"] = "0"
        for mode in ms:
            emit({"what": "render", "scene": name, "grid": list(voxels.shape), "walk": mode, "width": st.width, "height": st.height, "samples": args.samples,
                  "bounces": 64, "kernel_ms": stat(ms[mode]), "msamples_per_s": stat([pixels * args.samples / t / 1e3 for t in ms[mode]]),
                  "tracking_steps_per_sample": stat(steps[mode]), "nonzero_bricks": int(np.count_nonzero(scene.volgrid_majorants(0))),
                  "bricks": int(scene.volgrid_majorants(0).size)})
        if name == "dense":   # the rebuild after a one-stamp sculpt of the 96^3 grid, against the launch that follows
            brush = vpt.VptSdf(type=vpt.SDF_TYPES.index("sphere"))
            brush.frame.x[:], brush.frame.y[:], brush.frame.z[:], brush.frame.o[:] = (1, 0, 0), (0, 1, 0), (0, 0, 1), (-0.5, -0.5, -0.5)
            brush.p[0] = 0.06
            rebuild, launch_wall, launch_kernel = [], [], []
            for r in range(args.discard + args.repeat):
                scene.sculpt_volume(0, [vpt.Stamp(brush, 1, 0.0)], region=((40, 40, 40), (16, 16, 16)))
                dev.sculpt_volumes(scene.update_sculpts())
                t0 = time.perf_counter()
                dev.volgrid_majorants(0)
                t1 = time.perf_counter()
                st = scene.make_state(params)
                t2 = time.perf_counter()
                dev.pathtrace_samples(st, params, args.samples)
                t3 = time.perf_counter()
                if r >= args.discard:
                    rebuild.append((t1 - t0) * 1e3), launch_wall.append((t3 - t2) * 1e3), launch_kernel.append(dev.last_kernel_ms())
            emit({"what": "majorant rebuild after a one-stamp sculpt", "grid": list(voxels.shape), "rebuild_and_readback_wall_ms": stat(rebuild),
                  "render_call_wall_ms": stat(launch_wall), "render_kernel_ms": stat(launch_kernel), "table_builds": dev.volgrid_stats()["table_builds"]})
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "volgrid_measure.json"), "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
