"""Next-event estimation in the volgrid shader measured, on §29's two scenes and protocol (profiles/tools/volgrid_measure.py:
dense, sparse; 1280 x 533 x 64 spp, bounces 64, albedo 0.8, g 0.6, the brick walk).

Timing: the switch off and on alternating in every round after --discard warm-up rounds, in ONE process; median, minimum and maximum of
--repeat rounds of vpt_last_kernel_ms, tracking steps, shadow flights and shadow steps per sample.  Every timed launch follows the switch,
an edit, so each includes its pilot launch: compare the two cases with each other, not with §29's steady-state figures.

Noise: under the constant sky of the fixture and under a textured sky with a small bright patch (made here), the per-pixel RMS of a
64-spp render, off and on, against a --reference-samples render of the OFF path - the path the tests hold to float64 - and the equal-time
efficiency (rms_off^2 ms_off) / (rms_on^2 ms_on): above 1 the switch wins.  One JSON line per record, the list in
<out>/volgrid_nee_measure.json.

  python profiles/tools/volgrid_nee_measure.py [--out DIR (default profiles)] [--repeat 5] [--discard 2] [--resolution 1280] [--samples 64]
                                               [--reference-samples 16384]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from volgrid_measure import F, FIXTURE, GRIDSDF, ROOT, stat  # noqa: E402
import vpt_loader  # noqa: E402

TEXTURED = os.path.join(os.path.dirname(FIXTURE), "furnace_tex.json")


def scene_with(vpt, voxels, trdepth, patch):
    """volgrid_measure's scene; patch: the textured fixture with a sky of 0.25 and a patch of 64 over 1/128 of the sphere's map"""
    scene = vpt.HostScene(TEXTURED if patch else FIXTURE)
    cam = scene.camera(0)
    cam.aspect = 2.4
    scene.set_camera(0, cam)
    m = scene.material(0)
    m.scattering[:], m.scanisotropy, m.trdepth = (0.8, 0.8, 0.8), 0.6, trdepth
    scene.set_material(0, m)
    scene.update_bvh()
    scene.set_volume(0, voxels, res=1.0 / voxels.shape[2])
    scene.update_volumes()
    if patch:
        sky = np.full((64, 128, 4), 0.25, F)
        sky[12:20, 40:48, :3] = 64.0
        scene.set_texture(0, sky, linear=True)
        scene.set_environment(0, emission_tex=0)
        scene.update_textures()
    return scene


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--resolution", type=int, default=1280)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--reference-samples", type=int, default=16384)
    args = ap.parse_args()
    vpt = vpt_loader.load()
    os.environ["VPT_VOLGRID_NO_BRICKS"] = "0"
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    sdf, res = vpt.HostScene(GRIDSDF).volume(0)
    dense = vpt.density_from_sdf(sdf, 2.0 * res)
    sparse = np.zeros((128, 128, 128), F)
    sparse[48:80, 48:80, 48:80] = 1.0
    params = vpt.PathtraceParams(resolution=args.resolution, shader="volgrid", samples=args.samples, bounces=64)

    def counters(dev):
        nee = dev.volgrid_nee_stats()
        return np.array([dev.volgrid_stats()["steps"], nee["flights"], nee["steps"]], np.float64)

    for name, voxels in (("dense", dense), ("sparse", sparse)):
        scene = scene_with(vpt, voxels, 0.05, False)
        dev = vpt.DeviceScene(scene, 0)
        ms, per = ({c: [] for c in ("off", "on")} for _ in range(2))
        for r in range(args.discard + args.repeat):
            for case in ("off", "on"):
                dev.set_volgrid_nee(case == "on")
                st = scene.make_state(params)
                before = counters(dev)
                dev.pathtrace_samples(st, params, args.samples)
                if r >= args.discard:
                    ms[case].append(dev.last_kernel_ms())
                    per[case].append((counters(dev) - before) / (st.width * st.height * args.samples))
        for case in ("off", "on"):
            k = np.array(per[case])
            emit({"what": "timing", "scene": name, "grid": list(voxels.shape), "nee": case, "width": st.width, "height": st.height, "samples": args.samples,
                  "bounces": 64, "kernel_ms": stat(ms[case]), "tracking_steps_per_sample": stat(k[:, 0]), "shadow_flights_per_sample": stat(k[:, 1]),
                  "shadow_steps_per_sample": stat(k[:, 2]), "note": "every launch follows the switch and includes its pilot"})

    big = vpt.PathtraceParams(resolution=args.resolution, shader="volgrid", samples=args.reference_samples, bounces=64)
    for sky in ("constant", "patch"):
        for name, voxels in (("dense", dense), ("sparse", sparse)):
            scene = scene_with(vpt, voxels, 0.05, sky == "patch")
            dev = vpt.DeviceScene(scene, 0)
            ref = scene.make_state(big)
            dev.pathtrace_samples(ref, big, args.reference_samples)
            want = ref.image[..., :3].astype(np.float64) / args.reference_samples
            rms, ms = {}, {}
            for case in ("off", "on"):
                dev.set_volgrid_nee(case == "on")
                times = []
                for _ in range(3):   # the same streams, the same picture: three times of it
                    st = scene.make_state(params)
                    dev.pathtrace_samples(st, params, args.samples)
                    times.append(dev.last_kernel_ms())
                rms[case] = float(np.sqrt(np.mean((st.image[..., :3].astype(np.float64) / args.samples - want) ** 2)))
                ms[case] = stat(times)
            dev.set_volgrid_nee(False)
            emit({"what": "noise", "sky": sky, "scene": name, "width": st.width, "height": st.height, "samples": args.samples,
                  "reference_samples_off_path": args.reference_samples, "mean_radiance": float(want.mean()), "rms": rms, "kernel_ms": ms,
                  "equal_time_efficiency_on_over_off": (rms["off"] ** 2 * ms["off"]["median"]) / (rms["on"] ** 2 * ms["on"]["median"])})
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "volgrid_nee_measure.json"), "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
