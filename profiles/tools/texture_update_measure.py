"""vpt_scene_update_textures measured against the only way there was to dim or swap a sky or repaint a texture before it: host
make_lights + flatten (HostScene.update_textures) + vpt_scene_destroy + vpt_scene_create on the edited descriptor.

Four cases of tests/texture_edits.py on 03_volume, each with its inverse so that every round applies a real change: the sky's emission
0.5 <-> 0.25 (sky_dim: nothing but the environment's entry), a rectangle of the 2048 x 1024 sky times 4 and back (sky_repaint: in
place, the 2 M-entry chain), the sky swapped for the 1000 x 500 texture2.hdr and back (sky_swap_hdri: a resize in both directions, the
float pool grows by the new texels every time - the rounds of this case are fewer for that), the floor's bytes repainted and back
(floor_repaint: no light reads them).  Per case and direction: wall-clock time (host clock; both calls return with the device idle) of
the vpt_scene_update_textures call and of make_lights + flatten + destroy + create, in ONE process in interleaved rounds, median and
minimum of --repeat rounds after --discard warm-up rounds; launches, bytes and device time of the update (vpt_scene_update_stats).
The old way's figure adds the host's make_lights + flatten to destroy + create; the update's is the call alone.  That is the comparison
for a caller who fills a vpt_texture_edit from its own data.  A caller who goes through HostScene.update_textures() pays the host's
make_lights + flatten on the new way as well: ratio_with_host_mirror has it on both sides.
One JSON line per record, and the list in <out>/texture_update_measure.json.

  python profiles/tools/texture_update_measure.py [--out DIR (default .)] [--repeat 8] [--discard 2] [--workloads sky_dim,...]"""
import argparse
import ctypes as C
import json
import os
import pathlib
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import texture_edits as T  # noqa: E402
import vpt_loader  # noqa: E402


def workloads(vpt, work):
    """name -> (recomputed CDF entries per direction (forward, back), function(host scene, forward: bool))"""
    keep = {}

    def dim(h, fwd):
        h.set_environment(0, emission=(0.25, 0.25, 0.25) if fwd else (0.5, 0.5, 0.5))

    def repaint(h, fwd):
        sky = keep.setdefault("sky", h.texture(T.SKY)[0])
        if fwd:
            T.repaint_sky(h, work)
        else:
            h.set_texture(T.SKY, sky)

    def swap(h, fwd):
        sky = keep.setdefault("sky", h.texture(T.SKY)[0])
        other = keep.setdefault("other", T.file_texels(vpt, work, "shared_textures/texture2.hdr")[0])
        h.set_texture(T.SKY, other if fwd else sky)

    def floor(h, fwd):
        was = keep.setdefault("floor", h.texture(T.FLOOR)[0])
        if fwd:
            T.repaint_floor(h, work)
        else:
            h.set_texture(T.FLOOR, was)

    return {"sky_dim": ((0, 0), dim), "sky_repaint": ((2048 * 1024, 2048 * 1024), repaint), "sky_swap_hdri": ((1000 * 500, 2048 * 1024), swap),
            "floor_repaint": ((0, 0), floor)}


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "n": len(xs)}


def measure(vpt, work, name, repeat, discard):
    entries, apply = workloads(vpt, work)[name]
    path = os.path.join(T.SCENES, T.S03)
    h = vpt.HostScene(path)
    A, B = vpt.DeviceScene(vpt.HostScene(path), 0), vpt.DeviceScene(h, 0)
    out = []
    times = {d: {"update": [], "host": [], "recreate": [], "device": [], "stats": None} for d in (True, False)}
    for r in range(2 * (repeat + discard)):
        fwd = r % 2 == 0
        apply(h, fwd)
        t0 = time.perf_counter()
        edit = h.update_textures()   # make_lights + flatten: the old way needs all of it, the new way the edit alone
        t1 = time.perf_counter()
        abi, keep = edit.to_abi()
        t2 = time.perf_counter()
        vpt._check(vpt.hip.vpt_scene_update_textures(A.handle, C.byref(abi)), "vpt_scene_update_textures")
        t3 = time.perf_counter()
        desc, curves = h.desc, h.curves
        t4 = time.perf_counter()
        vpt.hip.vpt_scene_destroy(B.handle)
        B.handle = vpt._p()
        vpt._check(vpt.hip.vpt_scene_create_curves(desc, curves, 0, C.byref(B.handle)), "vpt_scene_create")
        t5 = time.perf_counter()
        assert A.light_tables_hash() == B.light_tables_hash()
        if r >= 2 * discard:
            t = times[fwd]
            t["update"].append((t3 - t2) * 1e3), t["host"].append((t1 - t0) * 1e3), t["recreate"].append((t5 - t4) * 1e3)
            t["stats"] = A.update_stats()
            t["device"].append(t["stats"][2])
    for fwd in (True, False):
        t = times[fwd]
        rec = {"workload": name, "scene": T.S03, "direction": "forward" if fwd else "back", "recomputed_cdf_entries": entries[0 if fwd else 1],
               "update_textures": stat(t["update"]), "update_device": stat(t["device"]), "host_make_lights_and_flatten": stat(t["host"]),
               "destroy_and_create": stat(t["recreate"]), "launches": t["stats"][0], "bytes": t["stats"][1]}
        rec["old_way_median_ms"] = rec["host_make_lights_and_flatten"]["median_ms"] + rec["destroy_and_create"]["median_ms"]
        rec["ratio_median"] = rec["old_way_median_ms"] / rec["update_textures"]["median_ms"]
        rec["ratio_with_host_mirror"] = rec["old_way_median_ms"] / (rec["host_make_lights_and_flatten"]["median_ms"] + rec["update_textures"]["median_ms"])
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--workloads", default="sky_dim,sky_repaint,sky_swap_hdri,floor_repaint")
    a = ap.parse_args()
    vpt = vpt_loader.load()
    records = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.workloads.split(","):
            repeat = min(a.repeat, 4) if name == "sky_swap_hdri" else a.repeat   # its float pool grows with every round
            records += measure(vpt, pathlib.Path(tmp), name, repeat, min(a.discard, 1) if name == "sky_swap_hdri" else a.discard)
    os.makedirs(a.out, exist_ok=True)
    json.dump(records, open(os.path.join(a.out, "texture_update_measure.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
