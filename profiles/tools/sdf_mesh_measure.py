"""vpt_scene_mesh_volume measured against the route to a mesh that existed before it.

Subjects: the 96^3 and 64^3 grids of 06_gridsdf_full (volumes 0 and 1) where they lie in the resident pool, a 256^3 bake of
03_volume's bunny put into volume 0 of a second handle (baked by vpt_bake_sdf, handed over by vpt_scene_update_volumes), and an 8^3 region
of the 64^3 grid: next to no work, so what remains is the fixed cost of one call.  Per subject, in ONE process, every side in every round
after --discard warm-up rounds; median, minimum and maximum of --repeat rounds:
 - mesh: the wall-clock time of ONE vpt_scene_mesh_volume call into arrays of a capacity the caller keeps (host clock; the call returns
   with the device idle and the mesh on the host), its device time (vpt_sdf_mesh_stats.device_ms: events around the counting passes
   and around the emitting passes), the counting call alone (outputs NULL: classify and scan), and DeviceScene.mesh_volume as Python
   calls it (count, then fill: the counting passes run twice);
 - old route: vpt_scene_get_voxels (the whole volume comes back over PCIe) and a host mesher.  No mesher shipped with the project before
   this one, so the host mirror of the rule (mesh_sdf with device None: one CPU thread, serial loops) STANDS IN for whatever mesher a
   caller would have brought; each part timed, and their sum.
The bytes that cross PCIe on each side are computed from the counts.  After the last round the two routes' meshes are compared bit for
bit.  One JSON line per record, and the list in <out>/sdf_mesh_measure.json.

  python profiles/tools/sdf_mesh_measure.py [--out DIR (default .)] [--repeat 7] [--discard 2] [--bake 256]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vpt_loader  # noqa: E402
from bake_sdf_measure import load_shape  # noqa: E402

SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "06_gridsdf_full", "gridsdf_full.json")
F = np.float32


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "max_ms": float(np.max(xs)), "n": len(xs)}


def one_call(vpt, dev, volume, region, out):
    """vpt_scene_mesh_volume into the arrays of `out` (None: the counting call); the stats it left"""
    st = vpt.VptSdfMeshStats()
    box = None if region is None else vpt.VptSdfMeshRegion((C.c_int32 * 3)(*region[0]), (C.c_int32 * 3)(*region[1]))
    args = (None, None, 0, None, 0) if out is None else (out[0].ctypes.data, out[1].ctypes.data, len(out[0]), out[2].ctypes.data, len(out[2]))
    vpt._check(vpt.hip.vpt_scene_mesh_volume(dev.handle, volume, None, C.byref(box) if box else None, *args, C.byref(st)), "vpt_scene_mesh_volume")
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--bake", type=int, default=256)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    vpt = vpt_loader.load()
    if vpt.device_count() < 1:
        raise SystemExit("sdf_mesh_measure needs a GPU: a time taken elsewhere says nothing")
    records = []

    def save(rec):
        print(json.dumps(rec), flush=True)
        records.append(rec)
        with open(os.path.join(a.out, "sdf_mesh_measure.json"), "w") as f:
            json.dump(records, f, indent=1)

    host = vpt.HostScene(SCENE)
    dev = vpt.DeviceScene(host, 0)
    # the bake: on the device, then into volume 0 of a handle of its own (the host scene gets the voxels, not a bake of its own)
    positions, triangles = load_shape(vpt, a.out)
    baked = vpt.bake_sdf(positions, triangles, a.bake, device=0)
    big_host = vpt.HostScene(SCENE)
    big_host.set_volume(0, baked.voxels, res=baked.res)
    big = vpt.DeviceScene(vpt.HostScene(SCENE), 0)
    big.update_volumes(big_host.update_volumes())
    subjects = [("sackboy_96", dev, host, 0, None), ("bunny_64", dev, host, 1, None), (f"bunny_bake_{a.bake}", big, big_host, 0, None),
                ("fixed_cost_8^3_region", dev, host, 1, ((28, 28, 28), (8, 8, 8)))]
    for name, d, h, volume, region in subjects:
        counts = one_call(vpt, d, volume, region, None)
        nv, nq = counts.num_vertices, counts.num_quads
        out = (np.zeros((max(1, nv), 3), F), np.zeros((max(1, nv), 3), F), np.zeros((max(1, nq), 4), np.int32))
        whd = h.volume(volume)[0].shape[::-1]
        keys = ("wall", "device", "count_wall", "count_device", "python_wall", "old_get", "old_host", "old_route")
        t = {k: [] for k in keys}
        mirror = None
        for r in range(a.discard + a.repeat):
            st, wall = timed(lambda: one_call(vpt, d, volume, region, out))
            cst, count_wall = timed(lambda: one_call(vpt, d, volume, region, None))
            _, python_wall = timed(lambda: d.mesh_volume(volume, region=region))
            voxels, get_ms = timed(lambda: d.get_voxels(volume))
            mirror, host_ms = timed(lambda: h.mesh_volume(volume, region=region))   # (h.volume copies the grid first: part of any host route that starts from the scene's copy)
            if r >= a.discard:
                t["wall"].append(wall), t["device"].append(st.device_ms), t["count_wall"].append(count_wall), t["count_device"].append(cst.device_ms)
                t["python_wall"].append(python_wall), t["old_get"].append(get_ms), t["old_host"].append(host_ms), t["old_route"].append(get_ms + host_ms)
        got = {"positions": out[0][:nv], "normals": out[1][:nv], "quads": out[2][:nq]}
        same = all(mirror[k] is None and len(got[k]) == 0 or mirror[k] is not None and got[k].tobytes() == mirror[k].tobytes() for k in got)
        rec = {"subject": name, "whd": list(whd), "region": None if region is None else [list(region[0]), list(region[1])],
               "voxels": int(np.prod(whd if region is None else region[1])), "vertices": nv, "quads": nq, "launches": st.launches,
               "mesh_bytes_down": 24 * nv + 16 * nq + 16, "mesh_bytes_up": 0, "old_bytes_down": 4 * int(np.prod(whd)),
               "mesh_wall": stat(t["wall"]), "mesh_device": stat(t["device"]), "count_only_wall": stat(t["count_wall"]),
               "count_only_device": stat(t["count_device"]), "python_two_calls_wall": stat(t["python_wall"]),
               "old_get_voxels": stat(t["old_get"]), "old_host_mesher_stand_in_1_thread": stat(t["old_host"]), "old_route_wall": stat(t["old_route"]),
               "ratio_old_over_mesh": float(np.median(t["old_route"]) / np.median(t["wall"])),
               "ratio_get_voxels_alone_over_mesh": float(np.median(t["old_get"]) / np.median(t["wall"])),
               "device_equals_mirror": bool(same)}
        save(rec)


if __name__ == "__main__":
    main()
