"""vpt_scene_update measured against what the library offered for the same change before it: vpt_scene_destroy + vpt_scene_create on
the edited descriptor.

Per workload (03_volume, 05_head1ss_sub, 09_curves_synth/dense.json) and edit kind (camera only; one instance; all instances; all
vertices of the largest shape that is no light's): wall-clock time of the vpt_scene_update call and of destroy + create, both in ONE
process in interleaved rounds (update, re-create, update, ...), median and minimum of --repeat rounds after --discard warm-up rounds;
the device time between the first and the last launch of the update, the number of its launches and the bytes it sent
(vpt_scene_update_stats); for the vertex edit the bytes the device rewrites over bench.py's HBM figure, as the bound the device time is
read against; and the same update with a launch per level throughout (VPT_UPDATE_NO_FUSE=1 in a child process) beside the default, which
finishes the narrow top levels in one launch.  Every round applies a real change: the edit and its inverse take turns.
--frame: the headline frame (03_volume, 1280 wide, volpathtrace, 16 spp through vpt_render) after a camera update against after a
re-creation.  One JSON line per record, and the list in <out>/scene_update_measure.json.

  python profiles/tools/scene_update_measure.py [--out DIR (default .)] [--repeat 24] [--discard 4] [--workloads a,b] [--frame]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scene_edits as E  # noqa: E402
import vpt_loader  # noqa: E402

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
WORKLOADS = {"03_volume": "03_volume/volume.json", "05_head1ss_sub": "05_head1ss_sub/head1ss_sub.json", "09_curves_dense": "09_curves_synth/dense.json"}
HBM_BYTES_PER_S = 8.0e12   # bench.py's roofline figure


def largest_free_shape(h):
    lit = E.lit_shapes(h)
    return max((s for s in range(h.count("shapes")) if s not in lit), key=lambda s: len(h.shape_positions(s)))


def edit_kinds(h):
    """name -> function(host scene, forward: bool) applying the edit or its inverse through the setters"""
    n = h.count("instances")
    big = largest_free_shape(h)
    p0, c0 = h.shape_positions(big), h.camera(0)
    frames = [h.instance_frame(i) for i in range(n)]

    def camera(h, fwd):
        c = h.camera(0)
        c.lens = float(np.float32(c0.lens) * np.float32(1.1 if fwd else 1.0))
        h.set_camera(0, c)

    def moved(i, fwd):
        f = frames[i].copy()
        f[9] += np.float32(0.01 if fwd else 0.0)
        return f

    return {"camera": camera,
            "one_instance": lambda h, fwd: h.set_instance_frame(n - 1, moved(n - 1, fwd)),
            "all_instances": lambda h, fwd: [h.set_instance_frame(i, moved(i, fwd)) for i in range(n)],
            "all_vertices_of_largest_shape": lambda h, fwd: h.set_shape_positions(big, E.nudge(p0) if fwd else p0)}


def vertex_edit_bytes(h, dev):
    """bytes the device rewrites for the vertex edit of the largest shape: vertices, leaf records in every form, nodes, quad nodes"""
    big = largest_free_shape(h)
    stats = json.loads(h.stats())["shapes"][big]
    elems = max(stats["triangles"], stats["quads"], stats.get("points", 0), stats.get("lines", 0))
    leaf, attr = dev.record_bytes()
    general = elems * (64 + (64 if len(h.shape_normals(big)) else 0))
    compact = elems * (leaf + (48 if len(h.shape_normals(big)) else 0)) if leaf == 48 else 0
    return stats["positions"] * 16 + general + compact + stats["bvh_nodes"] * 32 + (stats["bvh_nodes"] // 4) * 96


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "n": len(xs)}


def measure(vpt, name, scene_file, repeat, discard):
    out = []
    path = os.path.join(SCENES, scene_file)
    for kind in edit_kinds(vpt.HostScene(path)):
        h = vpt.HostScene(path)
        apply = edit_kinds(h)[kind]
        A = vpt.DeviceScene(vpt.HostScene(path), 0)
        B = vpt.DeviceScene(h, 0)
        upd, rec, dev_ms = [], [], []
        for r in range(repeat + discard):
            apply(h, r % 2 == 0)
            edit = h.update_bvh()
            abi, keep = edit.to_abi()
            t0 = time.perf_counter()
            vpt._check(vpt.hip.vpt_scene_update(A.handle, C.byref(abi)), "vpt_scene_update")
            t1 = time.perf_counter()
            desc, curves = h.desc, h.curves
            t2 = time.perf_counter()
            vpt.hip.vpt_scene_destroy(B.handle)
            B.handle = vpt._p()
            vpt._check(vpt.hip.vpt_scene_create_curves(desc, curves, 0, C.byref(B.handle)), "vpt_scene_create")
            t3 = time.perf_counter()
            if r >= discard:
                upd.append((t1 - t0) * 1e3), rec.append((t3 - t2) * 1e3), dev_ms.append(A.update_stats()[2])
        launches, sent, _ = A.update_stats()
        rec_ = {"workload": name, "edit": kind, "update": stat(upd), "recreate": stat(rec), "update_device": stat(dev_ms), "launches": launches,
                "bytes_sent": sent, "fused_top_levels": not os.environ.get("VPT_UPDATE_NO_FUSE")}
        rec_["speedup_median"] = rec_["recreate"]["median_ms"] / rec_["update"]["median_ms"]
        if kind == "all_vertices_of_largest_shape":
            b = vertex_edit_bytes(h, A)
            rec_["bytes_rewritten"], rec_["hbm_bound_ms"] = b, b / HBM_BYTES_PER_S * 1e3
        print(json.dumps(rec_), flush=True)
        out.append(rec_)
    return out


def frame(vpt, repeat, discard):
    path = os.path.join(SCENES, WORKLOADS["03_volume"])
    h = vpt.HostScene(path)
    camera = edit_kinds(h)["camera"]
    A, B = vpt.DeviceScene(vpt.HostScene(path), 0), vpt.DeviceScene(h, 0)
    p = vpt.PathtraceParams(resolution=1280, samples=16, shader="volpathtrace", bounces=64)
    upd, rec = [], []
    for r in range(repeat + discard):
        camera(h, r % 2 == 0)
        edit = h.update_bvh()
        st = h.make_state(p)
        t0 = time.perf_counter()
        A.update(edit)
        A.pathtrace_samples(st, p, 16)
        t1 = time.perf_counter()
        st = h.make_state(p)
        t2 = time.perf_counter()
        B.close()
        B = vpt.DeviceScene(h, 0)
        B.pathtrace_samples(st, p, 16)
        t3 = time.perf_counter()
        if r >= discard:
            upd.append((t1 - t0) * 1e3), rec.append((t3 - t2) * 1e3)
    rec_ = {"workload": "headline frame 1280x533 x 16 spp, camera edit per frame (host state in and out)", "update_then_render": stat(upd),
            "recreate_then_render": stat(rec)}
    print(json.dumps(rec_), flush=True)
    return [rec_]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--repeat", type=int, default=24)
    ap.add_argument("--discard", type=int, default=4)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--frame", action="store_true")
    ap.add_argument("--child", action="store_true", help="internal: print the records, write no file")
    a = ap.parse_args()
    vpt = vpt_loader.load()
    records = []
    for name in a.workloads.split(","):
        records += measure(vpt, name, WORKLOADS[name], a.repeat, a.discard)
    if a.frame:
        records += frame(vpt, a.repeat, a.discard)
    if a.child:
        return
    # the same with a launch per level throughout: in a child process, so that the two do not share a handle's state
    env = dict(os.environ, VPT_UPDATE_NO_FUSE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--repeat", str(a.repeat), "--discard", str(a.discard), "--workloads",
                        a.workloads], env=env, capture_output=True, text=True, timeout=900)
    records += [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    os.makedirs(a.out, exist_ok=True)
    json.dump(records, open(os.path.join(a.out, "scene_update_measure.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
