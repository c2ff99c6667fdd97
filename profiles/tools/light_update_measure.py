"""vpt_scene_update_lights measured against the only way there was to switch a lamp or deform an emitter before it: host make_lights +
flatten (HostScene.update_lights) + vpt_scene_destroy + vpt_scene_create on the edited descriptor.

Three cases of tests/light_edits.py: jade switched on and off (03_volume: a 6 144-quad light comes and goes), material1 switched on
and off (05_head1ss_sub: 144 046 triangles), arealight1's four vertices stretched and back (03_volume).  Per case: wall-clock time
(host clock; both calls return with the device idle) of the vpt_scene_update_lights call and of make_lights + flatten + destroy +
create, both in ONE process in interleaved rounds, median and minimum of --repeat rounds after --discard warm-up rounds; the two parts
of the old way apart; launches and bytes of the update (vpt_scene_update_stats).  Every round applies a real change: the edit and its
inverse take turns, and the two directions are recorded apart (switching ON recomputes a CDF, switching OFF only moves the others).
The same with the plain running sum (VPT_LIGHTS_PLAIN=1, in a child process).  One JSON line per record, and the list in
<out>/light_update_measure.json.  The time of the running-sum kernel itself comes from a separate `rocprofv3 --kernel-trace --stats`
run of this script (--workloads head --repeat 8), in both forms.

  python profiles/tools/light_update_measure.py [--out DIR (default .)] [--repeat 8] [--discard 2] [--workloads jade,head,arealight1]"""
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
import light_edits as L  # noqa: E402
import scene_edits as E  # noqa: E402
import vpt_loader  # noqa: E402


def workloads():
    """name -> (scene file, elements of the light concerned, function(host scene, forward: bool))"""
    def toggle(scene_file, name):
        return lambda h, fwd: L.emit(h, L.index_of(scene_file, "materials", name), L.WARM if fwd else (0.0, 0.0, 0.0))

    def stretch(h, fwd, keep={}):
        s = L.index_of(L.S03, "shapes", "arealight1")
        p0 = keep.setdefault("p0", h.shape_positions(s))
        h.set_shape_positions(s, E.nudge(L.stretch(p0)) if fwd else p0)

    return {"jade": (L.S03, 6144, toggle(L.S03, "jade")), "head": (L.HEAD, 144046, toggle(L.HEAD, "material1")), "arealight1": (L.S03, 1, stretch)}


def stat(xs):
    return {"median_ms": float(np.median(xs)), "min_ms": float(np.min(xs)), "n": len(xs)}


def measure(vpt, name, repeat, discard):
    scene_file, elements, apply = workloads()[name]
    path = os.path.join(L.SCENES, scene_file)
    h = vpt.HostScene(path)
    A, B = vpt.DeviceScene(vpt.HostScene(path), 0), vpt.DeviceScene(h, 0)
    out = []
    times = {True: {"update": [], "host": [], "recreate": [], "stats": None}, False: {"update": [], "host": [], "recreate": [], "stats": None}}
    for r in range(2 * (repeat + discard)):
        fwd = r % 2 == 0
        apply(h, fwd)
        t0 = time.perf_counter()
        edit = h.update_lights()   # update_bvh + make_lights + flatten: the old way needs all of it, the new way the edit alone
        t1 = time.perf_counter()
        abi, keep = edit.to_abi()
        t2 = time.perf_counter()
        vpt._check(vpt.hip.vpt_scene_update_lights(A.handle, C.byref(abi)), "vpt_scene_update_lights")
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
    for fwd in (True, False):
        t = times[fwd]
        rec = {"workload": name, "scene": scene_file, "elements": elements, "direction": "on / moved" if fwd else "off / back",
               "running_sum": "plain" if os.environ.get("VPT_LIGHTS_PLAIN") else "wave", "update_lights": stat(t["update"]),
               "host_make_lights_and_flatten": stat(t["host"]), "destroy_and_create": stat(t["recreate"]), "launches": t["stats"][0], "bytes": t["stats"][1]}
        rec["old_way_median_ms"] = rec["host_make_lights_and_flatten"]["median_ms"] + rec["destroy_and_create"]["median_ms"]
        rec["speedup_median"] = rec["old_way_median_ms"] / rec["update_lights"]["median_ms"]
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".")
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--workloads", default="jade,head,arealight1")
    ap.add_argument("--child", action="store_true", help="internal: print the records, write no file")
    a = ap.parse_args()
    vpt = vpt_loader.load()
    records = []
    for name in a.workloads.split(","):
        records += measure(vpt, name, a.repeat, a.discard)
    if a.child:
        return
    env = dict(os.environ, VPT_LIGHTS_PLAIN="1")   # in a child process, so that the two do not share a handle's state
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--repeat", str(a.repeat), "--discard", str(a.discard), "--workloads",
                        a.workloads], env=env, capture_output=True, text=True, timeout=900)
    records += [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    os.makedirs(a.out, exist_ok=True)
    json.dump(records, open(os.path.join(a.out, "light_update_measure.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
