"""Re-tesselating a subdiv of a resident scene on the device (include/vpt.h: vpt_scene_update_subdivs) measured against
the parent's way of the same edit: the host mirror's tesselate_surface (HostScene.set_subdiv), then vpt_scene_update with the shape's
vertices.  Everything runs in ONE process; per workload the three sides - device path fused, device path with VPT_UPDATE_NO_FUSE=1,
the parent's way - alternate round by round after --discard warm-up rounds, and every figure is the median of --repeat rounds (an even
number: the two device forms swap places every round, after one untimed device edit that follows the parent's host work).  The
parent's row is taken --spread (5) times: the spread of its medians is what a difference has to exceed.
Workloads: 01_surface_min's cube (4 levels) and suzanne (2 levels) as they are; copies under --work with the cube at 6 levels
(24 576 quads) and suzanne at 4; each with a moved cage, and - the cube, which has texcoords, with a displacement texture added in
the copy - with a displacement amount that changes.  Wall time is around the whole call (for the parent's way: set_subdiv, reading the
shape's arrays, vpt_scene_update); device time, launches and bytes are vpt_scene_update_stats'.  Also per workload: the wall time of
making the plan on the host and of attaching it, the bytes attach sends, and the HBM the plan holds by the rule of DESIGN.md §25.
One JSON line per record, and the list in <out>/subdiv_update_measure.json.

  python profiles/tools/subdiv_update_measure.py [--out DIR (default profiles)] [--work DIR] [--repeat 10] [--discard 2] [--spread 5]"""
import argparse
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
import vpt_loader  # noqa: E402

SURF = "01_surface_min/surface_min.json"
SUZANNE, CUBE = 2, 3


def pad16(n):
    return (n + 15) // 16 * 16


def plan_hbm_bytes(plan, nv_shape):
    """the one allocation of an attached plan (csrc/vpt_subdiv_update.hip: subdiv_attach): every uploaded array and every scratch buffer
    at a 16-byte aligned offset"""
    refined, widest = len(plan.cage_positions), 0
    sizes = [plan.cage_positions.nbytes, plan.cage_normals.nbytes]
    for L in plan.levels:
        refined += len(L["edges"]) + len(L["faces"])
        widest = max(widest, refined)
        sizes += [L[k].nbytes for k in ("edges", "faces", "new_faces", "valence", "offsets", "items")]
    quad_lists, tri_lists = plan.subdivisions > 0 and plan.smooth, plan.displacement_tex >= 0
    corners = int((plan.quads[:, 2] != plan.quads[:, 3]).sum()) + 3 * len(plan.quads)
    sizes += [plan.quads.nbytes if quad_lists else 0, 4 * (refined + 1) if quad_lists else 0, 4 * corners if quad_lists else 0, plan.verts.nbytes]
    triangles = int((plan.quads[:, 2] != plan.quads[:, 3]).sum()) + len(plan.quads)
    sizes += [4 * (nv_shape + 1) if tri_lists else 0, 12 * triangles if tri_lists else 0]
    sizes += [12 * widest] * 3 + [12 * refined if quad_lists else 0] + [12 * nv_shape] * 2 + [12 * nv_shape if tri_lists else 0]
    total = 0
    for s in sizes:
        total = pad16(total) + s
    return total


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs)), "n": len(xs)}


def measure(vpt, name, file, index, kind, a):
    import subdiv_edits as S
    host = vpt.HostScene(file)
    A, B = vpt.DeviceScene(vpt.HostScene(file), 0), vpt.DeviceScene(host, 0)
    s = host.subdiv(index)
    shape, cage = s["shape"], s["positions"]
    t0 = time.perf_counter()
    plan = host.subdiv_plan(index)
    t1 = time.perf_counter()
    A.attach_subdiv(index, plan)
    t2 = time.perf_counter()
    nv = len(host.shape_positions(shape))
    rec = {"workload": name, "edit": kind, "subdivisions": s["subdivisions"], "cage_vertices": len(cage), "shape_vertices": nv, "quads": len(plan.quads),
           "plan_host_ms": (t1 - t0) * 1e3, "attach_wall_ms": (t2 - t1) * 1e3, "attach_bytes": A.update_stats()[1], "plan_hbm_bytes": plan_hbm_bytes(plan, nv)}
    cages = [S.moved(cage, 1), S.moved(cage, 2)]
    amounts = [s["displacement"] * 2, s["displacement"]]

    def payload(r):
        return (cages[r % 2], None) if kind == "moved_cage" else (None, amounts[r % 2])

    def device_path(r, no_fuse):
        os.environ.pop("VPT_UPDATE_NO_FUSE", None)
        if no_fuse:
            os.environ["VPT_UPDATE_NO_FUSE"] = "1"
        edit = vpt.SubdivEdit({index: payload(r)}, shape_of={index: shape})
        t = time.perf_counter()
        A.update_subdivs(edit)
        wall = (time.perf_counter() - t) * 1e3
        os.environ.pop("VPT_UPDATE_NO_FUSE", None)
        return (wall,) + A.update_stats()

    def parents_way(r):
        positions, amount = payload(r)
        t = time.perf_counter()
        host.set_subdiv(index, positions=positions, displacement=amount)
        normals = host.shape_normals(shape)
        B.update(vpt.SceneEdit(shapes={shape: (host.shape_positions(shape), normals if len(normals) else None)}))
        wall = (time.perf_counter() - t) * 1e3
        stats = B.update_stats()
        host.update_subdivs()   # the mirror's own bookkeeping, not part of the edit
        return (wall,) + stats

    sides = {"device_fused": [], "device_unfused": [], "parent": [[] for _ in range(a.spread)]}
    for row in range(a.spread):
        for r in range(a.repeat + a.discard):
            p = parents_way(r)
            device_path(r + 1, r % 2 == 0)   # untimed: the device idled through the parent's host work, and whichever form came next paid for waking it (0.12 ms)
            if r % 2:   # and the two device forms swap places every round
                u, f = device_path(r, True), device_path(r, False)
            else:
                f, u = device_path(r, False), device_path(r, True)
            if r >= a.discard:
                sides["parent"][row].append(p)
                if row == 0:
                    sides["device_fused"].append(f), sides["device_unfused"].append(u)
    assert A.shape_tables_hash() == B.shape_tables_hash(), "the two ways left different tables"

    def side(rows):
        return {"wall_ms": stat([x[0] for x in rows]), "device_ms": stat([x[3] for x in rows]), "launches": rows[-1][1], "bytes_down": rows[-1][2]}

    medians = [float(np.median([x[0] for x in rows])) for rows in sides["parent"]]
    rec.update(device_fused=side(sides["device_fused"]), device_unfused=side(sides["device_unfused"]), parent=side([x for rows in sides["parent"] for x in rows]),
               parent_row_medians_wall_ms=medians, parent_spread_wall_ms=max(medians) - min(medians))
    spread = rec["parent_spread_wall_ms"]
    rec["device_no_slower_than_parent"] = bool(rec["device_fused"]["wall_ms"]["median"] <= rec["parent"]["wall_ms"]["median"] + spread)
    rec["fused_no_slower_than_unfused"] = bool(rec["device_fused"]["wall_ms"]["median"] <= rec["device_unfused"]["wall_ms"]["median"] + spread)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--work", default=None)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--spread", type=int, default=5)
    a = ap.parse_args()
    vpt = vpt_loader.load()
    if vpt.device_count() < 1:
        raise SystemExit("subdiv_update_measure needs a GPU: nothing here is measured without one")
    import subdiv_edits as S
    work = pathlib.Path(a.work or tempfile.mkdtemp())

    def displaced_cube(levels):
        def change(d):
            d["subdivs"][CUBE].update(subdivisions=levels, displacement=0.01, displacement_tex=d["subdivs"][1]["displacement_tex"])
        return change
    own = S.path(SURF)
    cube4 = S.write_scene(SURF, work / "cube4", change=displaced_cube(4))
    large = S.write_scene(SURF, work / "large", settings={SUZANNE: {"subdivisions": 4}}, change=displaced_cube(6))
    workloads = [("cube_4_levels", own, CUBE, "moved_cage"), ("suzanne_2_levels", own, SUZANNE, "moved_cage"), ("cube_4_levels_displaced", cube4, CUBE, "displacement"),
                 ("suzanne_4_levels", large, SUZANNE, "moved_cage"), ("cube_6_levels_displaced", large, CUBE, "displacement"),
                 ("cube_6_levels_displaced", large, CUBE, "moved_cage")]
    records = [measure(vpt, *w, a) for w in workloads]
    os.makedirs(a.out, exist_ok=True)
    json.dump(records, open(os.path.join(a.out, "subdiv_update_measure.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
