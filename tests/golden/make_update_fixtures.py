"""Fixtures that pin the host mirror's update_bvh (and through it vpt_scene_update) to the reference itself.  Run where
oracle/_ref/ref_driver exists (like make_fixtures.py).  For every case of tests/scene_edits.py: PINNED the edited scene is written
out - instance frames into the scene file, moved vertices into copies of the binary PLY files, x / y / z patched in place - and
loaded by the reference's own driver, whose --stats (its make_bvh of the edited scene) go to tests/golden/update_stats.json.  A
refit keeps the topology of the ORIGINAL scene, so a case is only a fixture if the fresh build of the edited scene happens to have
that topology: checked here through the host mirror (start, num, axis, internal of every node, every primitive order) - a case
that fails the check is refused, not written.
For the cases of scene_edits.STATE_CASES the reference also renders the edited scene (states in tests/golden/update_states.npz, at the
sizes tests/cases.py and make_curves_scene.py use), and the share of pixels that are stable under 1-ulp nudges of libm
(oracle_lib.unstable_pixels, a property of the reference alone) is measured here on the CPU and recorded: the GPU test's floor is
0.02 under it, and a case whose share is under 0.8 is refused.
A scene whose edited shapes are not PLY files or come from subdivision cages (01_surface_min) is written with every such shape as the
host mirror holds it after tesselation - all arrays into a new PLY, v of the texcoords as 1 - v because the loaders flip it - and
without its "subdivs": the reference then loads the very vertices its own tesselation gives (the committed pos_fnv hashes say so).
The flip does not give the texcoords' bits back, so such a case pins positions and BVHs and gets no rendered state."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scene_edits  # noqa: E402
import vpt_loader  # noqa: E402
import oracle_lib  # noqa: E402
from make_curves_scene import write_ply  # noqa: E402
from oracle_lib import REF_DRIVER  # noqa: E402

SCENES = os.path.join(HERE, "scenes")


def patch_ply_positions(src, dst, positions):
    """copy of a binary little-endian PLY whose vertex properties are all floats, x / y / z replaced"""
    raw = open(src, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode().splitlines()
    assert lines[1] == "format binary_little_endian 1.0", src
    at = next(i for i, l in enumerate(lines) if l.startswith("element vertex"))
    count = int(lines[at].split()[2])
    props = []
    for l in lines[at + 1:]:
        if not l.startswith("property"):
            break
        assert l.split()[1] == "float", (src, l)
        props.append(l.split()[2])
    assert props[:3] == ["x", "y", "z"] and count == len(positions), src
    verts = np.frombuffer(raw, "<f4", count * len(props), end).reshape(count, len(props)).copy()
    verts[:, :3] = positions
    open(dst, "wb").write(raw[:end] + verts.astype("<f4").tobytes() + raw[end + verts.nbytes:])


def write_edited_scene(vpt, scene_file, edited, out):
    """the scene of `scene_file` as the HostScene `edited` holds it now, under directory `out`; returns the scene file's path"""
    src_dir = os.path.dirname(os.path.join(SCENES, scene_file))
    d = json.load(open(os.path.join(SCENES, scene_file)))
    original = vpt.HostScene(os.path.join(SCENES, scene_file))
    for i, inst in enumerate(d["instances"]):
        if not np.array_equal(original.instance_frame(i), edited.instance_frame(i)):
            inst["frame"] = [float(x) for x in edited.instance_frame(i)]
    os.makedirs(os.path.join(out, "edited_shapes"), exist_ok=True)
    subdivided = {sd.get("shape") for sd in d.get("subdivs", [])}
    moved = {s for s in range(len(d["shapes"])) if not np.array_equal(original.shape_positions(s), edited.shape_positions(s))}
    whole = any(s in subdivided or not d["shapes"][s]["uri"].endswith(".ply") for s in moved)   # tesselated meshes go out as they are
    for s, shape in enumerate(d["shapes"]):
        uri = os.path.join(src_dir, shape["uri"])
        if whole and (s in moved or s in subdivided):
            a = edited.shape_arrays(s)
            opt = lambda x: x if len(x) else None
            uv = a["texcoords"].copy()
            if len(uv):
                uv[:, 1] = np.float32(1) - uv[:, 1]
            faces = a["triangles"] if len(a["triangles"]) else a["quads"]
            write_ply(os.path.join(out, "edited_shapes", f"{s}.ply"), a["positions"], opt(a["normals"]), opt(uv), opt(a["colors"]), opt(a["radius"]),
                      lines=[list(l) for l in a["lines"]], points=[[q] for q in a["points"]], faces=[list(f) for f in faces])
        elif s in moved:
            patch_ply_positions(uri, os.path.join(out, "edited_shapes", f"{s}.ply"), edited.shape_positions(s))
        else:
            shape["uri"] = os.path.relpath(uri, out)
            continue
        shape["uri"] = f"edited_shapes/{s}.ply"
    if whole:
        d.pop("subdivs", None)
    for key in ("textures", "subdivs", "volumes"):
        for item in d.get(key, []):
            if "uri" in item:
                item["uri"] = os.path.relpath(os.path.join(src_dir, item["uri"]), out)
    path = os.path.join(out, "edited.json")
    json.dump(d, open(path, "w"))
    return path


def topology(vpt, h):
    import ctypes as C
    d = vpt.VptSceneDescBvh.from_address(h.desc + vpt.VptSceneDescBvh.OFFSET)
    a, b = h.bvh_nodes()
    prims = lambda p, n: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), (int(n),)).tobytes() if n else b""
    return ([x[k].tobytes() for x in (a, b) for k in ("start", "num", "axis", "internal")],
            prims(d.scene_bvh_prims, d.num_scene_bvh_prims), prims(d.shape_bvh_prims, d.num_shape_bvh_prims))


def main():
    vpt = vpt_loader.load()
    assert os.path.exists(REF_DRIVER), "build the reference driver first (make -C oracle ref)"
    out, states = {}, {}
    for name, (scene_file, edit) in scene_edits.PINNED.items():
        original = vpt.HostScene(os.path.join(SCENES, scene_file))
        edited = vpt.HostScene(os.path.join(SCENES, scene_file))
        edit(edited)
        edited.update_bvh()
        with tempfile.TemporaryDirectory(dir=SCENES) as tmp:   # beside the scenes: relative links stay short
            path = write_edited_scene(vpt, scene_file, edited, tmp)
            rebuilt = vpt.HostScene(path)
            if topology(vpt, rebuilt) != topology(vpt, original):
                print(f"{name}: a fresh build of the edited scene has another topology - REFUSED, no fixture")
                continue
            stats_file = os.path.join(tmp, "stats.json")
            subprocess.check_call([REF_DRIVER, "--scene", path, "--shader", "eyelight", "--resolution", "16", "--samples", "1", "--stats", stats_file,
                                   "--state", os.path.join(tmp, "state.bin")], stdout=subprocess.DEVNULL)
            stats = json.load(open(stats_file))
            state = None
            if name in scene_edits.STATE_CANDIDATES:
                shader, res, spp, bounces = scene_edits.STATE_CANDIDATES[name]
                w, h, image, hits, rngs, _ = oracle_lib.reference_render(path, shader, res, spp, bounces, workdir=tmp)
                p = vpt.PathtraceParams(resolution=res, samples=spp, shader=shader, bounces=bounces)
                u_stream, u_rad = oracle_lib.unstable_pixels(edited, p, spp, image, rngs, lambda: edited.make_state(p), rounds=16)
                share = float((~(u_stream | u_rad)).mean())
                state = {"shader": shader, "resolution": res, "samples": spp, "bounces": bounces, "stable_share": share}
                if share >= 0.8:
                    states[name + "_image"], states[name + "_rngs"] = image, rngs
                else:   # the exclusion would swallow the frame: the share is recorded, the state is not a fixture
                    state["refused"] = True
        keep = ("positions", "pos_fnv", "bvh_nodes", "bvh_nodes_fnv", "bvh_prims_fnv")
        out[name] = {"scene": scene_file, "stats": {"scene_bvh": stats["scene_bvh"], "shapes": [{k: s[k] for k in keep} for s in stats["shapes"]]}}
        if state:
            out[name]["state_refused" if state.get("refused") else "state"] = state
        same = json.loads(edited.stats())["scene_bvh"] == stats["scene_bvh"]
        print(f"{name}: written; the mirror's refit {'equals' if same else 'DIFFERS FROM'} the reference's build; {state}", flush=True)
    json.dump(out, open(os.path.join(HERE, "update_stats.json"), "w"), indent=1)
    np.savez_compressed(os.path.join(HERE, "update_states.npz"), **states)


if __name__ == "__main__":
    main()
