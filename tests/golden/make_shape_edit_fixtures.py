"""Fixtures that pin the host mirror's edit_shapes (and through it vpt_scene_update_shapes) to the reference itself.  Run where
oracle/_ref/ref_driver exists (like make_instance_edit_fixtures.py).  For every case of tests/shape_edits.py the scene is taken
through the case's steps on the host mirror and written out: the shapes the edit made as binary float32 PLY, the instance array as
the mirror holds it; the reference's own driver loads that file, and its --stats (its make_bvh and make_lights of the edited scene:
the scene BVH's counts and hashes, per shape positions, pos_fnv, bvh_nodes, bvh_nodes_fnv, bvh_prims_fnv, and cdf_len / cdf_back /
cdf_fnv of every light) go to tests/golden/shape_edit_stats.json.
No case may be recorded as refused: new geometry is float32 in binary PLY so that the loader gives it back bit for bit, and this
script checks it - it compares the reference's statistics with the mirror's and names the case that differs.  A case whose scene
BVH is not built anew by the edit (no shape replaced) keeps the tree the scene was loaded with, which is make_bvh's of the same
instance boxes: the comparison holds for it too."""
import json
import os
import pathlib
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shape_edits as S  # noqa: E402
import vpt_loader  # noqa: E402
from oracle_lib import REF_DRIVER  # noqa: E402

KEEP = ("positions", "pos_fnv", "bvh_nodes", "bvh_nodes_fnv", "bvh_prims_fnv")


def main():
    vpt = vpt_loader.load()
    assert os.path.exists(REF_DRIVER), "build the reference driver first (make -C oracle ref)"
    out, differs = {}, []
    for name, case in S.CASES.items():
        with tempfile.TemporaryDirectory(dir=S.SCENES) as tmp:   # beside the scenes: relative links stay short
            source = case.path(pathlib.Path(tmp) / "source")
            edited, names = vpt.HostScene(source), S.shape_names(source)
            S.apply(edited, case, names=names)
            mine = json.loads(edited.stats())
            path = S.write_edited_scene(source, edited, names, os.path.join(tmp, "written"))
            stats_file = os.path.join(tmp, "stats.json")
            subprocess.check_call([REF_DRIVER, "--scene", path, "--shader", "eyelight", "--resolution", "16", "--samples", "1", "--stats", stats_file,
                                   "--state", os.path.join(tmp, "state.bin")], stdout=subprocess.DEVNULL)
            stats = json.load(open(stats_file))
        out[name] = {"stats": {"scene_bvh": stats["scene_bvh"], "shapes": [{k: s[k] for k in KEEP} for s in stats["shapes"]], "lights": stats["lights"]}}
        same_bvh = mine["scene_bvh"] == stats["scene_bvh"] and len(mine["shapes"]) == len(stats["shapes"]) and \
            all(m[k] == s[k] for m, s in zip(mine["shapes"], stats["shapes"]) for k in KEEP)
        same_lights = mine["lights"] == stats["lights"]
        print(f"{name}: the reference's shape and scene BVHs {'equal' if same_bvh else 'DIFFER FROM'} the mirror's; "
              f"its lights {'equal' if same_lights else 'DIFFER FROM'} the mirror's", flush=True)
        if not (same_bvh and same_lights):
            differs.append(name)
    assert not differs, f"change the numbers of {differs} in tests/shape_edits.py: the reference's loader does not give them back bit for bit"
    json.dump(out, open(os.path.join(HERE, "shape_edit_stats.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
