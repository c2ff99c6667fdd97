"""Fixtures that pin the host mirror's edit_instances (and through it vpt_scene_update_instances) to the reference itself.  Run
where oracle/_ref/ref_driver exists (like make_rebuild_fixtures.py).  For every case of tests/instance_edits.py the scene is taken
through the case's steps on the host mirror and written out with its instance array rewritten as the mirror holds it; the
reference's own driver loads that file, and its --stats (its make_bvh and make_lights of the edited scene: the scene BVH's counts and
hashes, the shapes' hashes, cdf_len / cdf_back / cdf_fnv of every light) go to tests/golden/instance_edit_stats.json.
No case may be recorded as refused: the frames of the cases are dyadic so that the loader gives them back bit for bit, and this
script checks it - it compares the reference's scene-BVH hashes and lights with the mirror's and says which case differs.  A case
that differs gets other numbers in tests/instance_edits.py, not a refusal."""
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
import instance_edits as I  # noqa: E402
import vpt_loader  # noqa: E402
from oracle_lib import REF_DRIVER  # noqa: E402

KEEP = ("positions", "pos_fnv", "bvh_nodes", "bvh_nodes_fnv", "bvh_prims_fnv")


def main():
    vpt = vpt_loader.load()
    assert os.path.exists(REF_DRIVER), "build the reference driver first (make -C oracle ref)"
    out, differs = {}, []
    for name, case in I.CASES.items():
        with tempfile.TemporaryDirectory(dir=I.SCENES) as tmp:   # beside the scenes: relative links stay short
            source = case.path(pathlib.Path(tmp) / "source")
            edited = vpt.HostScene(source)
            I.apply(edited, case)
            mine = json.loads(edited.stats())
            path = I.write_edited_scene(source, edited, os.path.join(tmp, "written"))
            stats_file = os.path.join(tmp, "stats.json")
            subprocess.check_call([REF_DRIVER, "--scene", path, "--shader", "eyelight", "--resolution", "16", "--samples", "1", "--stats", stats_file,
                                   "--state", os.path.join(tmp, "state.bin")], stdout=subprocess.DEVNULL)
            stats = json.load(open(stats_file))
        out[name] = {"stats": {"scene_bvh": stats["scene_bvh"], "shapes": [{k: s[k] for k in KEEP} for s in stats["shapes"]], "lights": stats["lights"]}}
        same_bvh = mine["scene_bvh"] == stats["scene_bvh"] and all(m[k] == s[k] for m, s in zip(mine["shapes"], stats["shapes"]) for k in KEEP)
        same_lights = mine["lights"] == stats["lights"]
        print(f"{name}: the reference's scene BVH {stats['scene_bvh']['nodes_fnv']} {'equals' if same_bvh else 'DIFFERS FROM'} the mirror's "
              f"{mine['scene_bvh']['nodes_fnv']}; its lights {'equal' if same_lights else 'DIFFER FROM'} the mirror's", flush=True)
        if not (same_bvh and same_lights):
            differs.append(name)
    assert not differs, f"change the numbers of {differs} in tests/instance_edits.py: the reference's loader does not give them back bit for bit"
    json.dump(out, open(os.path.join(HERE, "instance_edit_stats.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
