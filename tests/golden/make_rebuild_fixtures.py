"""Fixtures that pin the host mirror's rebuild_bvh (and through it vpt_scene_rebuild_bvh) to the reference itself.  Run where
oracle/_ref/ref_driver exists (like make_update_fixtures.py, whose scene writer this script uses).  For every case of
tests/rebuild_edits.py the scene is taken through the case's steps on the host mirror, written out as the mirror holds it - instance
frames into the scene file, moved vertices into copies of the PLY files or, for the synthetic OBJ shapes, into new PLY files - and
loaded by the reference's own driver, whose --stats (its make_bvh of the edited scene: node counts, hashes of nodes and primitive
orders) go to tests/golden/rebuild_stats.json.  A case is a fixture only if the reference's loader reads the written scene bit for
bit (the position hashes of its statistics equal the mirror's); one that does not is recorded as refused, with the reason."""
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
sys.path.insert(0, HERE)
import rebuild_edits as R  # noqa: E402
import vpt_loader  # noqa: E402
from make_update_fixtures import SCENES, write_edited_scene  # noqa: E402
from oracle_lib import REF_DRIVER  # noqa: E402

KEEP = ("positions", "pos_fnv", "bvh_nodes", "bvh_nodes_fnv", "bvh_prims_fnv")


def main():
    vpt = vpt_loader.load()
    assert os.path.exists(REF_DRIVER), "build the reference driver first (make -C oracle ref)"
    out = {}
    for name, case in R.CASES.items():
        with tempfile.TemporaryDirectory(dir=SCENES) as tmp:   # beside the scenes: relative links stay short
            source = case.path(pathlib.Path(tmp) / "source")
            edited = vpt.HostScene(source)
            R.apply(edited, case)
            mine = json.loads(edited.stats())
            try:
                path = write_edited_scene(vpt, source, edited, os.path.join(tmp, "written"))
            except AssertionError as e:
                out[name] = {"refused": f"the edited scene cannot be written for the reference's loader: {e}"}
                print(f"{name}: REFUSED ({out[name]['refused']})", flush=True)
                continue
            stats_file = os.path.join(tmp, "stats.json")
            subprocess.check_call([REF_DRIVER, "--scene", path, "--shader", "eyelight", "--resolution", "16", "--samples", "1", "--stats", stats_file,
                                   "--state", os.path.join(tmp, "state.bin")], stdout=subprocess.DEVNULL)
            stats = json.load(open(stats_file))
        if [s["pos_fnv"] for s in stats["shapes"]] != [s["pos_fnv"] for s in mine["shapes"]]:
            out[name] = {"refused": "the reference's loader does not give the written vertices back bit for bit (position hashes differ)"}
            print(f"{name}: REFUSED ({out[name]['refused']})", flush=True)
            continue
        out[name] = {"stats": {"scene_bvh": stats["scene_bvh"], "shapes": [{k: s[k] for k in KEEP} for s in stats["shapes"]]}}
        same = mine["scene_bvh"] == stats["scene_bvh"] and all(m[k] == s[k] for m, s in zip(mine["shapes"], stats["shapes"]) for k in KEEP)
        print(f"{name}: written; the mirror's rebuild {'equals' if same else 'DIFFERS FROM'} the reference's build", flush=True)
    json.dump(out, open(os.path.join(HERE, "rebuild_stats.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
