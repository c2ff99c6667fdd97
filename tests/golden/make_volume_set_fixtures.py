"""Fixtures that pin the host mirror's update_volume_set (and through it vpt_scene_update_volume_set) to the reference itself.  Run where
oracle/_ref/ref_driver exists (like make_volume_edit_fixtures.py, whose pattern this follows).  For every case of
tests/volume_set_edits.py's STATE_CASES the edited scene is written out with its .sdf files (volume_set_edits.write_edited_scene: from the numpy
side of the case, not from the scene under test) and rendered by the reference's own driver at 96 pixels with 2 or 3 samples; the
states go to tests/golden/volume_set_states.npz, what was rendered to tests/golden/volume_set_stats.json.  The test
(tests/test_volume_set_host.py) asks the oracle over the HostScene edited through the setters for the same bits; this script
prints whether it gives them."""
import json
import os
import pathlib
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import volume_set_edits as V  # noqa: E402
import vpt_loader  # noqa: E402
import oracle_lib  # noqa: E402
from oracle_lib import REF_DRIVER  # noqa: E402

SCENES = os.path.join(HERE, "scenes")
BOUNCES = 4


def main():
    vpt = vpt_loader.load()
    assert os.path.exists(REF_DRIVER), "build the reference driver first (make -C oracle ref)"
    out, states = {}, {}
    for name, (shader, res, spp) in V.STATE_CASES.items():
        scene_file = V.scene_of(vpt, name)
        with tempfile.TemporaryDirectory(dir=SCENES) as tmp:   # beside the scenes: relative links stay short
            work = pathlib.Path(tmp)
            path = V.write_edited_scene(vpt, name, work)
            w, h, image, hits, rngs, _ = oracle_lib.reference_render(path, shader, res, spp, BOUNCES, workdir=tmp)
            states[name + "_image"], states[name + "_rngs"] = image, rngs
            out[name] = {"scene": scene_file, "shader": shader, "resolution": res, "samples": spp, "bounces": BOUNCES, "width": w, "height": h}
            edited = vpt.HostScene(os.path.join(SCENES, scene_file))
            V.apply(vpt, name, edited)
            p = vpt.PathtraceParams(resolution=res, samples=spp, shader=shader, bounces=BOUNCES)
            st = edited.make_state(p)
            oracle_lib.oracle_render(edited, p, st, spp, nthreads=0)
            same = np.array_equal(st.rngs, rngs) and np.array_equal(st.image.view(np.uint32), image.view(np.uint32))
            print(f"{name}: written; the oracle on the edited HostScene {'equals' if same else 'DIFFERS FROM'} the reference's render", flush=True)
    json.dump({k: out[k] for k in sorted(out)}, open(os.path.join(HERE, "volume_set_stats.json"), "w"), indent=1)
    np.savez_compressed(os.path.join(HERE, "volume_set_states.npz"), **states)


if __name__ == "__main__":
    main()
