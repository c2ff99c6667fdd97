"""Fixtures that pin the host mirror's update_lights (and through it vpt_scene_update_lights) to the reference itself.  Run where
oracle/_ref/ref_driver exists (like make_update_fixtures.py, whose pattern this follows).  For every case of tests/light_edits.py:
CASES the edited scene is written out - the materials' emission and instance frames into the scene file, moved vertices into copies
of the binary PLY files - and loaded by the reference's own driver, whose --stats (its make_lights of the edited scene: order,
cdf_len, cdf_back and cdf_fnv of every light) go to tests/golden/light_edit_stats.json.  An update keeps the topology of the
ORIGINAL scene, so a case is only a fixture if the fresh build of the edited scene has that topology (checked through the host
mirror): a case that fails the check is refused, not written.
For the cases of light_edits.STATE_CANDIDATES, in their order until STATE_WANTED are found, the reference also renders the edited
scene (states in tests/golden/light_edit_states.npz), and the share of pixels that are stable under 1-ulp nudges of libm
(oracle_lib.unstable_pixels, a property of the reference alone) is measured here on the CPU and recorded: the GPU test's floor is
0.02 under it, and a case whose share is under 0.8 is refused and the next candidate taken."""
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
sys.path.insert(0, HERE)
import light_edits  # noqa: E402
import vpt_loader  # noqa: E402
import oracle_lib  # noqa: E402
from make_update_fixtures import topology  # noqa: E402
from oracle_lib import REF_DRIVER  # noqa: E402

SCENES = os.path.join(HERE, "scenes")


def main():
    vpt = vpt_loader.load()
    assert os.path.exists(REF_DRIVER), "build the reference driver first (make -C oracle ref)"
    out, states, found = {}, {}, 0
    for name, (scene_file, edit) in light_edits.CASES.items():
        original = vpt.HostScene(os.path.join(SCENES, scene_file))
        edited = vpt.HostScene(os.path.join(SCENES, scene_file))
        edit(edited)
        edited.update_lights()
        with tempfile.TemporaryDirectory(dir=SCENES) as tmp:   # beside the scenes: relative links stay short
            path = light_edits.write_edited_scene(vpt, scene_file, edited, tmp)
            rebuilt = vpt.HostScene(path)
            if topology(vpt, rebuilt) != topology(vpt, original):
                print(f"{name}: a fresh build of the edited scene has another topology - REFUSED, no fixture")
                continue
            stats_file = os.path.join(tmp, "stats.json")
            shader = "implicit" if scene_file in (light_edits.GRID, light_edits.SDFN) else "eyelight"
            subprocess.check_call([REF_DRIVER, "--scene", path, "--shader", shader, "--resolution", "16", "--samples", "1", "--stats", stats_file,
                                   "--state", os.path.join(tmp, "state.bin")], stdout=subprocess.DEVNULL)
            stats = json.load(open(stats_file))
            state = None
            if name in light_edits.STATE_CANDIDATES and found < light_edits.STATE_WANTED:
                shader, res, spp, bounces = light_edits.STATE_CANDIDATES[name]
                w, h, image, hits, rngs, _ = oracle_lib.reference_render(path, shader, res, spp, bounces, workdir=tmp)
                p = vpt.PathtraceParams(resolution=res, samples=spp, shader=shader, bounces=bounces)
                u_stream, u_rad = oracle_lib.unstable_pixels(edited, p, spp, image, rngs, lambda: edited.make_state(p), rounds=16)
                share = float((~(u_stream | u_rad)).mean())
                state = {"shader": shader, "resolution": res, "samples": spp, "bounces": bounces, "stable_share": share}
                if share >= 0.8:
                    states[name + "_image"], states[name + "_rngs"] = image, rngs
                    found += 1
                else:   # the exclusion would swallow the frame: the share is recorded, the state is not a fixture
                    state["refused"] = True
        out[name] = {"scene": scene_file, "stats": {"lights": stats["lights"]}}
        if state:
            out[name]["state_refused" if state.get("refused") else "state"] = state
        same = light_edits.lights_of(edited.stats()) == stats["lights"]
        print(f"{name}: written; the mirror's lights {'equal' if same else 'DIFFER FROM'} the reference's make_lights; {state}", flush=True)
    json.dump(out, open(os.path.join(HERE, "light_edit_stats.json"), "w"), indent=1)
    np.savez_compressed(os.path.join(HERE, "light_edit_states.npz"), **states)


if __name__ == "__main__":
    main()
