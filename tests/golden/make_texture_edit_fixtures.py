"""Fixtures that pin the host mirror's update_textures (and through it vpt_scene_update_textures) to the reference itself.  Run where
oracle/_ref/ref_driver exists (like make_light_edit_fixtures.py, whose pattern this follows).  For every case of
tests/texture_edits.py that a scene file can express (AS_SCENE_FILE: the environment's emission or emission_tex changed, or another
image file in the sky's slot) the edited scene is written out and loaded by the reference's own driver, whose --stats (its
make_lights of the edited scene: order, cdf_len, cdf_back and cdf_fnv of every light; the hashes of its BVHs) go to
tests/golden/texture_edit_stats.json.
For the cases of texture_edits.STATE_CANDIDATES, in their order until STATE_WANTED are found, the reference also renders the edited
scene (states in tests/golden/texture_edit_states.npz), and the share of pixels that are stable under 1-ulp nudges of libm
(oracle_lib.unstable_pixels, a property of the reference alone) is measured here on the CPU and recorded: the GPU test's floor is
0.02 under it, and a case whose share is under 0.8 is refused and the next candidate taken.
The K2 case of texture_edits (grid_sky_13x5) replaces the sky in 06_gridsdf_synth's one texture slot: the scene has a slot, so the
alternative of switching its environment's emission on and off is not used.  It has no scene file and no fixture here."""
import json
import os
import pathlib
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import texture_edits as T  # noqa: E402
import vpt_loader  # noqa: E402
import oracle_lib  # noqa: E402
from oracle_lib import REF_DRIVER  # noqa: E402

SCENES = os.path.join(HERE, "scenes")


def main():
    vpt = vpt_loader.load()
    assert os.path.exists(REF_DRIVER), "build the reference driver first (make -C oracle ref)"
    out, states, found = {}, {}, 0
    names = list(T.STATE_CANDIDATES) + [n for n in T.AS_SCENE_FILE if n not in T.STATE_CANDIDATES]
    for name in names:
        with tempfile.TemporaryDirectory(dir=SCENES) as tmp:   # beside the scenes: relative links stay short
            work = pathlib.Path(tmp)
            edited = vpt.HostScene(os.path.join(SCENES, T.S03))
            T.apply(vpt, name, edited, work)
            path = T.write_edited_scene(name, work)
            stats_file = os.path.join(tmp, "stats.json")
            subprocess.check_call([REF_DRIVER, "--scene", path, "--shader", "eyelight", "--resolution", "16", "--samples", "1", "--stats", stats_file,
                                   "--state", os.path.join(tmp, "state.bin")], stdout=subprocess.DEVNULL)
            stats = json.load(open(stats_file))
            state = None
            if name in T.STATE_CANDIDATES and found < T.STATE_WANTED:
                shader, res, spp, bounces = T.STATE_CANDIDATES[name]
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
            bvh = {"scene_bvh": stats["scene_bvh"], "shapes": [{k: s[k] for k in ("bvh_nodes", "bvh_nodes_fnv", "bvh_prims_fnv")} for s in stats["shapes"]]}
            out[name] = {"scene": T.S03, "stats": {"lights": stats["lights"], "textures": stats["textures"], **bvh}}
            if state:
                out[name]["state_refused" if state.get("refused") else "state"] = state
            same = T.lights_of(edited.stats()) == stats["lights"]
            print(f"{name}: written; the mirror's lights {'equal' if same else 'DIFFER FROM'} the reference's make_lights; {state}", flush=True)
    json.dump({k: out[k] for k in sorted(out)}, open(os.path.join(HERE, "texture_edit_stats.json"), "w"), indent=1)
    np.savez_compressed(os.path.join(HERE, "texture_edit_states.npz"), **states)


if __name__ == "__main__":
    main()
