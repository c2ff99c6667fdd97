"""Fixtures that pin the light tables at the sizes of tests/light_shapes.py to the reference itself.  Run where oracle/_ref is built
(make -C oracle ref), like make_light_edit_fixtures.py, whose pattern this follows:

    python tests/golden/make_light_size_fixtures.py

light_sizes_stats.json   for every case and for `several`, the `lights` section the reference's driver printed (--stats: its
                         make_lights) for the scene written with the emission on: instance, cdf_len, cdf_back, cdf_fnv of every light
light_sizes_kat.npz      for the cases of light_shapes.KAT_CASES, 512 sample_lights and 512 lights_pdf records and what the
                         reference's own functions returned for them (oracle/_ref/ref_tables on the scene's path).  The records are
                         light_shapes.sample_records / pdf_records: half of the `rel` values sit on and beside CDF entries at the
                         borders of the index groups, half of the pdf directions are the reference's own sampled ones."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kat_lib  # noqa: E402
import light_shapes as S  # noqa: E402
import oracle_lib  # noqa: E402
import vpt_loader  # noqa: E402

STATS = os.path.join(HERE, "light_sizes_stats.json")
KAT = os.path.join(HERE, "light_sizes_kat.npz")


def kat_tables(vpt, case, path):
    """{key: array} of one case: its records and the reference's answers"""
    host = vpt.HostScene(path)
    lights, cdf = host.lights()
    (light, _), = S.lights_under_test(case).items()
    own = cdf[int(lights[light]["cdf_offset"]):][:case.n]
    sl = S.sample_records(case, own, light, len(lights))
    aimed = S.run_reference(path, "sample_lights", 0, sl)
    pdf = S.pdf_records(case, sl, aimed)
    return {case.name + "_sl_in": sl, case.name + "_sl_out": aimed, case.name + "_pdf_in": pdf, case.name + "_pdf_out": S.run_reference(path, "lights_pdf", 450, pdf)}


def main():
    assert os.path.exists(oracle_lib.REF_DRIVER) and kat_lib.have_reference(), "build the reference programs first (make -C oracle ref)"
    vpt = vpt_loader.load()
    stats, tables = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, case in list(S.CASES.items()) + [("several", "several")]:
            path = S.write_scene(os.path.join(tmp, name), case, on=True)
            stats[name] = {"lights": S.reference_lights(path, os.path.join(tmp, name))}
            if name in S.KAT_CASES:
                tables.update(kat_tables(vpt, case, path))
            print(f"{name}: {stats[name]['lights']}", flush=True)
    json.dump(stats, open(STATS, "w"), indent=1)
    np.savez_compressed(KAT, **tables)
    print("wrote", STATS, os.path.getsize(STATS), "bytes;", KAT, os.path.getsize(KAT), "bytes")


if __name__ == "__main__":
    main()
