#!/usr/bin/env python3
"""Regenerates tests/golden/sculpt_kat.npz: a wider table of the six analytic SDF functions than kat_tables.npz holds (its points lie
in +-0.3 only), answered by the REFERENCE'S OWN sdf_data::f through the reference build (oracle/_ref/ref_tables, op sdf_function, as
tests/golden/make_kat.py asks it): for 07_sdfunction_synth's ten SDFs, 4 096 points in +-1.5 and, per SDF, points on the faces of its
shape, on the coordinate axes and planes, and the origin.  tests/test_sculpt_host.py pins the brush distance of the sculpt rule
(csrc/vpt_sculpt_rule.h) to it bit for bit.  Data only.  Run where the reference build exists:

    python tests/golden/make_sculpt_fixtures.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kat_lib as K  # noqa: E402
import vpt_loader  # noqa: E402

OUT = os.path.join(HERE, "sculpt_kat.npz")
KEY = "07_sdfunction_synth"
F = np.float32


def special_points(sdf):
    """points where the functions' selects and square roots meet their edge cases: the origin, the axes, the coordinate planes, and the
    faces, edges and corners of the shape's own extents (half extents, radii, heights), both signs"""
    ext = sorted({abs(float(v)) for v in list(sdf.p) + list(sdf.whd) + [0.5 * float(w) for w in sdf.whd]} | {0.0})
    vals = sorted({s * v for v in ext for s in (-1.0, 1.0)} | {0.125, -0.125})
    pts = [(x, y, z) for x in vals for y in vals for z in vals]
    return np.array(pts, F)


def main():
    assert K.have_reference(), "build oracle/_ref first: make -C oracle ref"
    vpt = vpt_loader.load()
    host = vpt.HostScene(K.scene_path(KEY))
    nsdf = host.count_implicit("sdfs")
    rng = np.random.default_rng(2700)
    n = 4096
    rec = np.zeros((n, 4), F)
    rec[:, 0] = rng.integers(0, nsdf, size=n)
    rec[:, 1:4] = rng.uniform(-1.5, 1.5, size=(n, 3))
    extra = []
    for i in range(nsdf):
        pts = special_points(host.sdf(i))
        on_axes = (pts == 0).sum(axis=1) >= 2   # the origin and the points of the three axes: always kept
        keep, rest = pts[on_axes], pts[~on_axes]
        if len(rest) > 216:   # of the others at most six values per axis and SDF
            rest = rest[rng.choice(len(rest), 216, replace=False)]
        pts = np.concatenate([keep, rest])
        extra.append(np.concatenate([np.full((len(pts), 1), i, F), pts], axis=1))
    rec = np.ascontiguousarray(np.concatenate([rec] + extra), F)
    out = K.run_reference(KEY, "sdf_function", 0, rec)
    np.savez_compressed(OUT, sdf_function_in=rec, sdf_function_out=out)
    print(f"wrote {OUT}: {len(rec)} records, {os.path.getsize(OUT) // 1024} KiB; finite {np.isfinite(out).mean():.3f}")


if __name__ == "__main__":
    main()
