"""The float64 reference and certificate of tests/curve_exact.py, shown right and sharp without a GPU: a float32 restatement of the
reference's intersect_point / intersect_line (tests/curve_restated.py), run as a brute force over every element, passes the certificate
with no violation on every ray set; the rays whose verdict rests on an undecided pair stay under their caps; the ray sets reach what
they are meant to reach; and each of seven planted defects is rejected.

Measured with the bounds of curve_exact's docstring (float32 restatement, no violation anywhere):
  synthetic sets   4.1 % of the rays undecided (168 of 4 088; cap 10 %, for every set too): lines 5.7 % (of them the 120 rays parallel to
                   a segment, undecidable against it by construction: 61), points 3.1 %, edge 3.9 %, tmin 3.6 %, inside 0 %
  dense.json       1.0 % (5 of the 512 rays of test_intersect_on_dense_strands against the 20 000 segments; cap 15 %)"""
import os

import numpy as np
import pytest

import curve_cases
import curve_exact
import curve_restated
from conftest import GOLDEN

DENSE = os.path.join(GOLDEN, "scenes", "09_curves_synth", "dense.json")
PIXELS = 96
LINE_PIXELS, POINT_PIXELS = 30, 15     # the floors of the AOV test (tests/test_curve_exact_gpu.py), known here from the float64 reference


@pytest.fixture(scope="module")
def case(vpt, tmp_path_factory):
    return curve_cases.Case(vpt, tmp_path_factory.mktemp("curve_exact"))


@pytest.fixture(scope="module")
def restated(case):
    """{set: (ids, uvt)} of the float32 restatement"""
    return {name: curve_restated.brute_force(case.elements, rays) for name, rays in case.sets.items()}


def _report(verdict):
    return f"{len(verdict.violations)} violations, the first: {verdict.violations[:3]}"


def test_float32_restatement_passes_with_no_violation_and_few_undecided(case, restated):
    undecided = total = 0
    for name, (ids, uvt) in restated.items():
        assert len(case.sets[name]) <= 8192 and case.sets[name].dtype == np.float32
        verdict = curve_exact.certify(case.refs[name], ids, uvt)
        print(f"{name}: {len(ids)} rays, {(ids[:, 0] >= 0).sum()} hits, undecided {verdict.undecided.sum()} ({verdict.share:.1%})")
        assert not verdict.violations, f"{name}: {_report(verdict)}"
        assert verdict.share <= 0.10, name
        undecided, total = undecided + int(verdict.undecided.sum()), total + len(ids)
    print(f"synthetic sets: {undecided} of {total} rays undecided ({undecided / total:.1%})")
    assert undecided <= 0.10 * total


def test_single_instance_queries_pass(case):
    for variant in ("lines_all", "points_colors"):
        for frame in curve_cases.FRAMES:
            inst = curve_cases.instance_of(variant, frame)
            name = "lines" if variant.startswith("lines") else "points"
            el = [e for e in case.elements if e.instance == inst]
            ids, uvt = curve_restated.brute_force(el, case.sets[name])
            verdict = curve_exact.certify(case.refs[name], ids, uvt, instances=[inst])
            assert not verdict.violations, f"{variant} {frame}: {_report(verdict)}"
            assert (ids[:, 0] == inst).sum() >= 30


def test_dense_strands_pass_with_few_undecided(vpt):
    scene = vpt.HostScene(DENSE)
    elements = curve_exact.curve_instances(scene, [2])
    assert len(elements) == 1 and len(elements[0]) == 20000
    rays = curve_cases.dense_rays()
    ids, uvt = curve_restated.brute_force(elements, rays)
    verdict = curve_exact.certify(curve_exact.Reference(elements, rays, chunk=32), ids, uvt)
    print(f"dense: {(ids[:, 0] >= 0).sum()} hits, {verdict.undecided.sum()} of {len(rays)} rays undecided ({verdict.share:.1%})")
    assert not verdict.violations, _report(verdict)
    assert (ids[:, 0] == 2).sum() > len(rays) // 8
    assert verdict.undecided.sum() <= 0.15 * len(rays)


def test_ray_sets_reach_what_they_are_meant_to(case):
    rays = np.concatenate(list(case.sets.values()))
    cover = curve_exact.coverage(case.elements, rays)
    print({k: v for k, v in cover.items() if k != "hits"}, "fewest decided hits on an instance:", min(cover["hits"].values()))
    assert len(cover["hits"]) == 3 * len(curve_cases.VARIANTS) and min(cover["hits"].values()) >= 30, cover["hits"]
    assert cover["clamped0"] >= 100 and cover["clamped1"] >= 100
    assert cover["near_misses"] >= 100
    assert cover["tmin_only"] >= 20


@pytest.fixture(scope="module")
def pixel_rays(case):
    return curve_exact.camera_rays(case.scene.camera(0), PIXELS, PIXELS).reshape(-1, 6)


def test_pixel_centre_rays_reach_every_variant(case, pixel_rays):
    ref = curve_exact.Reference(case.elements, pixel_rays.astype(np.float32))
    nearest = curve_exact.nearest_decided(ref)
    ids, uvt = curve_restated.brute_force(case.elements, ref.rays)
    verdict = curve_exact.certify(ref, ids, uvt)
    assert not verdict.violations, _report(verdict)
    sure = (nearest == ids).all(1) & ~verdict.undecided & (ids[:, 0] >= 0)     # the nearest decided hit, and nothing undecided before it
    counts = {v: int((sure & (ids[:, 0] // 3 == k)).sum()) for k, v in enumerate(curve_cases.VARIANTS)}
    print(counts)
    for variant, n in counts.items():
        assert n >= (LINE_PIXELS if variant in curve_cases.LINE_VARIANTS else POINT_PIXELS), counts


@pytest.mark.parametrize("mutation", curve_restated.MUTATIONS)
def test_planted_defect_is_rejected(case, restated, mutation):
    found = 0
    for name, rays in case.sets.items():
        ids, uvt = curve_restated.brute_force(case.elements, rays, mutation)
        verdict = curve_exact.certify(case.refs[name], ids, uvt)
        found += len(verdict.violations)
    print(f"{mutation}: {found} violations")
    assert found > 0


def test_shading_reference_tells_the_lerp_order_and_the_normal_source(case):
    g = np.random.default_rng(3)
    el = [e for e in case.elements if e.instance == curve_cases.instance_of("lines_all", "rigid")][0]
    n = 64
    element, u, v = g.integers(0, len(el), n), g.uniform(0.05, 0.45, n), g.uniform(0, 1, n)
    outgoing = g.normal(size=(n, 3))
    color = case.material_color(el.instance)
    right = curve_exact.shade(el, color, element, u, v, outgoing)
    wrong = curve_exact.shade(el, color, element, 1 - u, v, outgoing)          # lerp(c1, c0, u) is lerp(c0, c1, 1 - u)
    assert (np.abs(right["color"] - wrong["color"]).max(1) > 100 * right["e_color"]).mean() > 0.9
    assert (np.abs(right["texcoord"] - wrong["texcoord"]).max(1) > 100 * right["e_texcoord"]).mean() > 0.9
    bare = curve_exact.Elements(el.instance, el.shape, False, dict(case.scene.shape_arrays(el.shape), normals=np.zeros((0, 3), np.float32)),
                                case.scene.instance_frame(el.instance))
    tangent = curve_exact.shade(bare, color, element, u, v, outgoing)          # the same shape without its normals: the line tangent
    assert (np.abs(right["normal"] - tangent["normal"]).max(1) > 100 * right["e_normal"]).mean() > 0.9
    # the values themselves, against the formulas written out for one hit
    A, (i0, i1) = el.arrays, el.ids[element[0]]
    assert np.allclose(right["color"][0], color * (A["colors"][i0, :3] * (1 - u[0]) + A["colors"][i1, :3] * u[0]), rtol=1e-12)
    nrm = A["normals"][i0] * (1 - u[0]) + A["normals"][i1] * u[0]
    nrm = el.M @ (nrm / np.linalg.norm(nrm))
    nrm /= np.linalg.norm(nrm)
    w = outgoing[0] - nrm * (outgoing[0] @ nrm)
    assert np.allclose(right["normal"][0], w / np.linalg.norm(w), rtol=1e-12)
    assert abs(right["normal"][0] @ nrm) < 1e-12
