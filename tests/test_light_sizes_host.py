"""The host side of the light tables at the sizes where the device code changes form (tests/light_shapes.py): for
every case the CDF that HostScene.update_lights() builds after the emission was switched on, against a plain float32 model of the
operation (light_shapes.model_cdf), against the same scene loaded afresh, and against what the reference's own make_lights printed
(tests/golden/light_sizes_stats.json); and the CPU restatement of sample_lights / sample_lights_pdf against the reference's answers
on records that sit on the borders of the CDF index (tests/golden/light_sizes_kat.npz).  No device."""
import json
import os

import numpy as np
import pytest

import kat_lib as K
import light_edits as L
import light_shapes as S
import oracle_lib
from conftest import GOLDEN

F = np.float32
ALL = list(S.CASES) + ["several"]


def case_of(name):
    return "several" if name == "several" else S.CASES[name]


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """name -> (path of the scene as it starts, path of the scene written with the emission on); written once"""
    cache = {}

    def get(name):
        if name not in cache:
            d = tmp_path_factory.mktemp(name.replace("-", "_"))
            cache[name] = (S.write_scene(d, case_of(name)), S.write_scene(d, case_of(name), on=True))
        return cache[name]
    return get


def fixture_stats():
    return json.load(open(os.path.join(GOLDEN, "light_sizes_stats.json")))


@pytest.fixture(scope="module")
def tables():
    return np.load(os.path.join(GOLDEN, "light_sizes_kat.npz"))


def edited(vpt, scenes, name):
    h = vpt.HostScene(scenes(name)[0])
    before = L.lights_of(h.stats())
    S.edit(case_of(name))(h)
    assert not h.update_lights().empty()
    assert L.lights_of(h.stats()) != before
    return h


def cdf_of(host, light):
    lights, cdf = host.lights()
    return cdf[int(lights[light]["cdf_offset"]):][:int(lights[light]["cdf_len"])]


def test_the_cases_are_the_ones_the_kernels_change_form_at():
    """the list itself: every size group, both element kinds at 4 / 65 / 257 / 4097, every index depth from 2 to 5 levels"""
    n_of = lambda pattern, quads=False: sorted(c.n for c in S.CASES.values() if c.pattern == pattern and c.quads == quads)   # noqa: E731
    assert n_of("varied") == [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 65536, 65537]
    assert n_of("varied", True) == [4, 65, 257, 4097] and n_of("plateaus") == [65, 257, 4097]
    assert sorted((c.n, c.total) for c in S.CASES.values() if c.pattern == "tiny") == [(65, 5e-6), (65, 2e-5), (4097, 5e-6), (4097, 2e-5)]
    assert n_of("all_zero") == [65]
    assert {S.CASES[f"tri_{n}_varied"].levels() for n in (65, 256)} == {2} and S.CASES["tri_257_varied"].levels() == 3
    assert [S.CASES[f"tri_{n}_varied"].levels() for n in (4096, 4097, 65536, 65537)] == [3, 4, 4, 5]
    assert [(c.n, c.quads) for c in S.SEVERAL] == [(3, False), (65, True), (130, False), (4097, True)]
    assert set(ALL) == set(fixture_stats())


@pytest.mark.parametrize("name", list(S.CASES))
def test_geometry_keeps_every_element_in_its_cell(name):
    case = S.CASES[name]
    verts, faces = S.geometry(case)
    side = int(np.ceil(np.sqrt(case.n)))
    pitch = max(1.0 / side, S.MIN_PITCH)
    assert pitch >= 1.0 / 256
    p = verts[faces].astype(np.float64)   # (n, k, 3)
    i = np.arange(case.n)
    lo = np.stack([(i // side) * pitch, (i % side) * pitch], 1)
    assert (p[..., :2] > lo[:, None, :]).all() and (p[..., :2] < lo[:, None, :] + pitch).all() and (p[..., 2] == 0).all()
    assert p[..., :2].min() > 0 and p[..., :2].max() < (1 if case.n <= 65536 else 1 + pitch)
    areas = S.model_areas(verts, faces)
    dead = areas == 0
    if case.pattern == "varied":
        assert not dead.any() and (case.n < 63 or areas.max() / areas.min() > 300)
    if case.pattern == "plateaus":
        start = case.run_start
        assert start % 16 == 0 and dead[start:start + S.RUN].all() and not dead[start - 1] and not dead[start + S.RUN + 1] and dead[::4].all() and dead[0] and dead[-1]
        assert (~dead).sum() > case.n // 2
    if case.pattern == "tiny":
        assert abs(float(S.model_cdf(verts, faces)[-1]) / case.total - 1) < 1e-3
        assert (case.total < 1e-5) == (F(S.model_cdf(verts, faces)[-1]) - F(0.00001) < 0)
    if case.pattern == "all_zero":
        assert dead.all()


@pytest.mark.parametrize("name", ALL)
def test_update_lights_equals_the_model_the_fresh_scene_and_the_reference(vpt, scenes, name):
    h = edited(vpt, scenes, name)
    lights, cdf = h.lights()
    under_test = S.lights_under_test(case_of(name))
    assert len(lights) == (4 if name == "several" else 2)
    for light, case in under_test.items():
        assert int(lights[light]["cdf_len"]) == case.n and int(lights[light]["instance"]) == 2 + (light if name == "several" else 0)
        positions, elements = S.shape_of_light(h, light)
        assert elements.shape == (case.n, 4 if case.quads else 3)
        origin = (1.25 * (light % 2), 1.25 * (light // 2)) if name == "several" else (0.0, 0.0)
        assert positions[elements].tobytes() == S.geometry(case, origin)[0].reshape(case.n, -1, 3).tobytes()   # the file round trip
        want = S.model_cdf(positions, elements)
        got = cdf_of(h, light)
        assert got.tobytes() == want.tobytes(), (name, light, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    fresh = vpt.HostScene(scenes(name)[1])
    assert lights.tobytes() == fresh.lights()[0].tobytes() and cdf.tobytes() == fresh.lights()[1].tobytes()
    assert L.lights_of(h.stats()) == L.lights_of(fresh.stats()) == fixture_stats()[name]["lights"]


@pytest.mark.parametrize("name", S.NUDGED)
def test_moved_vertices_equal_the_model(vpt, scenes, name):
    """the recompute of a light that already exists: x * 1.25 over the test shape of the scene with the emission on"""
    h = vpt.HostScene(scenes(name)[1])
    before = cdf_of(h, 1).copy()
    S.nudge(scenes(name)[1], S.CASES[name])(h)
    assert not h.update_lights().empty()
    got = cdf_of(h, 1)
    assert got.tobytes() == S.model_cdf(*S.shape_of_light(h, 1)).tobytes()
    assert (got != before).all()


def test_the_comparison_sees_an_off_by_one_in_the_model(vpt, scenes):
    """two wrong models - the quad's second triangle taken at (p2, p3, p0), the running sum started at 0 - differ from the host's CDF"""
    h = edited(vpt, scenes, "quad_65_varied")
    p, q = S.shape_of_light(h, 1)
    got = cdf_of(h, 1)
    assert got.tobytes() == S.model_cdf(p, q).tobytes()
    shifted = (S._triangle_area(p[q[:, 0]], p[q[:, 1]], p[q[:, 3]]) + S._triangle_area(p[q[:, 2]], p[q[:, 3]], p[q[:, 0]])).astype(F)
    assert np.add.accumulate(shifted, dtype=F).tobytes() != got.tobytes()
    from_zero = np.concatenate([[F(0)], np.add.accumulate(S.model_areas(p, q), dtype=F)[:-1]]).astype(F)
    assert from_zero.tobytes() != got.tobytes()


def test_reference_stats_are_what_the_reference_prints_now(scenes, tmp_path):
    """wherever oracle/_ref is built: the committed `lights` sections are regenerated from the reference's driver and must be unchanged"""
    if not oracle_lib.have_reference() or not os.path.exists(oracle_lib.REF_DRIVER):
        pytest.skip("oracle/_ref/ref_driver not built; the fixture is committed data")
    want = fixture_stats()
    for name in ALL:
        assert S.reference_lights(scenes(name)[1], tmp_path) == want[name]["lights"], name


# ---- known-answer tables -------------------------------------------------------------------------------------------------------------
def test_kat_file_is_small_and_complete(tables):
    assert os.path.getsize(os.path.join(GOLDEN, "light_sizes_kat.npz")) < 500_000
    assert set(tables.files) == {f"{n}_{t}" for n in S.KAT_CASES for t in ("sl_in", "sl_out", "pdf_in", "pdf_out")}
    assert {"tri_4_varied", "tri_5_varied", "tri_64_varied", "tri_65_varied", "tri_257_varied", "tri_4097_varied", "tri_65_plateaus", "tri_257_plateaus",
            "tri_4097_plateaus", "tri_65_tiny_5e-6", "tri_65_tiny_2e-5", "tri_4097_tiny_5e-6", "tri_4097_tiny_2e-5", "tri_65_all_zero"} == set(S.KAT_CASES)


@pytest.mark.parametrize("name", S.KAT_CASES)
def test_kat_records_are_the_generators(vpt, scenes, tables, name):
    """the committed records are light_shapes.sample_records / pdf_records of the host's CDF: half of the `rel` values on and beside
    the entries of border_ks, half of the pdf directions the reference's sampled ones"""
    case = S.CASES[name]
    h = vpt.HostScene(scenes(name)[1])
    cdf = cdf_of(h, 1)
    sl = S.sample_records(case, cdf, 1, 2)
    assert sl.shape == (S.KAT_RECORDS, 7) and sl.tobytes() == tables[name + "_sl_in"].tobytes()
    assert S.pdf_records(case, sl, tables[name + "_sl_out"]).tobytes() == tables[name + "_pdf_in"].tobytes()
    assert (np.abs(sl[:, 2]) >= 0.5).all() and (np.abs(sl[:, 2]) <= 2).all()
    if cdf[-1] > 0:
        on_entries = {float(F(cdf[k] / cdf[-1])) for k in S.border_ks(case)}
        assert len(on_entries & set(sl[::2, 4].tolist())) >= len(on_entries) - 1   # all but a 1.0, which is clamped under 1
        assert (np.minimum((sl[::2, 3] * 2).astype(int), 1) == 1).all()


@pytest.mark.parametrize("name", S.KAT_CASES)
def test_oracle_reproduces_the_reference_tables(vpt, oracle, scenes, tables, name):
    h = vpt.HostScene(scenes(name)[1])
    for op, iparam, key in (("sample_lights", 0, "sl"), ("lights_pdf", 450, "pdf")):
        got = K.run_oracle(oracle, h, op, iparam, tables[f"{name}_{key}_in"])
        ok = K.bits_equal(got, tables[f"{name}_{key}_out"])
        assert ok.all(), (name, op, np.argwhere(~ok)[:5].tolist())


def test_kat_tables_are_what_the_reference_returns_now(scenes, tables):
    if not K.have_reference():
        pytest.skip("oracle/_ref/ref_tables not built; the tables are committed data")
    for name in S.KAT_CASES:
        for op, iparam, key in (("sample_lights", 0, "sl"), ("lights_pdf", 450, "pdf")):
            out = S.run_reference(scenes(name)[1], op, iparam, tables[f"{name}_{key}_in"])
            assert K.bits_equal(out, tables[f"{name}_{key}_out"]).all(), (name, op)


def aims_at(case, rec, direction):
    """element whose cell the ray {position, direction} crosses the plane z = 0 in (-1: outside the lattice), per record"""
    side = int(np.ceil(np.sqrt(case.n)))
    pitch = max(1.0 / side, S.MIN_PITCH)
    o, d = rec[:, 0:3].astype(np.float64), direction.astype(np.float64)
    t = -o[:, 2] / d[:, 2]
    xy = o[:, :2] + d[:, :2] * t[:, None]
    cell = np.floor(xy / pitch).astype(np.int64)
    inside = (cell >= 0).all(1) & (cell < side).all(1) & (t > 0)
    return np.where(inside, cell[:, 0] * side + cell[:, 1], -1), xy


@pytest.mark.parametrize("name", [n for n in S.KAT_CASES if "tiny" in n])
def test_tiny_tables_show_the_references_behaviour(tables, name):
    """total area under 1e-5: sample_discrete clamps every sample to back - 0.00001f < 0 and upper_bound returns 0 - every record that
    selects the test light aims inside element 0.  Just over it (2e-5) the clamp cuts the range in half: other elements are sampled,
    none past the entry at back - 0.00001f."""
    case = S.CASES[name]
    rec, out = tables[name + "_sl_in"], tables[name + "_sl_out"]
    test_light = np.minimum((rec[:, 3] * 2).astype(int), 1) == 1
    assert test_light.sum() > S.KAT_RECORDS // 2
    element, xy = aims_at(case, rec[test_light], out[test_light])
    verts, faces = S.geometry(case)
    if case.total < 1e-5:
        box = verts[faces[0]].astype(np.float64)[:, :2]
        assert (element == 0).all()
        assert (xy >= box.min(0) - 1e-6).all() and (xy <= box.max(0) + 1e-6).all()
    else:
        cdf = S.model_cdf(verts, faces)
        last = int(np.searchsorted(cdf, cdf[-1] - F(0.00001), side="right"))
        assert (element >= 0).all() and len(set(element.tolist())) > 8 and element.max() <= last < case.n - 1


@pytest.mark.parametrize("name", [n for n in S.KAT_CASES if "tiny" not in n and "zero" not in n])
def test_border_records_select_the_bordering_elements(tables, name):
    """the `rel` values on CDF entries select the element AFTER the entry (upper_bound), those just under it the element itself or,
    among equal entries, the first element after the tie - as the plain model's searchsorted says, for the reference's directions"""
    case = S.CASES[name]
    verts, faces = S.geometry(case)
    cdf = S.model_cdf(verts, faces)
    rec, out = tables[name + "_sl_in"][::2], tables[name + "_sl_out"][::2]
    r = np.minimum(np.maximum((rec[:, 4] * cdf[-1]).astype(F), F(0)), cdf[-1] - F(0.00001))
    want = np.minimum(np.searchsorted(cdf, r, side="right"), case.n - 1)
    element, _ = aims_at(case, rec, out)
    assert (element == want).all(), (name, np.argwhere(element != want)[:5].tolist())
    assert S.model_areas(verts, faces)[want].min() > 0   # a degenerate element is never selected
