"""The light tables on the GPU at the sizes where the code changes form (tests/light_shapes.py): vpt_light_update.hip's
kernels (areas, the 64-lane running sum, index levels, guide table), build_lights on the host and search_light_cdf in the kernels.
Per case A = DeviceScene(scene as it starts) with update_lights(emission on), B = DeviceScene(the host scene after the same edit).
The light list and CDF of A are the host mirror's byte for byte - which tests/test_light_sizes_host.py ties to the plain model and to
the reference's make_lights - the six table hashes are B's, the search structure equals the plain binary search, the `indexed` figure
is what the documented rule gives, sample_lights / sample_lights_pdf return the reference's answers on records that sit on the borders
of the index groups, and renders are B's bit for bit.

The known answers are the committed tables of tests/golden/light_sizes_kat.npz (the reference's own functions) where a case has them,
and the CPU restatement's answers (oracle: it reproduces the committed tables bit for bit, test_light_sizes_host.py) on the same kind
of records elsewhere.  The tolerance is test_kat.TOLERANCE as it stands with a share of 1.0; on top of it the three ops are held to the
reference's bits (check_kat)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kat_lib as K
import light_shapes as S
from conftest import GOLDEN, ROOT
from test_kat import TOLERANCE
from test_light_update_gpu import assert_same_lights
from test_scene_update_gpu import assert_same_bvh, same_state

pytestmark = pytest.mark.gpu

ALL = list(S.CASES) + ["several"]


def case_of(name):
    return "several" if name == "several" else S.CASES[name]


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    cache = {}

    def get(name, on=False):
        if (name, on) not in cache:
            cache[name, on] = S.write_scene(tmp_path_factory.mktemp(name.replace("-", "_")), case_of(name), on=on)
        return cache[name, on]
    return get


@pytest.fixture(scope="module")
def tables():
    return np.load(os.path.join(GOLDEN, "light_sizes_kat.npz"))


def render(vpt, dev, host, shader):
    p = vpt.PathtraceParams(resolution=32, samples=4, shader=shader, bounces=4)
    st = host.make_state(p)
    dev.pathtrace_samples(st, p, 4)
    return st


def close_share(op, got, ref):
    """(share within test_kat.TOLERANCE[op], exact share, worst ulp distance); NaN equals NaN (kat_lib.ulp_distance, as bits_equal)"""
    ulps, rel, _ = TOLERANCE[op]
    d = K.ulp_distance(got, ref)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)
        close = (d <= ulps) | (err <= np.maximum(rel * np.abs(ref), 1e-6 * np.maximum(1.0, np.abs(ref))))
    return float(close.mean()), float(K.bits_equal(got, ref).mean()), int(d.max())


def check_kat(oracle, tables, dev, host, name, light, case, what):
    """sample_lights, lights_pdf and lights_pdf_k2 of `dev` against the known answers: share 1.0, nothing left out"""
    lights, cdf = host.lights()
    if name in S.KAT_CASES:
        sl, aimed, pdf, pdf_ref = (tables[f"{name}_{t}"] for t in ("sl_in", "sl_out", "pdf_in", "pdf_out"))
    else:
        sl = S.sample_records(case, cdf[int(lights[light]["cdf_offset"]):][:case.n], light, len(lights))
        aimed = K.run_oracle(oracle, host, "sample_lights", 0, sl)
        pdf = S.pdf_records(case, sl, aimed)
        pdf_ref = K.run_oracle(oracle, host, "lights_pdf", 450, pdf)
    for op, rec, ref, iparam in (("sample_lights", sl, aimed, 0), ("lights_pdf", pdf, pdf_ref, 450), ("lights_pdf_k2", pdf, pdf_ref, 450)):
        got = dev.kat(K.OPS[op][0], rec, iparam)
        share, exact, worst = close_share("lights_pdf" if op == "lights_pdf_k2" else op, got, ref)
        print(f"KAT {what} {name} light {light} {op}: within tolerance {share:.5f}, exact {exact:.5f}, worst ulp distance {worst}", flush=True)
        assert share == 1.0, (what, name, light, op, share, worst)
        # These scenes have no environment, so no libm call is on either path: sample_lights is sqrt and division (correctly rounded on
        # both sides), sample_lights_pdf an exact intersection and + * /.  Measured on MI355X: every record of every case exact.
        assert exact == 1.0, (what, name, light, op, exact, worst)


def check_lights(vpt, oracle, tables, A, B, host, name):
    assert_same_lights(A, B, host, name)
    assert_same_bvh(A, host, name)
    for light, case in S.lights_under_test(case_of(name)).items():
        for what, dev in (("updated", A), ("fresh", B)):
            assert dev.selftest_light_cdf(light, 1 << 16) == (0, case.indexed()), (name, what, light)
            check_kat(oracle, tables, dev, host, name, light, case, what)
    for shader in ("pathtrace", "eyelight"):
        assert same_state(render(vpt, A, host, shader), render(vpt, B, host, shader)), f"{name}: {shader} differs from the fresh scene's render"


def updated_pair(vpt, scenes, name):
    A = vpt.DeviceScene(vpt.HostScene(scenes(name)), 0)
    host = vpt.HostScene(scenes(name))
    S.edit(case_of(name))(host)
    what = host.update_lights()
    assert not what.empty()
    A.update_lights(what)
    return A, vpt.DeviceScene(host, 0), host


@pytest.mark.parametrize("name", list(S.CASES))
def test_a_light_of_this_size_equals_a_fresh_scene(vpt, oracle, scenes, tables, name):
    A, B, host = updated_pair(vpt, scenes, name)
    lights, _ = A.get_lights()
    assert len(lights) == 2 and int(lights[1]["cdf_len"]) == S.CASES[name].n
    check_lights(vpt, oracle, tables, A, B, host, name)
    C = vpt.DeviceScene(vpt.HostScene(scenes(name)), 0)   # the edit is not a no-op
    assert A.light_tables_hash() != C.light_tables_hash()


def test_several_lights_in_one_edit(vpt, oracle, scenes, tables):
    """four emitters on and the lamp off in one edit: one lit_areas_kernel launch with four jobs of 3 / 65 / 130 / 4 097 elements,
    triangles and quads mixed, and every offset rebased.  Launches (vpt_light_update.hip: light_update_apply; the edit has materials
    only, so vpt_scene_update.hip launches nothing before it): 1 areas (all jobs on grid.y, < 65 535 of them) + 1 running sum (a wave per
    job) + per recomputed light with n > 64 one for the index levels and one for the guide table (65, 130, 4 097: 3 x 2; the 3-triangle
    light has no index) + 1 for the light records = 9."""
    A, B, host = updated_pair(vpt, scenes, "several")
    lights, _ = A.get_lights()
    assert [int(l["cdf_len"]) for l in lights] == [3, 65, 130, 4097] and [int(l["instance"]) for l in lights] == [2, 3, 4, 5]
    indexed_jobs = sum(1 for c in S.SEVERAL if c.n > 64)
    assert A.update_stats()[0] == 1 + 1 + 2 * indexed_jobs + 1 == 9
    check_lights(vpt, oracle, tables, A, B, host, "several")


@pytest.mark.parametrize("name", S.NUDGED)
def test_moved_vertices_of_a_light_that_exists(vpt, oracle, scenes, tables, name):
    """x * 1.25 over the test shape of a scene whose emitter is already on: the recompute path for a light that stays in the list"""
    on = scenes(name, on=True)
    A = vpt.DeviceScene(vpt.HostScene(on), 0)
    host = vpt.HostScene(on)
    before = A.light_tables_hash()
    S.nudge(on, S.CASES[name])(host)
    A.update_lights(host.update_lights())
    B = vpt.DeviceScene(host, 0)
    assert A.light_tables_hash() != before
    got = A.get_lights()[1][1:]   # the lamp's one entry, then the test light's
    assert got.tobytes() == S.model_cdf(*S.shape_of_light(host, 1)).tobytes()
    case = S.CASES[name]
    moved = S.Case(name + "_moved", case.n)   # no committed tables for the moved shape: the restatement's answers
    assert_same_lights(A, B, host, name)
    assert_same_bvh(A, host, name)
    for what, dev in (("updated", A), ("fresh", B)):
        assert dev.selftest_light_cdf(1, 1 << 16) == (0, case.indexed())
        check_kat(oracle, tables, dev, host, moved.name, 1, moved, what)
    for shader in ("pathtrace", "eyelight"):
        assert same_state(render(vpt, A, host, shader), render(vpt, B, host, shader)), (name, shader)


@pytest.mark.parametrize("n", S.LEVEL_BORDERS)
def test_fresh_scene_at_a_level_border(vpt, oracle, scenes, tables, n):
    """no update at all: build_lights and search_light_cdf on a scene created with the emitter on, pinned without the update kernels"""
    name = f"tri_{n}_varied"
    host = vpt.HostScene(scenes(name, on=True))
    B = vpt.DeviceScene(host, 0)
    lights, cdf = B.get_lights()
    assert lights.tobytes() == host.lights()[0].tobytes() and cdf.tobytes() == host.lights()[1].tobytes()
    assert B.selftest_light_cdf(1, 1 << 16) == (0, 2)
    check_kat(oracle, tables, B, host, name, 1, S.CASES[name], "fresh only")


@pytest.mark.parametrize("name", S.PLAIN)
def test_the_plain_running_sum_gives_the_same_bits(name):
    """VPT_LIGHTS_PLAIN=1: the one-lane chain in place of the 64-lane form, in a child process as test_switches_keep_the_equality"""
    test = "test_several_lights_in_one_edit" if name == "several" else f"test_a_light_of_this_size_equals_a_fresh_scene[{name}]"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", f"{__file__}::{test}"],
                       env=dict(os.environ, VPT_LIGHTS_PLAIN="1"), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
