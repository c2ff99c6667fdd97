"""Deterministic emitters of a chosen length, for the places where the light tables change form: the 64-lane blocks
of the running sum, the n > 64 threshold of the CDF index, the lengths at which the 16-ary index gains a level (17, 257, 4 097,
65 537), the one-leaf shapes of 1..4 primitives that are walked inline, ties between CDF entries, and lights whose total area is
under sample_discrete's 1e-5.  Shared by tests/test_light_sizes_host.py, tests/test_light_sizes_gpu.py and the fixture script
tests/golden/make_light_size_fixtures.py.

A case is a scene (synth_scenes._Writer: OBJ shapes, no environment) of
  instance 0   a floor quad at z = -0.75;
  instance 1   a one-quad lamp at z = 2.5, emissive from the start: a light that stays and is moved device to device;
  instance 2   the test shape: n triangles or quads at z = 0, element i in cell (i // side, i % side) of a side x side lattice
               over the unit square, side = ceil(sqrt(n)).  Its material starts without emission and is switched on (edit()).
The lattice pitch is 1 / side and never under 1 / 256; every element keeps 5 % of the pitch clear of its cell's border, so a search
that returns a neighbour of the right element moves a sampled direction by more than 1e-3 at the distances of query_points (0.5
to 2 from the square), far above any tolerance.  n = 65 537 needs 257 columns: at the pitch of 1 / 256 its lattice overhangs the
unit square by one cell.

Area patterns (numpy default_rng seeded from the case, float32 vertices, written with repr by the _Writer):
  varied     the leg of element i is 0.9 pitch * 10^(-1.5 u_i), u_i uniform: areas over three decades
  plateaus   varied, with every fourth element degenerate (all vertices equal: area +0, equal consecutive CDF entries), the first
             and the last among them, and a run of 20 consecutive degenerate elements that starts on a multiple of 16 (a whole group
             of the index with one value; the element after it is a fourth one, so 21 entries are equal)
  tiny       varied, scaled to a total area of 5e-6 (back - 0.00001f < 0: every sample is clamped below zero) or 2e-5 (just on
             the safe side)
  all_zero   every element degenerate: back == 0, an index without a guide table
`several` is one scene with four test shapes (3 triangles, 65 quads, 130 triangles, 4 097 quads, instances 2..5) that one edit
switches on while it switches the lamp off."""
import math
import os
import zlib

import numpy as np

import light_edits
import synth_scenes

F = np.float32
MIN_PITCH = 1.0 / 256
LAMP, TEST = 2, 4                       # material ids: _Writer's lamp_small; the first test material
ON = (3.0, 2.5, 2.0)
RUN = 20                                # length of the plateaus' run of degenerate elements


class Case:
    def __init__(self, name, n, quads=False, pattern="varied", total=None):
        self.name, self.n, self.quads, self.pattern, self.total = name, n, quads, pattern, total

    @property
    def run_start(self):
        """first element of the 20-run of `plateaus`: a multiple of 16 near the middle"""
        return 16 * (self.n // 32)

    def indexed(self):
        """what vpt_selftest_light_cdf reports by the rule of vpt_device.h / build_lights: 0 no index (n <= 64), 2 index levels and
        guide table (n > 64, back > 0, n / 4 >= 16), 1 levels alone (back == 0)"""
        return 0 if self.n <= 64 else 1 if self.pattern == "all_zero" else 2

    def levels(self):
        """levels of the 16-ary index, level 0 (the CDF) included: one more at 17, 257, 4 097, 65 537"""
        size, levels = self.n, 1
        while size > 16:
            size, levels = (size + 15) // 16, levels + 1
        return levels


SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 65536, 65537)
LEVEL_BORDERS = (255, 256, 257, 4095, 4096, 4097, 65536, 65537)
_cases = [Case(f"tri_{n}_varied", n) for n in SIZES]
_cases += [Case(f"quad_{n}_varied", n, quads=True) for n in (4, 65, 257, 4097)]
_cases += [Case(f"tri_{n}_plateaus", n, pattern="plateaus") for n in (65, 257, 4097)]
_cases += [Case(f"tri_{n}_tiny_{tag}", n, pattern="tiny", total=total) for n in (65, 4097) for tag, total in (("5e-6", 5e-6), ("2e-5", 2e-5))]
_cases += [Case("tri_65_all_zero", 65, pattern="all_zero")]
CASES = {c.name: c for c in _cases}
SEVERAL = (Case("several_tri_3", 3), Case("several_quad_65", 65, quads=True), Case("several_tri_130", 130), Case("several_quad_4097", 4097, quads=True))
# the cases with committed known-answer tables (tests/golden/light_sizes_kat.npz)
KAT_CASES = [f"tri_{n}_varied" for n in (4, 5, 64, 65, 257, 4097)] + [c.name for c in _cases if c.pattern != "varied"]
NUDGED = ("tri_64_varied", "tri_65_varied", "tri_129_varied", "tri_4097_varied")
PLAIN = ("tri_63_varied", "tri_64_varied", "tri_65_varied", "tri_129_varied", "tri_65_plateaus", "several")


def _seed(name):
    return zlib.crc32(name.encode())


def geometry(case, origin=(0.0, 0.0)):
    """(vertices (n * k, 3) float32, faces (n, k)) of a case's test shape, k = 3 or 4; element i owns vertices k i .. k i + k - 1"""
    rng = np.random.default_rng(_seed(case.name))
    n, k = case.n, 4 if case.quads else 3
    side = max(1, math.ceil(math.sqrt(n)))
    pitch = max(1.0 / side, MIN_PITCH)
    i = np.arange(n)
    corner = np.stack([(i // side) * pitch + 0.05 * pitch + origin[0], (i % side) * pitch + 0.05 * pitch + origin[1]], 1)   # float64
    leg = 0.9 * pitch * 10.0 ** (-1.5 * rng.random(n))
    j = 0.5 * rng.random((n, 3))
    # a right triangle with jittered far corners, or a convex quad, in units of the leg
    unit = np.zeros((n, k, 2))
    unit[:, 1] = np.stack([np.ones(n), j[:, 0]], 1)
    if case.quads:
        unit[:, 2] = np.stack([1 - 0.4 * j[:, 2], 1 - 0.4 * j[:, 2]], 1)
        unit[:, 3] = np.stack([j[:, 1], np.ones(n)], 1)
    else:
        unit[:, 2] = np.stack([j[:, 1], np.ones(n)], 1)
    if case.pattern == "tiny":   # the total of the exact areas := case.total; the float32 sums are checked against it by the tests
        x, y = unit[..., 0] * leg[:, None], unit[..., 1] * leg[:, None]
        exact = 0.5 * np.abs(np.sum(x * np.roll(y, -1, 1) - np.roll(x, -1, 1) * y, 1)).sum()   # shoelace
        leg = leg * math.sqrt(case.total / exact)
    dead = np.zeros(n, bool)
    if case.pattern == "plateaus":
        dead[::4] = True
        dead[0] = dead[n - 1] = True
        dead[case.run_start:case.run_start + RUN] = True
    elif case.pattern == "all_zero":
        dead[:] = True
    leg = np.where(dead, 0.0, leg)
    xy = corner[:, None, :] + unit * leg[:, None, None]
    verts = np.concatenate([xy, np.zeros((n, k, 1))], 2).reshape(n * k, 3).astype(F)
    return verts, np.arange(n * k).reshape(n, k)


def _identity(o=(0, 0, 0)):
    return np.concatenate([np.eye(3).reshape(-1), o])


def write_scene(dirpath, case, on=False):
    """the scene of one case (or of `several`, case = "several") under dirpath; on: written with the emission already switched (what
    the edit leads to).  Returns the path; the two variants share their shape files."""
    w = synth_scenes._Writer(dirpath)
    shapes = SEVERAL if case == "several" else (case,)
    for s, c in enumerate(shapes):
        w.materials.append({"name": f"test{s}", "type": "matte", "color": [0, 0, 0], **({"emission": list(ON)} if on else {})})
    if case == "several" and on:
        del w.materials[LAMP]["emission"]
    floor = w.shape("floor", [[-3, -3, 0], [4, -3, 0], [4, 4, 0], [-3, 4, 0]], [[0, 1, 2, 3]])
    lamp = w.shape("lamp", [[0.25, 0.25, 0], [0.25, 0.75, 0], [0.75, 0.75, 0], [0.75, 0.25, 0]], [[0, 1, 2, 3]])   # faces down
    w.instance(floor, _identity((0, 0, -0.75)), 0)
    w.instance(lamp, _identity((0, 0, 2.5)), LAMP)
    for s, c in enumerate(shapes):
        origin = (1.25 * (s % 2), 1.25 * (s // 2)) if case == "several" else (0.0, 0.0)
        w.instance(w.shape(c.name, *geometry(c, origin)), _identity(), TEST + s)
    name = (case if case == "several" else case.name) + ("_on" if on else "")
    path, _ = w.write(name, synth_scenes._look_at([0.5, -2.5, 2.0], [0.5, 0.5, 0.0]), env=0)
    return path


def edit(case):
    """the edit that leads from write_scene(.., on=False) to write_scene(.., on=True)"""
    if case == "several":
        return light_edits.several(*[lambda h, s=s: light_edits.emit(h, TEST + s, ON) for s in range(len(SEVERAL))], lambda h: light_edits.emit(h, LAMP, (0.0, 0.0, 0.0)))
    return lambda h: light_edits.emit(h, TEST, ON)


def nudge(scene_path, case):
    """light_edits.nudge_shape with stretch over the test shape: every area changes"""
    return light_edits.nudge_shape(scene_path, case.name, light_edits.stretch)


def lights_under_test(case):
    """{light id: Case} of the test shapes in the "on" scene: the lamp is light 0 (instance 1), the test shape light 1 (instance 2);
    in `several` the lamp is off and the four shapes are lights 0..3"""
    return dict(enumerate(SEVERAL)) if case == "several" else {1: case}


# ---- the plain model of the operation ------------------------------------------------------------------------------------------------
def _triangle_area(p0, p1, p2):
    """length(cross(p1 - p0, p2 - p0)) / 2 (yocto_geometry.h:506-510, yocto_math.h:1610-1617), one float32 operation at a time"""
    a, b = (p1 - p0).astype(F), (p2 - p0).astype(F)
    mul = lambda x, y: (x * y).astype(F)   # noqa: E731
    c = [(mul(a[:, 1], b[:, 2]) - mul(a[:, 2], b[:, 1])).astype(F), (mul(a[:, 2], b[:, 0]) - mul(a[:, 0], b[:, 2])).astype(F),
         (mul(a[:, 0], b[:, 1]) - mul(a[:, 1], b[:, 0])).astype(F)]
    d = ((mul(c[0], c[0]) + mul(c[1], c[1])).astype(F) + mul(c[2], c[2])).astype(F)
    return (np.sqrt(d).astype(F) / F(2)).astype(F)


def model_areas(positions, elements):
    p = np.asarray(positions, F)
    q = np.asarray(elements)
    if q.shape[1] == 3:
        return _triangle_area(p[q[:, 0]], p[q[:, 1]], p[q[:, 2]])
    return (_triangle_area(p[q[:, 0]], p[q[:, 1]], p[q[:, 3]]) + _triangle_area(p[q[:, 2]], p[q[:, 3]], p[q[:, 1]])).astype(F)   # quad_area, :512-518


def model_cdf(positions, elements):
    """the element CDF make_lights builds: cdf[0] = area_0, cdf[i] = area_i + cdf[i - 1] in float32 (np.add.accumulate is that serial
    chain).  Guards itself: the last entry agrees with the float64 sum of float64 areas to n 2^-24 relative, the forward bound of a
    serial float32 sum of non-negative terms (plus 8 ulp for the float32 areas themselves)."""
    cdf = np.add.accumulate(model_areas(positions, elements), dtype=F)
    p, q = np.asarray(positions, np.float64), np.asarray(elements)
    area = lambda a, b, c: 0.5 * np.linalg.norm(np.cross(p[b] - p[a], p[c] - p[a]), axis=1)   # noqa: E731
    exact = (area(q[:, 0], q[:, 1], q[:, 2]) if q.shape[1] == 3 else area(q[:, 0], q[:, 1], q[:, 3]) + area(q[:, 2], q[:, 3], q[:, 1])).sum()
    assert abs(float(cdf[-1]) - exact) <= (len(q) + 8) * 2.0 ** -24 * exact, (float(cdf[-1]), exact)
    return cdf


def shape_of_light(host, light):
    """(positions, elements) of the shape behind entry `light` of host.lights()"""
    lights, _ = host.lights()
    a = host.shape_arrays(host.instance_ids(int(lights[light]["instance"]))[0])
    return a["positions"], a["triangles"] if len(a["triangles"]) else a["quads"]


# ---- the reference's tables on a scene file ------------------------------------------------------------------------------------------
def run_reference(scene_path, op_name, iparam, records):
    """kat_lib.run_reference for a scene given by its path (oracle/_ref/ref_tables must be built)"""
    import subprocess
    import tempfile
    import kat_lib
    op, si, so = kat_lib.OPS[op_name]
    records = np.ascontiguousarray(records, F)
    assert records.shape[1] == si
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        records.tofile(fin)
        subprocess.check_call([kat_lib.REF_TABLES, scene_path, str(op), str(iparam), fin, fout])
        return np.fromfile(fout, F).reshape(records.shape[0], so)


def reference_lights(scene_path, workdir):
    """the `lights` section of the reference driver's --stats for a scene file (oracle/_ref/ref_driver must be built)"""
    import json
    import subprocess
    import oracle_lib
    stats = os.path.join(str(workdir), "stats.json")
    subprocess.check_call([oracle_lib.REF_DRIVER, "--scene", scene_path, "--shader", "eyelight", "--resolution", "16", "--samples", "1", "--stats", stats,
                           "--state", os.path.join(str(workdir), "state.bin")], stdout=subprocess.DEVNULL)
    return json.load(open(stats))["lights"]


# ---- known-answer records ------------------------------------------------------------------------------------------------------------
KAT_RECORDS = 512
LO, HI = (-0.5, -0.5, 0.5), (1.5, 1.5, 2.0)


def query_points(rng, n):
    """points 0.5 to 2 above or under the square (|z| >= 0.5), over it and up to 0.5 beside it"""
    p = rng.uniform(LO, HI, size=(n, 3))
    p[rng.random(n) < 0.5, 2] *= -1
    return p.astype(F)


def border_ks(case):
    """CDF entries whose neighbourhood the records probe: the ends of the first index group, of the first 256, of the CDF, and of
    the plateaus' 20-run"""
    ks = [0, 14, 15, 16, 17, 255, 256, 257, case.n - 2, case.n - 1]
    if case.pattern == "plateaus":
        ks += [case.run_start, case.run_start + RUN - 1]
    return sorted({k for k in ks if 0 <= k < case.n})


def sample_records(case, cdf, light, num_lights):
    """KAT_RECORDS sample_lights records {position, rl, rel, ruv} (kat_lib.gen_sample_lights); in every second one `rel` is
    float32(cdf[k] / back) or one of its two float neighbours, k from border_ks, and `rl` selects the test light"""
    import kat_lib
    rng = np.random.default_rng(_seed(case.name) ^ 0x5EED)
    rec = kat_lib.gen_sample_lights(rng, LO, HI, KAT_RECORDS)
    rec[:, 0:3] = query_points(rng, KAT_RECORDS)
    back = cdf[-1]
    if back > 0:
        ks = border_ks(case)
        for slot, r in enumerate(range(0, KAT_RECORDS, 2)):
            v = F(cdf[ks[(slot // 3) % len(ks)]] / back)
            v = (np.nextafter(v, F(-1)), v, np.nextafter(v, F(2)))[slot % 3]
            rec[r, 4] = min(max(v, F(0)), F(1 - 2.0 ** -24))
            rec[r, 3] = F((light + 0.5) / num_lights)
    return np.ascontiguousarray(rec, F)


def pdf_records(case, samples, aimed):
    """KAT_RECORDS lights_pdf records {position, direction}: the positions of `samples`, every second direction the reference's own
    sampled one (`aimed`), the others uniform"""
    import kat_lib
    rng = np.random.default_rng(_seed(case.name) ^ 0xD1235)
    rec = np.zeros((KAT_RECORDS, 6), F)
    rec[:, 0:3] = samples[:, 0:3]
    rec[:, 3:6] = kat_lib._unit(rng, KAT_RECORDS)
    rec[::2, 3:6] = aimed[::2]
    return rec
