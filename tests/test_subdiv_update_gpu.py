"""vpt_scene_attach_subdiv / vpt_scene_update_subdivs on the GPU (include/vpt.h).  The criterion is equality of bits, no
tolerance anywhere: A = a DeviceScene whose subdivs are re-tesselated on the device, against B = a second handle of the same scene edited
the parent's way - the host mirror's tesselate_surface (HostScene.set_subdiv), its vertices through vpt_scene_update, and through
vpt_scene_update_lights where a light's instance uses the shape (tests/subdiv_edits.py: parents_way).  Compared: the eight groups of
vpt_scene_shape_tables_hash, vpt_scene_get_bvh, vpt_scene_light_tables_hash, vpt_intersect on 300 NaN-prone rays and the state of a
volpathtrace render at 64 pixels, 2 samples.  The vertex pools are compared, too, with a fresh handle loaded from files that carry
the edit.  Scenes: 08_subdiv_synth (its four subdivs: every level of the tetra and the strip fits one workgroup) and 01_surface_min
(the cube's four levels refine to 26, 98, 386 and 1538 vertices: the fused launch, the launch per level and the 256-thread block
boundary).  Every test calls an entry point that exists only with the feature."""
import ctypes as C

import numpy as np
import pytest

import subdiv_edits as S
from test_scene_update_gpu import rays_for, same_state

pytestmark = pytest.mark.gpu
F = np.float32
RES, SPP = 64, 2
INVALID, UNSUPPORTED = r"\(-1\)", r"\(-5\)"


def render(vpt, dev, host, shader="volpathtrace"):
    p = vpt.PathtraceParams(resolution=RES, samples=SPP, shader=shader, bounces=4)
    st = host.make_state(p)
    dev.pathtrace_samples(st, p, SPP)
    return st


def tables(dev):
    return dev.shape_tables_hash(), [x.tobytes() for x in dev.get_bvh()], dev.light_tables_hash()


def assert_same(vpt, A, B, host, what):
    for k, (a, b) in enumerate(zip(A.shape_tables_hash(), B.shape_tables_hash())):
        assert a == b, f"{what}: group {k} of the shape tables differs from the parent's way"
    assert [x.tobytes() for x in A.get_bvh()] == [x.tobytes() for x in B.get_bvh()], f"{what}: the node arrays differ"
    assert A.light_tables_hash() == B.light_tables_hash(), f"{what}: the light tables differ"
    rays = rays_for(host, 300)
    (ia, ua), (ib, ub) = A.intersect(rays), B.intersect(rays)
    assert np.array_equal(ia, ib) and np.array_equal(ua.view(np.uint32), ub.view(np.uint32)), f"{what}: vpt_intersect differs"
    assert same_state(render(vpt, A, host), render(vpt, B, host)), f"{what}: the renders differ"


def pair(vpt, file):
    """(A, B, B's host mirror): two handles of one scene file"""
    host = vpt.HostScene(file)
    return vpt.DeviceScene(vpt.HostScene(file), 0), vpt.DeviceScene(host, 0), host


def both_ways(vpt, A, B, host, cages=None, amounts=None):
    """the edit on the mirror, then on A through update_subdivs and on B the parent's way; returns the SubdivEdit"""
    cages, amounts = cages or {}, amounts or {}
    for i in sorted(set(cages) | set(amounts)):
        host.set_subdiv(i, positions=cages.get(i), displacement=amounts.get(i))
    edit = host.update_subdivs()
    A.update_subdivs(edit)
    S.parents_way(vpt, B, host, sorted(edit.shape_of.values()))
    return edit


def keep_all(vpt, host, ids):
    return vpt.SubdivEdit({i: (None, None) for i in ids}, shape_of={i: host.subdiv(i)["shape"] for i in ids}, plan_of=host.subdiv_plan)


def pools(dev):
    return dev.shape_tables_hash()[1]   # positions, normals, texcoords and colors in one chain


@pytest.mark.parametrize("scene_file", [S.SYNTH, S.SURF])
def test_attach_is_idle_and_keep_all_reproduces(vpt, scene_file):
    host = vpt.HostScene(S.path(scene_file))
    A = vpt.DeviceScene(host, 0)
    before, picture = tables(A), render(vpt, A, host)
    for i in range(4):
        A.attach_subdiv(i, host.subdiv_plan(i))
        launches, nbytes, _ = A.update_stats()
        assert launches == 0 and nbytes > 12 * len(host.subdiv(i)["positions"])
    assert A.subdiv_count() == 4 and tables(A) == before and same_state(render(vpt, A, host), picture)
    A.update_subdivs(keep_all(vpt, host, range(4)))   # tesselated again from what the device holds: the same bytes
    assert A.update_stats()[0] > 0 and A.update_stats()[1] == 0 and A.subdiv_count() == 4
    assert tables(A) == before and same_state(render(vpt, A, host), picture)
    A.detach_subdiv(2)
    assert A.subdiv_count() == 3
    with pytest.raises(vpt.VptError, match="not attached"):
        vpt._check(vpt.hip.vpt_scene_detach_subdiv(A.handle, 2), "vpt_scene_detach_subdiv")
    A.update_subdivs(keep_all(vpt, host, [2]))   # attached again on first use
    assert A.subdiv_count() == 4 and tables(A) == before


@pytest.mark.parametrize("scene_file", [S.SYNTH, S.SURF])
def test_moved_cage(vpt, tmp_path, scene_file):
    A, B, host = pair(vpt, S.path(scene_file))
    before = tables(A)
    cages = {i: S.moved(host.subdiv(i)["positions"], 20 + i) for i in range(4)}
    both_ways(vpt, A, B, host, cages)
    assert tables(A) != before
    assert_same(vpt, A, B, host, scene_file)
    fresh = vpt.DeviceScene(vpt.HostScene(S.write_scene(scene_file, tmp_path, cages)), 0)
    assert pools(A) == pools(fresh), "the vertex pools differ from those of a scene loaded from the edited cages"


def test_displacement_amount(vpt, tmp_path):
    A, B, host = pair(vpt, S.path(S.SYNTH))
    both_ways(vpt, A, B, host, amounts={S.STRIP: 0.05, S.BALL: 0.0625})
    assert_same(vpt, A, B, host, "0.02 -> 0.05")
    fresh = vpt.DeviceScene(vpt.HostScene(S.write_scene(S.SYNTH, tmp_path / "a", settings={S.STRIP: {"displacement": 0.05}, S.BALL: {"displacement": 0.0625}})), 0)
    assert pools(A) == pools(fresh)
    both_ways(vpt, A, B, host, amounts={S.STRIP: 0.0})   # the smooth strip keeps its normals: quads_normals' instead of the displaced mesh's
    assert_same(vpt, A, B, host, "-> 0")
    fresh = vpt.DeviceScene(vpt.HostScene(S.write_scene(S.SYNTH, tmp_path / "b", settings={S.STRIP: {"displacement": 0.0}, S.BALL: {"displacement": 0.0625}})), 0)
    assert pools(A) == pools(fresh)
    both_ways(vpt, A, B, host, amounts={S.STRIP: 0.02})   # and on again
    assert_same(vpt, A, B, host, "0 -> 0.02")


def flat_ball_without_normals(d):
    """the ball's cage replaced by one without normals of its own (the strip's), still 0 levels, flat, displaced by the float texture"""
    d["subdivs"][S.BALL]["uri"] = d["shapes"][4]["uri"] = "subdivs/strip.obj"


def test_refusal_pool_change(vpt, tmp_path):
    for file in (S.path(S.SYNTH), S.write_scene(S.SYNTH, tmp_path, change=flat_ball_without_normals)):
        A, B, host = pair(vpt, file)
        ball = host.subdiv(S.BALL)
        assert ball["subdivisions"] == 0 and not ball["smooth"] and ball["displacement"] != 0
        A.attach_subdiv(S.BALL, host.subdiv_plan(S.BALL))
        before = tables(A)
        off = vpt.SubdivEdit({S.BALL: (None, 0.0)}, shape_of={S.BALL: ball["shape"]})
        if len(ball["quadsnorm"]) > 0:   # displaced: no normals; not displaced: the cage's own - the edit would add a pool
            with pytest.raises(vpt.VptError, match=UNSUPPORTED):
                A.update_subdivs(off)
            assert tables(A) == before and A.subdiv_count() == 1
            A.update_subdivs(keep_all(vpt, host, [S.BALL]))
            assert tables(A) == before
        else:   # no normals either way: switched off and on again like any amount
            both_ways(vpt, A, B, host, amounts={S.BALL: 0.0})
            assert tables(A) != before
            assert_same(vpt, A, B, host, "off")
            both_ways(vpt, A, B, host, amounts={S.BALL: 0.004})
            assert_same(vpt, A, B, host, "on")
    seen = [len(vpt.HostScene(f).subdiv(S.BALL)["quadsnorm"]) > 0 for f in (S.path(S.SYNTH), file)]
    assert sorted(seen) == [False, True], "both branches are to be seen"


def test_emissive_subdiv(vpt, tmp_path):
    def lit(d):
        d["instances"][1]["material"] = 5   # the bowtie's instance on the `light` material
    A, B, host = pair(vpt, S.write_scene(S.SYNTH, tmp_path, change=lit))
    assert host.subdiv(S.BOWTIE)["shape"] in S.lit_shapes(host)
    before = A.light_tables_hash()
    both_ways(vpt, A, B, host, {S.BOWTIE: S.moved(host.subdiv(S.BOWTIE)["positions"], 31, 0.02)})
    assert A.light_tables_hash() != before
    assert_same(vpt, A, B, host, "emissive bowtie")
    assert A.get_lights()[1].tobytes() == host.lights()[1].tobytes(), "the element CDF differs from the mirror's make_lights"


def test_texture_then_subdiv(vpt):
    A, B, host = pair(vpt, S.path(S.SYNTH))
    tex = host.subdiv(S.STRIP)["displacement_tex"]
    texels, _ = host.texture(tex)
    rng = np.random.default_rng(41)
    for shape in (texels.shape, (2 * texels.shape[0], 2 * texels.shape[1] + 3, 4)):   # repainted in place; then larger: the pool grows and moves
        host.set_texture(tex, rng.integers(0, 256, shape, dtype=np.uint8))
        edit = host.update_textures()
        A.update_textures(edit), B.update_textures(edit)
        before = pools(A)
        host.set_subdiv(S.STRIP)   # the mirror tesselates again from the new texels
        A.update_subdivs(host.update_subdivs())
        S.parents_way(vpt, B, host, [host.subdiv(S.STRIP)["shape"]])
        assert pools(A) != before
        assert_same(vpt, A, B, host, f"texture {shape}")
        assert pools(A) == pools(vpt.DeviceScene(host, 0)), "the vertex pools differ from a fresh handle with that texture"


def test_with_shape_edits(vpt):
    A, B, host = pair(vpt, S.path(S.SYNTH))
    A.update_subdivs(keep_all(vpt, host, [S.BOWTIE, S.STRIP]))
    host.remove_instances([0])   # the floor's: shape 0 can go, every later shape moves down by one
    edit = host.update_instances()
    A.update_instances(edit), B.update_instances(edit)
    host.remove_shapes([0])
    edit = host.update_shapes()
    A.update_shapes(edit), B.update_shapes(edit)
    assert host.subdiv(S.BOWTIE)["shape"] == 0 and A.subdiv_count() == 2
    both_ways(vpt, A, B, host, {S.BOWTIE: S.moved(host.subdiv(S.BOWTIE)["positions"], 51), S.STRIP: S.moved(host.subdiv(S.STRIP)["positions"], 52)}, {S.STRIP: 0.03})
    assert A.subdiv_count() == 2, "the plans followed the renumbering: nothing was attached again"
    assert_same(vpt, A, B, host, "after a removal")
    strip = host.subdiv(S.STRIP)["shape"]
    host.set_shape(strip, **{k: v for k, v in host.shape_arrays(strip).items() if len(v)})
    A.update_shapes(host.update_shapes())
    assert A.subdiv_count() == 1
    abi, keep = vpt.SubdivEdit({S.STRIP: (None, None)}).to_abi(A._subdiv_ids)
    before = tables(A)
    assert vpt.hip.vpt_scene_update_subdivs(A.handle, C.byref(abi)) == -1 and b"not attached" in vpt.hip.vpt_last_error()
    assert tables(A) == before
    del keep


def test_after_rebuild(vpt):
    A, B, host = pair(vpt, S.path(S.SURF))
    A.update_subdivs(keep_all(vpt, host, [S.CUBE]))
    rebuild = host.rebuild_bvh([host.subdiv(S.CUBE)["shape"]])
    A.rebuild_bvh(rebuild), B.rebuild_bvh(rebuild)
    both_ways(vpt, A, B, host, {S.CUBE: S.moved(host.subdiv(S.CUBE)["positions"], 61, 0.05)})
    assert A.subdiv_count() == 1
    assert_same(vpt, A, B, host, "after a rebuild")


@pytest.mark.parametrize("scene_file", [S.SYNTH, S.SURF])
def test_no_fuse_same_bits(vpt, monkeypatch, scene_file):
    host = vpt.HostScene(S.path(scene_file))
    cages = {i: S.moved(host.subdiv(i)["positions"], 70 + i) for i in range(4)}
    for i in range(4):
        host.set_subdiv(i, positions=cages[i])
    edit = host.update_subdivs()
    seen = []
    for no_fuse in (False, True):
        if no_fuse:
            monkeypatch.setenv("VPT_UPDATE_NO_FUSE", "1")
        A = vpt.DeviceScene(vpt.HostScene(S.path(scene_file)), 0)
        A.update_subdivs(edit)
        seen.append((tables(A), A.update_stats()[0]))
    assert seen[0][0] == seen[1][0], "the bits depend on the fusion switch"
    assert seen[0][1] < seen[1][1], "the switch changed no launch"


def pad16(n):
    return (n + 15) // 16 * 16


def test_pcie_bytes(vpt):
    A, B, host = pair(vpt, S.path(S.SURF))
    A.update_subdivs(keep_all(vpt, host, [S.CUBE]))
    cage = S.moved(host.subdiv(S.CUBE)["positions"], 81)
    both_ways(vpt, A, B, host, {S.CUBE: cage})
    shape = host.subdiv(S.CUBE)["shape"]
    nv, normals = len(host.shape_positions(shape)), len(host.shape_normals(shape)) > 0
    # what the refit itself sends besides the vertices it is given: the parent's bytes less its staged positions and normals
    refit_alone = B.update_stats()[1] - (pad16(12 * nv) + (12 * nv if normals else 0))
    launches, nbytes, ms = A.update_stats()
    print(f"cube: {launches} launches, {nbytes} bytes against {B.update_stats()[1]} the parent's way, {ms:.3f} device ms", flush=True)
    constant_per_subdiv = 0   # include/vpt.h: settings and table addresses travel as kernel arguments
    assert refit_alone >= 0 and nbytes <= 12 * len(cage) + constant_per_subdiv + refit_alone
    assert nbytes == 12 * len(cage)


def test_session_and_multi(vpt):
    A, B, host = pair(vpt, S.path(S.SYNTH))
    p = vpt.PathtraceParams(resolution=RES, samples=8, shader="volpathtrace", bounces=4)
    session = vpt.RenderSession(A, p, pratio=4)
    session.advance(3)
    M = vpt.MultiDeviceScene(vpt.HostScene(S.path(S.SYNTH)), [0])
    for i, cage in {S.BOWTIE: S.moved(host.subdiv(S.BOWTIE)["positions"], 91), S.STRIP: S.moved(host.subdiv(S.STRIP)["positions"], 92)}.items():
        host.set_subdiv(i, positions=cage, displacement=0.04 if i == S.STRIP else None)
    edit = host.update_subdivs()
    session.edit_subdivs(edit)
    assert session.samples == 0 and A.subdiv_count() == 2
    S.parents_way(vpt, B, host, sorted(edit.shape_of.values()))
    session.advance(SPP)
    want = host.make_state(p)
    B.pathtrace_samples(want, p, SPP)
    assert same_state(session.state(), want)
    with pytest.raises(vpt.VptError, match=INVALID):   # a refused edit leaves the session as it was
        session.edit_subdivs(vpt.SubdivEdit({S.STRIP: (np.full((9, 3), np.nan, F), None)}, shape_of=edit.shape_of))
    assert session.samples == SPP and same_state(session.state(), want)
    session.close()
    M.update_subdivs(edit)
    got = host.make_state(p)
    M.pathtrace_samples(got, p, SPP)
    assert same_state(got, want)


def test_levels_via_shape_edit(vpt, tmp_path):
    A, _, host = pair(vpt, S.path(S.SYNTH))
    A.update_subdivs(keep_all(vpt, host, [S.TETRA]))
    host.set_subdiv(S.TETRA, subdivisions=1)
    edit = host.update_shapes()
    assert list(edit.set) == [host.subdiv(S.TETRA)["shape"]]
    A.update_shapes(edit)
    assert A.subdiv_count() == 0   # the plan went with the shape it was made for
    fresh_host = vpt.HostScene(S.write_scene(S.SYNTH, tmp_path, settings={S.TETRA: {"subdivisions": 1}}))
    assert_same(vpt, A, vpt.DeviceScene(fresh_host, 0), fresh_host, "one level")
    A.update_subdivs(keep_all(vpt, host, [S.TETRA]))   # made again on next use, for the new level
    assert A.subdiv_count() == 1 and pools(A) == pools(vpt.DeviceScene(fresh_host, 0))


def test_bad_arguments(vpt):
    host = vpt.HostScene(S.path(S.SYNTH))
    A = vpt.DeviceScene(host, 0)
    A.attach_subdiv(S.BOWTIE, host.subdiv_plan(S.BOWTIE))
    before = tables(A)
    shape_of = {i: host.subdiv(i)["shape"] for i in range(4)}
    cage = host.subdiv(S.BOWTIE)["positions"]
    bad_cage = cage.copy()
    bad_cage[5, 2] = np.nan

    def raw(ids, cages=None, amounts=None, null_ids=False):
        ids = np.array(ids, np.int32)
        ptrs = (C.c_void_p * max(1, len(ids)))(*[None if c is None else c.ctypes.data for c in (cages or [None] * len(ids))])
        amounts = np.array(amounts if amounts is not None else [np.nan] * len(ids), F)
        abi = vpt.VptSubdivEdit(len(ids), None if null_ids else ids.ctypes.data, C.addressof(ptrs), amounts.ctypes.data)
        rc = vpt.hip.vpt_scene_update_subdivs(A.handle, C.byref(abi))
        return rc, vpt.hip.vpt_last_error().decode()

    dev_id = A._subdiv_ids[S.BOWTIE]
    for rc, message, word in (raw([99]) + ("out of range",), raw([-1]) + ("out of range",), raw([dev_id, dev_id]) + ("repeated",),
                              raw([dev_id], [bad_cage]) + ("not finite",), raw([dev_id], amounts=[np.inf]) + ("not finite",),
                              raw([dev_id], null_ids=True) + ("null",), raw([dev_id + 1]) + ("out of range",)):
        assert rc == -1 and word in message and "subdiv" in message, (rc, message, word)
    assert tables(A) == before
    # plans that disagree with the shape, or with themselves: refused on the host, nothing attached
    def plan_with(index, **changes):
        plan = host.subdiv_plan(index)
        for key, value in changes.items():
            setattr(plan, key, value)
        return plan
    tetra, strip = host.subdiv_plan(S.TETRA), host.subdiv_plan(S.STRIP)
    far = strip.verts.copy()
    far[7, 0] = 10 ** 6
    items = [L.copy() for L in [strip.levels[1]["items"]]][0]
    items[3] = -2
    for plan in (plan_with(S.TETRA, shape=shape_of[S.STRIP]), plan_with(S.TETRA, shape=99), plan_with(S.TETRA, verts=tetra.verts[:-1]),
                 plan_with(S.TETRA, quads=tetra.quads[:-1]), plan_with(S.TETRA, smooth=True), plan_with(S.STRIP, verts=far),
                 plan_with(S.STRIP, levels=[strip.levels[0], dict(strip.levels[1], items=items)]), plan_with(S.STRIP, levels=strip.levels[:1]),
                 plan_with(S.STRIP, displacement_tex=17), plan_with(S.STRIP, cage_positions=np.full_like(strip.cage_positions, np.inf)),
                 plan_with(S.BOWTIE)):   # (the last: its shape has a plan already)
        with pytest.raises(vpt.VptError, match=INVALID):
            A.attach_subdiv(3, plan)
    assert A.subdiv_count() == 1 and tables(A) == before
    with pytest.raises(vpt.VptError, match="no plan"):
        A.update_subdivs(vpt.SubdivEdit({S.TETRA: (None, None)}, shape_of=shape_of))
