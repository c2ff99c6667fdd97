"""First-hit AOVs of the implicit shaders on the MI355X (include/vpt.h: vpt_render_sdf_aov_device, vpt_session_pick_sdf).
Every criterion is equality of bits, with no tolerance and no excluded pixel: `normal` against K2's `implicit_normal` image, ids / hit /
depth against vpt_spheretrace on the pixel-centre rays, albedo against the materials' colours, any batching and any subset of planes
against the full pass, two ranks against one, the own form of the march (VPT_NO_GROUP_FORMS=1, a child process) against the group form,
the session's id frame and picks against the calls they stand for.

Scenes: 06_gridsdf_synth at 96 (96 x 40: hits and misses from the default camera) and at 100 (100 x 42: ragged tiles, partly filled
waves), 07_sdfunction_synth at 128 (every pixel hits; grid instances and analytic SDFs, among them a material of opacity 0.7).  Cameras:
the default one, `perspective-dof` (lens draws) and `orthographic-sharp` (the orthographic branch of eval_camera)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENE_03 = os.path.join(GOLDEN, "scenes", "03_volume", "volume.json")

pytestmark = pytest.mark.gpu

F = np.float32
GRID = os.path.join(GOLDEN, "scenes", "06_gridsdf_synth", "gridsdf_synth.json")
FUNCS = os.path.join(GOLDEN, "scenes", "07_sdfunction_synth", "sdfunction_synth.json")
CASES = {"grid96": (GRID, 96), "grid100": (GRID, 100), "funcs128": (FUNCS, 128)}   # name -> (file, resolution)
CAMERAS = ("default", "perspective-dof", "orthographic-sharp")
SHARP = ("default", "orthographic-sharp")   # no aperture: the camera ray through a pixel centre does not depend on the lens draws
FLOAT_PLANES = ("normal", "albedo", "depth")
ALL_PLANES = FLOAT_PLANES + ("ids", "hit")
FILL, FILL_ID = 3.5, -7   # what the buffers hold where nothing may be written
KAT_CAMERA, KAT_SDF_NORMAL = 3, 11


def camera_index(file, name):
    with open(file) as f:
        return [c["name"] for c in json.load(f)["cameras"]].index(name)


def params_of(vpt, case, camera, samples, shader="implicit_normal"):
    file, resolution = CASES[case]
    return vpt.PathtraceParams(camera=camera_index(file, camera), resolution=resolution, samples=samples, shader=shader, bounces=4)


def layout_of(vpt, host, params, rank=0, nranks=1):
    st = host.make_state(params)
    return vpt.VptLayout(st.width, st.height, 8, 8, rank, nranks)


def ibits(t):
    import torch
    return t.contiguous().view(torch.int32)


def same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(ibits(a), ibits(b))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class State:
    """hits / rng (and an image) of one rank's slots, initialised on the device; padding slots hold the fill pattern"""

    def __init__(self, vpt, layout):
        import torch
        self.slots = vpt.layout_slots(layout)
        self.image = torch.full((self.slots, 4), FILL, dtype=torch.float32, device="cuda")
        self.hits = torch.full((self.slots,), FILL_ID, dtype=torch.int32, device="cuda")
        self.rng = torch.full((self.slots, 2), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        vpt.state_init_device(layout, self.image.data_ptr(), self.hits.data_ptr(), self.rng.data_ptr())
        self.real = torch.from_numpy(vpt.layout_pixel_index(layout) >= 0).cuda()


def plane_buffers(state, names):
    """zero sums in the slots that hold a pixel, the fill pattern in the padding (and in all of ids / hit: the pass writes them)"""
    import torch
    out = {}
    for n in names:
        if n == "ids":
            out[n] = torch.full((state.slots, 2), FILL_ID, dtype=torch.int32, device="cuda")
        else:
            out[n] = torch.full((state.slots, 4), FILL, dtype=torch.float32, device="cuda")
            if n != "hit":
                out[n][state.real] = 0
    return out


def sdf_pass(vpt, dev, params, layout, batches, names):
    """the pass over a fresh device state in the given batches: (planes, state)"""
    import torch
    st = State(vpt, layout)
    planes = plane_buffers(st, names)
    for n in batches:
        dev.render_sdf_aov_device(params, layout, n, {k: t.data_ptr() for k, t in planes.items()}, st.hits.data_ptr(), st.rng.data_ptr())
    torch.cuda.synchronize()
    return planes, st


def padding_kept(planes, st):
    pad = ~st.real
    return all(bool((t[pad] == (FILL_ID if n == "ids" else FILL)).all()) for n, t in planes.items())


def rows_of(vpt, layout, planes):
    """the tile-major planes of a one-rank layout as row-major numpy arrays"""
    index = vpt.layout_pixel_index(layout)
    real = index >= 0
    out = {}
    for n, t in planes.items():
        a = t.cpu().numpy()
        rows = np.zeros((layout.width * layout.height,) + a.shape[1:], a.dtype)
        rows[index[real]] = a[real]
        out[n] = rows
    return out


def centre_rays(vpt, dev, camera, w, h):
    rec = np.zeros((h, w, 5), F)
    rec[..., 0] = camera
    rec[..., 1] = ((np.arange(w, dtype=F) + F(0.5)) / F(w))[None, :]
    rec[..., 2] = ((np.arange(h, dtype=F) + F(0.5)) / F(h))[:, None]
    return dev.kat(KAT_CAMERA, rec.reshape(-1, 5))   # eval_camera on the device


def spheretrace_frame(vpt, dev, params, w, h):
    """what the pass must report with samples = 1: (ids (n, 2), hit (n, 4), depth (n, 4)) from vpt_spheretrace on the pixel-centre rays"""
    rays = centre_rays(vpt, dev, params.camera, w, h)
    sid, t = dev.spheretrace(rays, -1, params.spheretrace_maxiter)
    hit = sid[:, 0] == 1
    assert ((sid[hit, 1] >= 0) != (sid[hit, 2] >= 0)).all()   # exactly one of the pair on a hit
    ids = np.where(hit[:, None], sid[:, 1:3], -1).astype(np.int32)
    want_hit, depth = np.zeros((w * h, 4), F), np.zeros((w * h, 4), F)
    o, d = rays[:, 0:3].astype(F), rays[:, 3:6].astype(F)
    position = o + d * t[:, None].astype(F)   # float32, the product first
    want_hit[hit, 0:3], want_hit[hit, 3] = position[hit], t[hit]
    depth[hit, 0], depth[hit, 3] = t[hit], 1
    return ids, want_hit, depth, hit


@pytest.fixture(scope="module")
def scenes(vpt):
    """case -> (HostScene, DeviceScene), made on first use and shared"""
    if vpt.device_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible (the HIP path has no CPU fallback)")
    made = {}

    def get(case):
        file = CASES[case][0]
        if file not in made:
            host = vpt.HostScene(file)
            made[file] = (host, vpt.DeviceScene(host, 0))
        return made[file]
    return get


@pytest.fixture(scope="module")
def full_pass(vpt, scenes):
    """(case, camera) -> (planes, state, layout, params) of five samples in one launch with every plane: computed once, shared, left unchanged"""
    made = {}

    def get(case, camera):
        if (case, camera) not in made:
            host, dev = scenes(case)
            params = params_of(vpt, case, camera, 16)
            layout = layout_of(vpt, host, params)
            made[case, camera] = sdf_pass(vpt, dev, params, layout, [5], ALL_PLANES) + (layout, params)
        return made[case, camera]
    return get


# ---- 1. the normal plane is K2's implicit_normal image ----------------------------------------------------------------------------
@pytest.mark.parametrize("samples,nsamples", [(1, 1), (16, 2), (16, 5)])
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("case", list(CASES))
def test_normal_equals_the_implicit_normal_shader(vpt, scenes, case, camera, samples, nsamples):
    import torch
    host, dev = scenes(case)
    params = params_of(vpt, case, camera, samples)
    layout = layout_of(vpt, host, params)
    planes, st = sdf_pass(vpt, dev, params, layout, [nsamples], ("normal", "ids"))
    want = State(vpt, layout)
    dev.render_device(params, layout, nsamples, want.image.data_ptr(), want.hits.data_ptr(), want.rng.data_ptr())
    torch.cuda.synchronize()
    # whole buffers: the padding slots of both still hold the pattern they were filled with
    assert same(planes["normal"], want.image), (case, camera, int((ibits(planes["normal"]) != ibits(want.image)).any(dim=1).sum()))
    assert same(st.hits, want.hits) and same(st.rng, want.rng), (case, camera)
    assert padding_kept(planes, st)
    assert bool((st.hits[st.real] == nsamples).all())
    hit = planes["ids"][st.real].max(dim=1).values >= 0
    print(f"{case} {camera}: {layout.width} x {layout.height}, first sample: {int(hit.sum())} hits, {int((~hit).sum())} misses")
    if case != "funcs128" and camera == "default":
        assert bool(hit.any()) and bool((~hit).any()), case   # both occur in the frame
    if case == "funcs128":
        if camera == "default":
            assert bool(hit.all())   # this camera shows an SDF in every pixel
        ids = planes["ids"][st.real]
        assert bool((ids[:, 0] >= 0).any()) and bool((ids[:, 1] >= 0).any())   # both kinds: a grid instance and an analytic SDF
    assert bool(((planes["ids"][st.real] >= 0).sum(dim=1) == hit.int()).all())   # exactly one of the pair on a hit, none on a miss


# ---- 2. batching ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("case", list(CASES))
def test_any_batching_gives_the_same_bits(vpt, scenes, full_pass, case, camera):
    host, dev = scenes(case)
    whole, st, layout, params = full_pass(case, camera)
    assert padding_kept(whole, st)
    for batches in ([2, 3], [1, 1, 1, 1, 1]):
        got, st2 = sdf_pass(vpt, dev, params, layout, batches, ALL_PLANES)
        for n in ALL_PLANES:
            assert same(got[n], whole[n]), (case, camera, batches, n)
        assert same(st.hits, st2.hits) and same(st.rng, st2.rng)
    first, _ = sdf_pass(vpt, dev, params, layout, [1], ("ids", "hit", "depth"))   # ids and hit are those of the first sample
    assert same(first["ids"], whole["ids"]) and same(first["hit"], whole["hit"])
    hit = first["ids"][st.real].max(dim=1).values >= 0
    assert same(first["depth"][st.real][hit][:, 0], first["hit"][st.real][hit][:, 3])   # whose t is the first depth sample
    assert bool((first["hit"][st.real][~hit] == 0).all()) and bool((first["depth"][st.real][~hit] == 0).all())


# ---- 3. ids, hit and depth are vpt_spheretrace's ----------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", SHARP)
@pytest.mark.parametrize("case", list(CASES))
def test_ids_hit_and_depth_equal_spheretrace(vpt, scenes, case, camera):
    host, dev = scenes(case)
    params = params_of(vpt, case, camera, 1)
    layout = layout_of(vpt, host, params)
    w, h = layout.width, layout.height
    planes, st = sdf_pass(vpt, dev, params, layout, [1], ("ids", "hit", "depth"))
    assert padding_kept(planes, st)
    got = rows_of(vpt, layout, planes)
    want_ids, want_hit, want_depth, hit = spheretrace_frame(vpt, dev, params, w, h)
    print(f"{case} {camera}: {w} x {h}, {int(hit.sum())} hits, {int((~hit).sum())} misses")
    assert hit.any(), case
    assert np.array_equal(got["ids"], want_ids), (case, int((got["ids"] != want_ids).any(axis=1).sum()))
    assert np.array_equal(bits(got["hit"][:, 3]), bits(want_hit[:, 3])), case   # t
    assert np.array_equal(bits(got["hit"][:, :3]), bits(want_hit[:, :3])), case   # o + d * t
    assert np.array_equal(bits(got["depth"]), bits(want_depth)), case


# ---- 4. albedo is the colour of the hit's material --------------------------------------------------------------------------------
@pytest.mark.parametrize("case,camera", [("grid96", "default"), ("funcs128", "default"), ("funcs128", "orthographic-sharp")])
def test_albedo_is_the_colour_of_the_ids_material(vpt, scenes, case, camera):
    host, dev = scenes(case)
    params = params_of(vpt, case, camera, 1)   # the pixel-centre branch of a camera without aperture: every sample traces the same ray
    layout = layout_of(vpt, host, params)
    nsamples = 3
    planes, st = sdf_pass(vpt, dev, params, layout, [nsamples], ("albedo", "ids"))
    got = rows_of(vpt, layout, planes)
    ids = got["ids"]
    grid_material = np.array([host.volume_instance(i).material for i in range(host.count_implicit("vol_instances"))], np.int64)
    sdf_material = np.array([host.sdf(j).material for j in range(host.count_implicit("sdfs"))], np.int64)
    hit = ids.max(axis=1) >= 0
    material = np.where(ids[:, 0] >= 0, grid_material[np.maximum(ids[:, 0], 0)], sdf_material[np.maximum(ids[:, 1], 0)])
    colours = np.array([list(host.material(m).color) for m in range(host.count("materials"))], F)
    opacity = np.array([host.material(m).opacity for m in range(host.count("materials"))], F)
    want = np.zeros((len(ids), 4), F)
    for _ in range(nsamples):   # the sums, sample by sample in float32
        want[hit, :3] = want[hit, :3] + colours[material[hit]]
        want[hit, 3] = want[hit, 3] + F(1)
    assert np.array_equal(bits(got["albedo"]), bits(want)), (case, camera)
    assert (want[hit, 3] == nsamples).all() and not want[~hit].any()
    if case == "funcs128" and camera == "default":
        # a first hit is reported whatever the opacity: the frame shows the material of opacity 0.7 with its own colour
        frosted = hit & (opacity[material] < 1)
        assert frosted.any() and np.unique(opacity[material[frosted]]).tolist() == [F(0.7)]


# ---- 5. subsets and ranks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["grid100", "funcs128"])
def test_a_subset_of_planes_has_the_bits_of_the_full_pass(vpt, scenes, full_pass, case):
    host, dev = scenes(case)
    full, st, layout, params = full_pass(case, "perspective-dof")
    for subset in [(n,) for n in FLOAT_PLANES + ("ids",)] + [("ids", "hit")]:
        got, st2 = sdf_pass(vpt, dev, params, layout, [5], subset)
        for n in subset:
            assert same(got[n], full[n]), (case, subset, n)
        assert same(st.hits, st2.hits) and same(st.rng, st2.rng), subset


def test_two_ranks_assemble_to_one(vpt, scenes, full_pass):
    import torch
    case = "grid100"
    host, dev = scenes(case)
    whole, st, one, params = full_pass(case, "default")
    names = ("normal", "depth", "ids", "hit")
    w, h = one.width, one.height

    def rows(layout, planes):
        """the planes of all ranks -> row-major, through the two resolves"""
        out = {}
        for n in ("normal", "depth"):
            out[n] = torch.full((h * w, 4), FILL, dtype=torch.float32, device="cuda")
            vpt.resolve_device(layout, planes[n].data_ptr(), 5, out[n].data_ptr())
        out["ids"] = torch.full((h * w, 2), FILL_ID, dtype=torch.int32, device="cuda")
        out["hit"] = torch.full((h * w, 4), FILL, dtype=torch.float32, device="cuda")
        vpt.resolve_sdf_ids_device(layout, planes["ids"].data_ptr(), planes["hit"].data_ptr(), out["ids"].data_ptr(), out["hit"].data_ptr())
        torch.cuda.synchronize()
        return out
    want = rows(one, whole)
    assert not bool((want["ids"] == FILL_ID).any()) and not bool((want["hit"] == FILL).any())   # the gather writes every pixel

    layouts = [layout_of(vpt, host, params, r, 2) for r in (0, 1)]
    slots = vpt.layout_slots(layouts[0])
    gathered = {n: torch.cat([plane_buffers(State(vpt, lay), (n,))[n] for lay in layouts]) for n in names}   # [nranks][slots]
    for r, lay in enumerate(layouts):
        st_r = State(vpt, lay)
        before = {n: t.clone() for n, t in gathered.items()}
        part = {n: t[r * slots:(r + 1) * slots] for n, t in gathered.items()}
        dev.render_sdf_aov_device(params, lay, 5, {n: t.data_ptr() for n, t in part.items()}, st_r.hits.data_ptr(), st_r.rng.data_ptr())
        torch.cuda.synchronize()
        other = slice((1 - r) * slots, (2 - r) * slots)
        for n in names:
            assert same(gathered[n][other], before[n][other]), (r, n)   # the other rank's slots are not touched
        assert padding_kept(part, st_r)
    got = rows(layouts[0], gathered)
    for n in names:
        assert same(got[n], want[n]), n


# ---- 6. the own form of the march gives the group form's bits ---------------------------------------------------------------------
SWITCH_CASES = [("grid100", "default"), ("grid100", "perspective-dof"), ("funcs128", "default")]   # the ragged size: partly filled waves


def host_passes(vpt):
    """five samples of every plane for SWITCH_CASES through the host-array entry point (numpy alone: the child needs no more), in this
    process's form of the march: name -> array"""
    record = {}
    for case, camera in SWITCH_CASES:
        host = vpt.HostScene(CASES[case][0])
        dev = vpt.DeviceScene(host, 0)
        params = params_of(vpt, case, camera, 16)
        st = host.make_state(params)
        planes = dev.render_sdf_aovs(st, params, 2)
        planes = dev.render_sdf_aovs(st, params, 3, into=planes)
        for n in ALL_PLANES:
            record[f"{case}.{camera}.{n}"] = planes[n]
        record[f"{case}.{camera}.hits"], record[f"{case}.{camera}.rng"] = st.hits, st.rngs
    return record


def test_group_forms_off_gives_the_same_bits(vpt, tmp_path, monkeypatch):
    """VPT_NO_GROUP_FORMS is read when a scene is created: in a child process, as the existing tests of such switches do"""
    monkeypatch.delenv("VPT_NO_GROUP_FORMS", raising=False)   # the scenes this process makes below run the group round
    out = str(tmp_path / "own_form.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, VPT_NO_GROUP_FORMS="1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    group = host_passes(vpt)
    with np.load(out) as own:
        assert sorted(own.files) == sorted(group)
        for name, want in group.items():
            a = own[name]
            assert a.shape == want.shape and a.dtype == want.dtype and np.array_equal(a.view(np.uint32), want.view(np.uint32)), name
            assert a.any(), name   # a frame with content


# ---- 7. the session ---------------------------------------------------------------------------------------------------------------
def check_pick(vpt, host, dev, s, ids, hit, x, y):
    p = s.pick_sdf(x, y)
    if ids[y, x].max() < 0:
        assert p is None
        return None
    assert (p["vol_instance"], p["sdf"]) == tuple(ids[y, x])
    assert np.array_equal(bits(np.append(p["position"], F(p["distance"]))), bits(hit[y, x]))
    kind, index = (0, p["vol_instance"]) if p["vol_instance"] >= 0 else (1, p["sdf"])
    record = np.array([[kind, index, *hit[y, x, :3], hit[y, x, 3]]], F)
    assert np.array_equal(bits(p["normal"]), bits(dev.kat(KAT_SDF_NORMAL, record)[0]))
    if kind == 0:
        inst = host.volume_instance(index)
        assert (p["volume"], p["material"]) == (inst.volume, inst.material)
    else:
        assert (p["volume"], p["material"]) == (-1, host.sdf(index).material)
    return p


def test_session_pick_sdf_and_sdf_ids(vpt):
    import ctypes as C
    host = vpt.HostScene(GRID)   # a scene of its own: the session edits it
    dev = vpt.DeviceScene(host, 0)
    params = vpt.PathtraceParams(resolution=96, samples=8, shader="implicit", bounces=2)
    s = vpt.RenderSession(dev, params)
    w, h = s.size
    assert (w, h) == (96, 40)

    def frame(session, device):
        ids, hit = session.sdf_ids()
        want_ids, want_hit, _, _ = spheretrace_frame(vpt, device, vpt.PathtraceParams(resolution=96, samples=1), w, h)
        assert np.array_equal(ids.reshape(-1, 2), want_ids) and np.array_equal(bits(hit.reshape(-1, 4)), bits(want_hit))
        return ids, hit
    ids, hit = frame(s, dev)
    assert s.stats() == (3, 0, 24 * w * h)   # state, pass, resolve; the two planes cross the bus
    hit_pixels, miss_pixels = np.argwhere(ids.max(axis=-1) >= 0), np.argwhere(ids.max(axis=-1) < 0)
    grid_pixels, sdf_pixels = np.argwhere(ids[..., 0] >= 0), np.argwhere(ids[..., 1] >= 0)
    assert len(grid_pixels) and len(sdf_pixels) and len(miss_pixels)
    for pixels in (grid_pixels, sdf_pixels):
        y, x = (int(c) for c in pixels[len(pixels) // 2])
        assert check_pick(vpt, host, dev, s, ids, hit, x, y) is not None
        assert s.stats() == (1, 0, 48)   # one launch packs the record, 48 bytes cross the bus
    my, mx = (int(c) for c in miss_pixels[0])
    assert s.pick_sdf(mx, my) is None
    out = vpt.VptSdfPick()
    assert vpt.hip.vpt_session_pick_sdf(s.handle, mx, my, C.byref(out)) == 0
    assert bytes(out) == np.array([0, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0, 0], np.int32).tobytes()   # a miss: hit 0, the ids -1, the floats 0
    for bad in ((-1, 0), (w, 0), (0, h), (0, -1)):
        with pytest.raises(vpt.VptError, match="outside"):
            s.pick_sdf(*bad)

    # an instance moves: the edit resets, the next pick makes the frame anew, and it is the frame of a fresh session on the edited scene
    y, x = (int(c) for c in grid_pixels[len(grid_pixels) // 2])
    moved = int(ids[y, x, 0])
    inst = host.volume_instance(moved)
    f = np.array([*inst.frame.x, *inst.frame.y, *inst.frame.z, *inst.frame.o], F)
    f[9:12] += np.array([0.05, 0.1, -0.05], F)
    host.set_volume_instance(moved, frame=f)
    s.edit_volumes(host.update_volumes())
    s.pick_sdf(x, y)
    assert s.stats()[0] == 4   # the frame's three launches and the pack
    ids2, hit2 = frame(s, dev)
    assert not np.array_equal(ids2, ids)
    fresh_dev = vpt.DeviceScene(host, 0)
    fresh = vpt.RenderSession(fresh_dev, params)
    ids3, hit3 = frame(fresh, fresh_dev)
    assert np.array_equal(ids3, ids2) and np.array_equal(bits(hit3), bits(hit2))
    for yy, xx in (hit_pixels[0], hit_pixels[-1], (y, x)):
        check_pick(vpt, host, dev, s, ids2, hit2, int(xx), int(yy))
    assert s.stats() == (1, 0, 48)
    fresh.close()
    # the mesh entry points keep refusing this session, and a mesh session refuses these
    assert vpt.hip.vpt_session_pick(s.handle, 1, 1, C.byref(vpt.VptPick())) == -5
    s.close()
    mesh_host = vpt.HostScene(SCENE_03)
    m = vpt.RenderSession(vpt.DeviceScene(mesh_host, 0), vpt.PathtraceParams(resolution=64, samples=4, shader="volpathtrace", bounces=2))
    assert vpt.hip.vpt_session_pick_sdf(m.handle, 1, 1, C.byref(out)) == -5 and b"vpt_session_pick" in vpt.hip.vpt_last_error()   # VPT_ERR_UNSUPPORTED
    buf = np.zeros((m.size[1], m.size[0], 2), np.int32)
    assert vpt.hip.vpt_session_get_sdf_ids(m.handle, buf.ctypes.data, None) == -5
    with pytest.raises(vpt.VptError):
        m.pick_sdf(1, 1)
    m.close()


def test_an_implicit_normal_session_serves_picks_too(vpt, scenes):
    host, dev = scenes("funcs128")
    s = vpt.RenderSession(dev, vpt.PathtraceParams(resolution=128, samples=4, shader="implicit_normal"))
    w, h = s.size
    ids, hit = s.sdf_ids()
    want_ids, want_hit, _, _ = spheretrace_frame(vpt, dev, vpt.PathtraceParams(resolution=128, samples=1), w, h)
    assert np.array_equal(ids.reshape(-1, 2), want_ids) and np.array_equal(bits(hit.reshape(-1, 4)), bits(want_hit))
    for j in np.unique(ids[..., 1][ids[..., 1] >= 0]):   # one pick per analytic SDF in view: every type's normal function
        y, x = (int(c) for c in np.argwhere(ids[..., 1] == j)[0])
        assert check_pick(vpt, host, dev, s, ids, hit, x, y)["sdf"] == j
    s.close()


# ---- 8. the host-array entry point ------------------------------------------------------------------------------------------------
def test_host_arrays_entry_point(vpt, scenes):
    """vpt_render_sdf_aov (DeviceScene.render_sdf_aovs): row-major planes in and out, batched, ends at the cap"""
    case, camera = "grid100", "perspective-dof"
    host, dev = scenes(case)
    params = params_of(vpt, case, camera, 6)
    st = host.make_state(params)
    got = dev.render_sdf_aovs(st, params, 2)
    got = dev.render_sdf_aovs(st, params, 100, into=got)   # ends at the cap
    assert st.samples == 6 and (st.hits == 6).all()
    want = host.make_state(params)
    dev.pathtrace_samples(want, params, 6)   # implicit_normal through K2
    assert np.array_equal(bits(got["normal"]), bits(want.image))
    assert np.array_equal(st.rngs, want.rngs)
    layout = layout_of(vpt, host, params)
    planes, _ = sdf_pass(vpt, dev, params, layout, [6], ALL_PLANES)   # and every plane is the device pass's, pixel for pixel
    rows = rows_of(vpt, layout, planes)
    for n in ALL_PLANES:
        assert got[n].shape[:2] == (st.height, st.width)
        assert np.array_equal(bits(got[n].reshape(rows[n].shape)), bits(rows[n])), n
    only = dev.render_sdf_aovs(host.make_state(params), params, 6, planes=("depth",))
    assert list(only) == ["depth"] and np.array_equal(bits(only["depth"]), bits(got["depth"]))


def test_device_entry_point_refusals_and_the_no_op(vpt, scenes):
    host, dev = scenes("grid96")
    params = params_of(vpt, "grid96", "default", 4)
    layout = layout_of(vpt, host, params)
    st = State(vpt, layout)
    planes = plane_buffers(st, ALL_PLANES)
    ptrs = {k: t.data_ptr() for k, t in planes.items()}
    with pytest.raises(vpt.VptError, match="every plane is null"):
        dev.render_sdf_aov_device(params, layout, 1, {}, st.hits.data_ptr(), st.rng.data_ptr())
    with pytest.raises(vpt.VptError, match="hit is given without ids"):
        dev.render_sdf_aov_device(params, layout, 1, {"hit": ptrs["hit"]}, st.hits.data_ptr(), st.rng.data_ptr())
    with pytest.raises(vpt.VptError, match="spheretrace_maxiter"):
        dev.render_sdf_aov_device(vpt.PathtraceParams(resolution=96, spheretrace_maxiter=(1 << 20) + 1), layout, 1, ptrs, st.hits.data_ptr(), st.rng.data_ptr())
    with pytest.raises(vpt.VptError, match="camera"):
        dev.render_sdf_aov_device(vpt.PathtraceParams(resolution=96, camera=99), layout, 1, ptrs, st.hits.data_ptr(), st.rng.data_ptr())
    import torch
    before = {k: t.clone() for k, t in planes.items()}
    hits, rng = st.hits.clone(), st.rng.clone()
    dev.render_sdf_aov_device(params, layout, 0, ptrs, st.hits.data_ptr(), st.rng.data_ptr())   # nsamples == 0: nothing happens
    torch.cuda.synchronize()
    assert all(same(planes[k], before[k]) for k in planes) and same(st.hits, hits) and same(st.rng, rng)
    # maxiter 0: no step is taken, every sample is a miss; the state advances all the same
    zero = vpt.PathtraceParams(resolution=96, samples=4, shader="implicit_normal", spheretrace_maxiter=0)
    dev.render_sdf_aov_device(zero, layout, 2, ptrs, st.hits.data_ptr(), st.rng.data_ptr())
    torch.cuda.synchronize()
    assert bool((planes["ids"][st.real] == -1).all()) and bool((planes["normal"][st.real] == 0).all()) and bool((st.hits[st.real] == 2).all())
    assert padding_kept(planes, st)


if __name__ == "__main__":   # the child of test_group_forms_off_gives_the_same_bits
    sys.path.insert(0, ROOT)
    import vpt_loader
    np.savez(sys.argv[1], **host_passes(vpt_loader.load()))
    print("dumped with VPT_NO_GROUP_FORMS=" + os.environ.get("VPT_NO_GROUP_FORMS", ""), flush=True)
