"""First-hit AOVs in one pass on the MI355X (include/vpt.h: vpt_render_aov_device, vpt_session_pick).  Every criterion is
equality of bits: the three float planes against the debug shaders whose rays the pass traces once, ids / uvt / depth against
vpt_intersect on the pixel-centre rays, any batching and any subset of planes against the full pass, two ranks against one, the
session's guides and id frame against the calls they stand for.

Scenes: 03_volume at 128 (textures, element and vertex normals) and at 100 (ragged tiles: 100 x 42), 01_surface_min at 96 (normal
maps), 09_curves_synth at 96 (the CURVES instance), a crowd of 64 (non-rigid instance frames, scene leaves of several instances) and
deep_scene (its traversal stack overflows into HBM: the SPILL instance)."""
import os

import numpy as np
import pytest

import synth_scenes as ss
from conftest import GOLDEN, SCENE_03

pytestmark = pytest.mark.gpu

F = np.float32
SURFACE = os.path.join(GOLDEN, "scenes", "01_surface_min", "surface_min.json")
CURVES = os.path.join(GOLDEN, "scenes", "09_curves_synth", "curves.json")
GRID = os.path.join(GOLDEN, "scenes", "06_gridsdf_synth", "gridsdf_synth.json")
CASES = {"volume": 128, "volume_ragged": 100, "surface": 96, "curves": 96, "crowd": 96, "deep": 96}   # name -> resolution
FLOAT_PLANES = ("normal", "albedo", "texcoord", "depth")
SHADER_OF = {"normal": "normal", "albedo": "color", "texcoord": "texcoord"}
FILL, FILL_ID = 3.5, -7   # what the buffers hold where nothing may be written


@pytest.fixture(scope="module")
def scene_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("aov")
    return {"volume": SCENE_03, "volume_ragged": SCENE_03, "surface": SURFACE, "curves": CURVES, "crowd": ss.crowd_scene(d / "crowd", 64)[0],
            "deep": ss.deep_scene(d / "deep")[0]}


@pytest.fixture(scope="module")
def scenes(vpt, scene_files):
    """name -> (HostScene, DeviceScene), made on first use and shared"""
    if vpt.device_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible (the HIP path has no CPU fallback)")
    made = {}

    def get(name):
        if name not in made:
            host = vpt.HostScene(scene_files[name])
            made[name] = (host, vpt.DeviceScene(host, 0))
        return made[name]
    return get


def params_of(vpt, name, samples, shader="normal"):
    return vpt.PathtraceParams(resolution=CASES[name], samples=samples, shader=shader, bounces=4)


def layout_of(vpt, host, params, rank=0, nranks=1):
    st = host.make_state(params)
    return vpt.VptLayout(st.width, st.height, 8, 8, rank, nranks)


def ibits(t):
    import torch
    return t.contiguous().view(torch.int32)


def same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(ibits(a), ibits(b))


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
    """zero sums in the slots that hold a pixel, the fill pattern in the padding"""
    import torch
    out = {}
    for n in names:
        if n == "ids":
            out[n] = torch.full((state.slots, 2), FILL_ID, dtype=torch.int32, device="cuda")
        elif n == "uvt":
            out[n] = torch.full((state.slots, 3), FILL, dtype=torch.float32, device="cuda")
        else:
            out[n] = torch.full((state.slots, 4), FILL, dtype=torch.float32, device="cuda")
            out[n][state.real] = 0
    return out


def aov_pass(vpt, dev, params, layout, batches, names):
    """the pass over a fresh device state in the given batches: (planes, state)"""
    import torch
    st = State(vpt, layout)
    planes = plane_buffers(st, names)
    for n in batches:
        dev.render_aov_device(params, layout, n, {k: t.data_ptr() for k, t in planes.items()}, st.hits.data_ptr(), st.rng.data_ptr())
    torch.cuda.synchronize()
    return planes, st


def debug_render(vpt, dev, params, layout, nsamples):
    import torch
    st = State(vpt, layout)
    dev.render_device(params, layout, nsamples, st.image.data_ptr(), st.hits.data_ptr(), st.rng.data_ptr())
    torch.cuda.synchronize()
    return st


def padding_kept(planes, st):
    pad = ~st.real
    return all(bool((t[pad] == (FILL_ID if n == "ids" else FILL)).all()) for n, t in planes.items())


# ---- 1. the planes are the debug shaders' images ----------------------------------------------------------------------------------
@pytest.mark.parametrize("samples,nsamples", [(1, 1), (16, 5)])
@pytest.mark.parametrize("name", list(CASES))
def test_planes_equal_the_debug_shaders(vpt, scenes, name, samples, nsamples):
    host, dev = scenes(name)
    layout = layout_of(vpt, host, params_of(vpt, name, samples))
    planes, st = aov_pass(vpt, dev, params_of(vpt, name, samples), layout, [nsamples], ("normal", "albedo", "texcoord"))
    for plane, shader in SHADER_OF.items():
        want = debug_render(vpt, dev, params_of(vpt, name, samples, shader), layout, nsamples)
        # whole buffers: the padding slots of both still hold the pattern they were filled with
        assert same(planes[plane], want.image), (name, plane, int((ibits(planes[plane]) != ibits(want.image)).any(dim=1).sum()))
        assert same(st.hits, want.hits) and same(st.rng, want.rng), (name, plane)
    assert padding_kept(planes, st)
    assert bool((st.hits[st.real] == nsamples).all())
    covered = float((planes["normal"][st.real][:, 3] > 0).float().mean())
    assert covered > 0.02, (name, covered)   # the frame shows the scene


# ---- 2. batching ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_any_batching_gives_the_same_bits(vpt, scenes, name):
    host, dev = scenes(name)
    params = params_of(vpt, name, 16)
    layout = layout_of(vpt, host, params)
    names = FLOAT_PLANES + ("ids", "uvt")
    whole, st = aov_pass(vpt, dev, params, layout, [5], names)
    for batches in ([2, 3], [1, 1, 3]):
        got, st2 = aov_pass(vpt, dev, params, layout, batches, names)
        for n in names:
            assert same(got[n], whole[n]), (name, batches, n)
        assert same(st.hits, st2.hits) and same(st.rng, st2.rng)
    first, _ = aov_pass(vpt, dev, params, layout, [1], ("ids", "uvt", "depth"))   # ids and uvt are those of the first sample
    assert same(first["ids"], whole["ids"]) and same(first["uvt"], whole["uvt"])
    hit = first["ids"][st.real][:, 0] >= 0
    assert same(first["depth"][st.real][hit][:, 0], first["uvt"][st.real][hit][:, 2])   # whose distance is the first depth sample


# ---- 3. ids, uvt and depth are vpt_intersect's ------------------------------------------------------------------------------------
def pinhole(vpt, scene_files, name, step_back=False):
    """a scene of its own whose camera has no aperture (set through vpt_scene_update where the file gives it one).  step_back: the
    camera also moves back along its own axis until the scene's bounding sphere spans two thirds of the smaller side of the frame.
    The cameras of the golden scenes and of deep_scene show geometry in every pixel (measured: 6784, 4200, 3840, 3840 and 9216 hits, no
    miss; only the crowd's shows background), so the frames in which hits AND misses must occur are taken from there: the sphere holds
    every primitive, so the frame's corners miss, and the view axis passes through its centre."""
    host = vpt.HostScene(scene_files[name])
    dev = vpt.DeviceScene(host, 0)
    cam = host.camera(0)
    if cam.aperture > 0 or step_back:
        cam.aperture = 0
        if step_back:
            root = dev.get_bvh()[0][0]
            lo, hi = root["bbox_min"].astype(np.float64), root["bbox_max"].astype(np.float64)
            side = cam.film / cam.aspect if cam.aspect >= 1 else cam.film * cam.aspect
            distance = np.linalg.norm(hi - lo) / 2 / (0.66 * (side / 2) / cam.lens)
            for k in range(3):
                cam.frame.o[k] = float((lo[k] + hi[k]) / 2 + cam.frame.z[k] * distance)
        host.set_camera(0, cam)
        dev.update(host.update_bvh())
    return host, dev


def centre_rays(vpt, dev, w, h):
    rec = np.zeros((h, w, 5), F)
    rec[..., 1] = ((np.arange(w, dtype=F) + F(0.5)) / F(w))[None, :]
    rec[..., 2] = ((np.arange(h, dtype=F) + F(0.5)) / F(h))[:, None]
    return dev.kat(3, rec.reshape(-1, 5))   # VPT_KAT_CAMERA: eval_camera on the device


@pytest.mark.parametrize("step_back", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_ids_uvt_and_depth_equal_intersect(vpt, scene_files, name, step_back):
    host, dev = pinhole(vpt, scene_files, name, step_back)
    params = params_of(vpt, name, 1)
    layout = layout_of(vpt, host, params)
    w, h = layout.width, layout.height
    planes, st = aov_pass(vpt, dev, params, layout, [1], ("ids", "uvt", "depth"))
    assert padding_kept(planes, st)
    index = vpt.layout_pixel_index(layout)
    real = index >= 0
    ids, uvt, depth = np.zeros((w * h, 2), np.int32), np.zeros((w * h, 3), F), np.zeros((w * h, 4), F)
    ids[index[real]], uvt[index[real]], depth[index[real]] = planes["ids"].cpu().numpy()[real], planes["uvt"].cpu().numpy()[real], planes["depth"].cpu().numpy()[real]
    want_ids, want_uvt = dev.intersect(centre_rays(vpt, dev, w, h))
    hit = want_ids[:, 0] >= 0
    print(f"{name}{' from further back' if step_back else ''}: {w} x {h}, {int(hit.sum())} hits, {int((~hit).sum())} misses")
    assert hit.any(), name
    if step_back or name == "crowd":
        assert (~hit).any(), name   # both occur in the frame
    assert np.array_equal(ids, want_ids), (name, int((ids != want_ids).any(axis=1).sum()))
    assert np.array_equal(uvt.view(np.uint32), want_uvt.view(np.uint32)), (name, int((uvt.view(np.uint32) != want_uvt.view(np.uint32)).any(axis=1).sum()))
    want_depth = np.zeros((w * h, 4), F)
    want_depth[hit, 0], want_depth[hit, 3] = want_uvt[hit, 2], 1
    assert np.array_equal(depth.view(np.uint32), want_depth.view(np.uint32)), name


# ---- 4. subsets and ranks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["volume_ragged", "curves"])
def test_a_subset_of_planes_has_the_bits_of_the_full_pass(vpt, scenes, name):
    host, dev = scenes(name)
    params = params_of(vpt, name, 16)
    layout = layout_of(vpt, host, params)
    full, st = aov_pass(vpt, dev, params, layout, [3], FLOAT_PLANES + ("ids", "uvt"))
    for subset in [(n,) for n in FLOAT_PLANES + ("ids",)] + [("ids", "uvt")]:
        got, st2 = aov_pass(vpt, dev, params, layout, [3], subset)
        for n in subset:
            assert same(got[n], full[n]), (name, subset, n)
        assert same(st.hits, st2.hits) and same(st.rng, st2.rng), subset


def test_two_ranks_assemble_to_one(vpt, scenes):
    import torch
    name = "volume_ragged"
    host, dev = scenes(name)
    params = params_of(vpt, name, 16)
    one = layout_of(vpt, host, params)
    names = ("normal", "depth", "ids", "uvt")
    whole, st = aov_pass(vpt, dev, params, one, [3], names)
    w, h = one.width, one.height

    def rows(layout, planes):
        """the planes of all ranks -> row-major, through the two resolves"""
        out = {}
        for n in ("normal", "depth"):
            out[n] = torch.full((h * w, 4), FILL, dtype=torch.float32, device="cuda")
            vpt.resolve_device(layout, planes[n].data_ptr(), 3, out[n].data_ptr())
        out["ids"] = torch.full((h * w, 2), FILL_ID, dtype=torch.int32, device="cuda")
        out["uvt"] = torch.full((h * w, 3), FILL, dtype=torch.float32, device="cuda")
        vpt.resolve_ids_device(layout, planes["ids"].data_ptr(), planes["uvt"].data_ptr(), out["ids"].data_ptr(), out["uvt"].data_ptr())
        torch.cuda.synchronize()
        return out
    want = rows(one, whole)
    assert not bool((want["ids"] == FILL_ID).any()) and not bool((want["uvt"] == FILL).any())   # the gather writes every pixel

    layouts = [layout_of(vpt, host, params, r, 2) for r in (0, 1)]
    slots = vpt.layout_slots(layouts[0])
    gathered = {n: torch.cat([plane_buffers(State(vpt, lay), (n,))[n] for lay in layouts]) for n in names}   # [nranks][slots]
    for r, lay in enumerate(layouts):
        st_r = State(vpt, lay)
        before = {n: t.clone() for n, t in gathered.items()}
        part = {n: t[r * slots:(r + 1) * slots] for n, t in gathered.items()}
        dev.render_aov_device(params, lay, 3, {n: t.data_ptr() for n, t in part.items()}, st_r.hits.data_ptr(), st_r.rng.data_ptr())
        torch.cuda.synchronize()
        other = slice((1 - r) * slots, (2 - r) * slots)
        for n in names:
            assert same(gathered[n][other], before[n][other]), (r, n)   # the other rank's slots are not touched
        assert padding_kept(part, st_r)
    got = rows(layouts[0], gathered)
    for n in names:
        assert same(got[n], want[n]), n


# ---- 5. the session ---------------------------------------------------------------------------------------------------------------
def resolved(vpt, host, dev, params, n):
    st = host.make_state(params)
    dev.pathtrace_samples(st, params, n)
    return vpt.get_render(st)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", ["volume", "curves"])
def test_session_guides_equal_the_two_renders(vpt, scene_files, name):
    host = vpt.HostScene(scene_files[name])
    dev = vpt.DeviceScene(host, 0)
    s = vpt.RenderSession(dev, params_of(vpt, name, 8, "volpathtrace"), denoise=True, guide_samples=4)
    normal, albedo = s.guides()
    assert s.stats() == (0, 0, 2 * 16 * s.size[0] * s.size[1])
    s.advance(2)
    again = s.guides()   # advances leave the guides alone
    s.close()
    for got, shader in ((normal, "normal"), (albedo, "color")):
        want = resolved(vpt, host, dev, params_of(vpt, name, 4, shader), 4)
        assert np.array_equal(bits(got), bits(want)), (name, shader, int((bits(got) != bits(want)).any(axis=-1).sum()))
    assert np.array_equal(bits(again[0]), bits(normal)) and np.array_equal(bits(again[1]), bits(albedo))
    # and the host-state path behind pathtrace_guides goes through the same pass
    hn, ha = vpt.pathtrace_guides(host, dev, params_of(vpt, name, 8, "volpathtrace"), samples=4)
    assert np.array_equal(bits(hn), bits(normal)) and np.array_equal(bits(ha), bits(albedo))


def test_session_pick_and_ids(vpt, scene_files):
    host, dev = pinhole(vpt, scene_files, "crowd")
    params = params_of(vpt, "crowd", 8, "pathtrace")
    s = vpt.RenderSession(dev, params, pratio=4)
    w, h = s.size

    def check_frame():
        ids, uvt = s.ids()
        want_ids, want_uvt = dev.intersect(centre_rays(vpt, dev, w, h))
        assert np.array_equal(ids.reshape(-1, 2), want_ids) and np.array_equal(bits(uvt.reshape(-1, 3)), bits(want_uvt))
        return ids, uvt
    ids, uvt = check_frame()
    assert s.stats()[2] >= 20 * w * h
    table = dev.get_instances()
    hit_pixels = np.argwhere(ids[..., 0] >= 0)
    miss_pixels = np.argwhere(ids[..., 0] < 0)
    assert len(hit_pixels) and len(miss_pixels)
    y, x = (int(c) for c in hit_pixels[len(hit_pixels) // 2])
    p = s.pick(x, y)
    assert s.stats() == (1, 0, 24)   # one launch packs the record, 24 bytes cross the bus
    inst = p["instance"]
    assert (inst, p["element"]) == tuple(ids[y, x]) and (F(p["u"]), F(p["v"]), F(p["distance"])) == tuple(uvt[y, x])
    assert (p["shape"], p["material"]) == (int(table["shape"][inst]), int(table["material"][inst]))
    my, mx = (int(c) for c in miss_pixels[0])
    assert s.pick(mx, my) is None
    for bad in ((-1, 0), (w, 0), (0, h), (0, -1)):
        with pytest.raises(vpt.VptError, match="outside"):
            s.pick(*bad)
    assert vpt.hip.vpt_session_pick(s.handle, w, 0, None) == -1   # VPT_ERR_INVALID_ARG

    # the picked instance goes: the id frame is made anew, and never names what the scene no longer holds
    count = host.count("instances")
    host.remove_instances([inst])
    s.edit_instances(host.update_instances())
    ids2, _ = check_frame()
    assert ids2[..., 0].max() < count - 1 and not np.array_equal(ids2, ids)
    p2 = s.pick(x, y)
    assert (p2 is None) == (ids2[y, x, 0] < 0) and (p2 is None or (p2["instance"], p2["element"]) == tuple(ids2[y, x]))
    table2 = dev.get_instances()
    if p2 is not None:
        assert (p2["shape"], p2["material"]) == (int(table2["shape"][p2["instance"]]), int(table2["material"][p2["instance"]]))

    # a camera edit re-makes it too
    cam = host.camera(0)
    cam.lens *= 0.8
    host.set_camera(0, cam)
    s.edit(host.update_bvh())
    ids3, _ = check_frame()
    assert not np.array_equal(ids3, ids2)
    s.close()


def test_id_frame_follows_a_frame_of_equal_pixels_and_more_slots(vpt, scene_files):
    """105 x 40 and 100 x 42 hold 4200 pixels each but 70 and 78 tiles: the id frame's tile-major buffers are sized by the slots, so a
    reset from one to the other (with an edit in between that no pick follows) has to allocate them anew"""
    host, dev = pinhole(vpt, scene_files, "crowd")

    def set_aspect(w, h, apply):
        cam = host.camera(0)
        cam.aspect = w / h
        host.set_camera(0, cam)
        apply(host.update_bvh())

    def frame_equals_intersect(s):
        w, h = s.size
        ids, uvt = s.ids()
        want_ids, want_uvt = dev.intersect(centre_rays(vpt, dev, w, h))
        assert np.array_equal(ids.reshape(-1, 2), want_ids) and np.array_equal(bits(uvt.reshape(-1, 3)), bits(want_uvt)), (w, h)
        assert (want_ids[:, 0] >= 0).any() and (want_ids[:, 0] < 0).any()
        return ids, uvt
    set_aspect(105, 40, dev.update)
    s = vpt.RenderSession(dev, vpt.PathtraceParams(resolution=105, samples=4, shader="pathtrace", bounces=2), pratio=4)
    assert s.size == (105, 40)
    frame_equals_intersect(s)
    s.pick(50, 20)                              # the id frame and its 24-byte record exist at the first size
    set_aspect(100, 42, s.edit)                 # a reset to 105 x 44 that no pick follows
    assert s.size == (105, 44)
    s.reset(params=vpt.PathtraceParams(resolution=100, samples=4, shader="pathtrace", bounces=2))
    assert s.size == (100, 42)
    slots = [vpt.layout_slots(vpt.VptLayout(w, h, 8, 8, 0, 1)) for w, h in ((105, 40), (100, 42))]
    assert slots == [4480, 4992]
    ids, uvt = frame_equals_intersect(s)
    for x, y in ((0, 0), (99, 41), (50, 21), (97, 3)):   # the last tiles of the larger layout among them
        p = s.pick(x, y)
        assert (p is None) == (ids[y, x, 0] < 0)
        if p is not None:
            assert (p["instance"], p["element"]) == tuple(ids[y, x]) and F(p["distance"]) == uvt[y, x, 2]
    s.close()


def test_session_error_cases(vpt, scenes):
    import ctypes as C
    host, dev = scenes("volume")
    s = vpt.RenderSession(dev, params_of(vpt, "volume", 8, "volpathtrace"))   # denoise off
    buf = np.zeros((s.size[1], s.size[0], 4), F)
    assert vpt.hip.vpt_session_get_guides(s.handle, buf.ctypes.data, None) == -1 and b"denoise" in vpt.hip.vpt_last_error()
    assert vpt.hip.vpt_session_get_ids(s.handle, None, None) == -1
    s.close()
    ghost = vpt.HostScene(GRID)
    gdev = vpt.DeviceScene(ghost, 0)
    for shader in ("implicit", "implicit_normal"):
        g = vpt.RenderSession(gdev, vpt.PathtraceParams(resolution=64, samples=4, shader=shader, bounces=2))
        out = vpt.VptPick()
        assert vpt.hip.vpt_session_pick(g.handle, 1, 1, C.byref(out)) == -5 and b"implicit" in vpt.hip.vpt_last_error()   # VPT_ERR_UNSUPPORTED
        ids = np.zeros((g.size[1], g.size[0], 2), np.int32)
        assert vpt.hip.vpt_session_get_ids(g.handle, ids.ctypes.data, None) == -5
        g.close()


def test_device_entry_point_refuses_bad_planes(vpt, scenes):
    host, dev = scenes("volume")
    params = params_of(vpt, "volume", 4)
    layout = layout_of(vpt, host, params)
    st = State(vpt, layout)
    uvt = plane_buffers(st, ("uvt",))["uvt"]
    with pytest.raises(vpt.VptError, match="every plane is null"):
        dev.render_aov_device(params, layout, 1, {}, st.hits.data_ptr(), st.rng.data_ptr())
    with pytest.raises(vpt.VptError, match="uvt is given without ids"):
        dev.render_aov_device(params, layout, 1, {"uvt": uvt.data_ptr()}, st.hits.data_ptr(), st.rng.data_ptr())


def test_host_arrays_entry_point(vpt, scenes):
    """vpt_render_aov (DeviceScene.render_aovs): row-major planes in and out, batched, equal to the resolved debug renders"""
    host, dev = scenes("surface")
    params = params_of(vpt, "surface", 6)
    st = host.make_state(params)
    got = dev.render_aovs(st, params, 2)
    got = dev.render_aovs(st, params, 100, into=got)   # ends at the cap
    assert st.samples == 6 and (st.hits == 6).all()
    for plane, shader in SHADER_OF.items():
        p = params_of(vpt, "surface", 6, shader)
        want = host.make_state(p)
        dev.pathtrace_samples(want, p, 6)
        assert np.array_equal(bits(got[plane]), bits(want.image)), plane
        assert np.array_equal(st.rngs, want.rngs)
    assert got["ids"].shape == (st.height, st.width, 2) and (got["ids"][..., 0] >= 0).all()   # this camera shows geometry in every pixel
    hit_t = got["uvt"][..., 2]
    assert np.array_equal(bits(got["depth"][..., 3]), bits(np.full_like(hit_t, 6))) and (got["depth"][..., 0] > 0).all()
