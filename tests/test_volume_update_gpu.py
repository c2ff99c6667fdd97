"""vpt_scene_update_volumes on the GPU (include/vpt.h).  The criterion is equality of bits, no tolerance anywhere:
A = DeviceScene(original) after A.update_volumes(edit) of every step of a case (tests/volume_edits.py) against B = a DeviceScene made
from the host scene after the same steps and update_volumes().  Compared: renders with implicit and implicit_normal at 96 pixels (image
as uint32, rngs, hits), vpt_scene_get_volumes (whd and res of every volume - its offset is the resident pool's and no part of the
contract - and every instance and SDF byte for byte), vpt_scene_get_voxels of every volume, the six hashes of the light tables.  Fresh
handles are held to the reference by tests/test_gpu_parity.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import sdf_exact as X
import volume_edits as V
from bake_meshes import TOOTHED, bits, icosphere, toothed_grid, write_volume_scene
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
F = np.float32
SHADERS = ("implicit", "implicit_normal")


def path(scene_file):
    return os.path.join(GOLDEN, "scenes", scene_file)


def render(vpt, dev, host, shader, spp=2):
    p = vpt.PathtraceParams(resolution=96, samples=spp, shader=shader, bounces=4)
    st = host.make_state(p)
    dev.pathtrace_samples(st, p, spp)
    return st


def same_state(a, b):
    return (a.samples == b.samples and np.array_equal(a.image.view(np.uint32), b.image.view(np.uint32)) and np.array_equal(a.rngs, b.rngs)
            and np.array_equal(a.hits, b.hits))


def tables(dev):
    """what the getters give, the pool's layout left out: ((whd, res) per volume, instances' bytes, SDFs' bytes, voxels' bits per volume)"""
    vols, insts, sdfs = dev.get_volumes()
    return ([(tuple(v.whd), F(v.res).tobytes()) for v in vols], [bytes(i) for i in insts], [bytes(s) for s in sdfs],
            [bits(dev.get_voxels(k)).tobytes() for k in range(len(vols))])


def assert_same_everything(vpt, A, B, host, what):
    ta, tb = tables(A), tables(B)
    for part, a, b in zip(("volumes", "vol_instances", "sdfs", "voxels"), ta, tb):
        assert a == b, f"{what}: {part} differ from a fresh handle's"
    mirror = [bits(host.volume(k)[0]).tobytes() for k in range(len(ta[0]))]
    assert ta[3] == mirror, f"{what}: voxels differ from the host mirror's"
    assert A.light_tables_hash() == B.light_tables_hash(), f"{what}: light tables differ from a fresh handle's"
    la, lb = A.get_lights(), host.lights()
    assert la[0].tobytes() == lb[0].tobytes() and la[1].tobytes() == lb[1].tobytes(), f"{what}: lights differ from the host mirror's"
    for shader in SHADERS:
        assert same_state(render(vpt, A, host, shader), render(vpt, B, host, shader)), f"{what}: {shader} differs from a fresh handle's"


@pytest.fixture(scope="module")
def originals(vpt):
    """scene file -> (host scene, its six hashes, its render per shader, its tables) of the unedited scenes, made once and never edited"""
    out = {}
    for scene_file in (V.GRID, V.SDFS):
        host = vpt.HostScene(path(scene_file))
        dev = vpt.DeviceScene(host, 0)
        out[scene_file] = (host, dev.light_tables_hash(), {s: render(vpt, dev, host, s) for s in SHADERS}, tables(dev))
    return out


def updated_pair(vpt, name, originals):
    """(A, B, edited host scene, the VolumeEdits)"""
    scene_file = V.cases(vpt)[name][0]
    A = vpt.DeviceScene(vpt.HostScene(path(scene_file)), 0)
    host = vpt.HostScene(path(scene_file))
    edits = V.apply(vpt, name, host, after_step=A.update_volumes, original=originals[scene_file][0])
    assert all(not e.empty() for e in edits) and host.update_volumes().empty()
    return A, vpt.DeviceScene(host, 0), host, edits


@pytest.mark.parametrize("name", V.NAMES)
def test_update_volumes_equals_a_fresh_scene(vpt, originals, name):
    A, B, host, edits = updated_pair(vpt, name, originals)
    scene_file = V.cases(vpt)[name][0]
    print(f"{name}: {A.update_stats()} (launches, bytes, device ms); lights {A.get_lights()[0].tolist()}", flush=True)
    assert_same_everything(vpt, A, B, host, name)
    _, hashes, renders, before = originals[scene_file]
    differs = A.light_tables_hash() != hashes or tables(A) != before or any(not same_state(render(vpt, A, host, s), renders[s]) for s in SHADERS)
    assert differs == (name not in V.NO_OPS), name


@pytest.mark.parametrize("tag,scene_file", [("grid", V.GRID), ("sdfs", V.SDFS)])
def test_a_new_res_reaches_every_instance_of_the_volume(vpt, originals, tag, scene_file):
    """sackboy with res 2.5: the picture changes where its instances are (06_gridsdf_synth has two), nothing of the lights does, and
    one region kernel is all that is launched"""
    A, _, host, _ = updated_pair(vpt, f"vol_res_{tag}", originals)
    _, hashes, renders, _ = originals[scene_file]
    assert A.light_tables_hash() == hashes
    assert not same_state(render(vpt, A, host, "implicit_normal"), renders["implicit_normal"])
    launches, sent, _ = A.update_stats()
    nsdf, ninst = host.count_implicit("sdfs"), host.count_implicit("vol_instances")
    assert launches == 1 and sent == 48 ** 3 * 4 + 24 + 144 * nsdf + 112 * ninst


@pytest.mark.parametrize("tag,scene_file", [("grid", V.GRID), ("sdfs", V.SDFS)])
def test_sdf_lights_follow_material_and_whd(vpt, originals, tag, scene_file):
    """the list grows and shrinks with an entry's material, the lamp's CDF entry follows its whd, and off-then-on is the original"""
    original, hashes, renders, _ = originals[scene_file]
    A, _, host, _ = updated_pair(vpt, f"light_on_{tag}", originals)
    lights, cdf = A.get_lights()
    assert [int(l["sdf"]) for l in lights] == [-1, V.FLOOR, V.LAMP] and cdf[-2:].tobytes() == np.array([F(2) * F(1e-5), F(0.5) * F(0.4)], F).tobytes()
    A, _, host, _ = updated_pair(vpt, f"light_off_{tag}", originals)
    assert [int(l["sdf"]) for l in A.get_lights()[0]] == [-1]
    A, _, host, _ = updated_pair(vpt, f"light_whd_{tag}", originals)
    lights, cdf = A.get_lights()
    assert [int(l["sdf"]) for l in lights] == [-1, V.LAMP] and cdf[-1:].tobytes() == np.array([F(0.3) * F(0.6)], F).tobytes()
    assert A.light_tables_hash() != hashes and A.light_tables_hash()[0] == hashes[0]   # the list stays, the CDF pool does not
    A, _, host, _ = updated_pair(vpt, f"light_off_on_{tag}", originals)
    assert A.light_tables_hash() == hashes and host.stats() == original.stats()
    for s, st in renders.items():
        assert same_state(st, render(vpt, A, original, s)), s


def test_an_edit_without_light_consequence_leaves_the_light_tables(vpt, originals):
    """a turned torus: nothing of the lights is sent or launched"""
    A, _, host, _ = updated_pair(vpt, "sdf_turned", originals)
    launches, sent, _ = A.update_stats()
    assert launches == 0 and sent == 84 + 144 * 10 + 112 * 2
    assert A.light_tables_hash() == originals[V.SDFS][1]


def test_a_plane_more_is_counted(vpt, originals):
    """sdf_num_planes has no getter: the mirror holds two planes now, and the device renders what a fresh handle does (the test above)"""
    A, B, host, _ = updated_pair(vpt, "sdf_to_plane", originals)
    assert [vpt.SDF_TYPES[host.sdf(k).type] for k in range(10)].count("plane") == 2
    assert [vpt.SDF_TYPES[s.type] for s in A.get_volumes()[2]].count("plane") == 2


@pytest.mark.parametrize("tag", V.TAGS)
def test_regrown_volumes_are_rebased_and_the_others_stay(vpt, originals, tag):
    scene_file = V.GRID if tag == "grid" else V.SDFS
    A, _, host, _ = updated_pair(vpt, f"grow_{tag}", originals)
    vols = A.get_volumes()[0]
    assert vols[V.SACKBOY].offset == 0 and vols[V.BUNNY].offset == 48 ** 3 + 40 ** 3 and tuple(vols[V.BUNNY].whd) == (44, 41, 37)
    assert tables(A)[3][V.SACKBOY] == originals[scene_file][3][3][V.SACKBOY]
    A, _, host, _ = updated_pair(vpt, f"regrow_both_{tag}", originals)
    vols = A.get_volumes()[0]
    assert [v.offset for v in vols] == [48 ** 3 + 40 ** 3, 48 ** 3 + 40 ** 3 + 50 * 49 * 48]


# ---- bakes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", V.TAGS)
@pytest.mark.parametrize("form", ["whole", "region", "union"])
def test_a_bake_equals_the_host_mirror_combined_on_the_host(vpt, originals, tag, form):
    """the resident 17 x 9 x 5 grid after the bake against bake_sdf_grid(device=None) combined with the grid before it, in numpy"""
    name = f"bake_{form}_{tag}"
    scene_file = V.cases(vpt)[name][0]
    A = vpt.DeviceScene(vpt.HostScene(path(scene_file)), 0)
    host = vpt.HostScene(path(scene_file))
    seen = []
    V.apply(vpt, name, host, after_step=lambda e: (A.update_volumes(e), seen.append(A.get_voxels(V.BUNNY))), original=originals[scene_file][0])
    resident, got = seen
    assert resident.shape == V.SMALL[::-1]
    want = V.baked_small(vpt, resident, V.REGION if form == "region" else None, V.UNION if form == "union" else V.REPLACE)
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(got), bits(resident)) and (form == "whole") == (not np.any(bits(got) == bits(resident)))
    launches, sent, _ = A.update_stats()
    assert launches == 1


def test_a_brute_bake_gives_the_same_bits():
    """VPT_BAKE_BRUTE=1 in a child process, as the existing tests of such switches do"""
    env = dict(os.environ, VPT_BAKE_BRUTE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", f"{__file__}::test_a_bake_equals_the_host_mirror_combined_on_the_host[region-grid]",
                        f"{__file__}::test_update_volumes_equals_a_fresh_scene[bake_union_sdfs]"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def one_volume_scene(vpt, tmp_path, whd, res, frame):
    vpt.save_volume(str(tmp_path / "flat.sdf"), np.ones(whd[::-1], F), res)
    write_volume_scene(tmp_path / "scene.json", "flat.sdf", frame, 1.0)
    return str(tmp_path / "scene.json")


def test_bake_bytes_do_not_depend_on_the_grid(vpt, tmp_path):
    """a bake entry counts its nodes and records and not one voxel: the same mesh into 8^3 and into 16^3 sends the same bytes"""
    verts, tris = icosphere(2, 0.3)
    sent = []
    for n in (8, 16):
        res, origin, step, frame = vpt.fit_volume(verts.min(axis=0), verts.max(axis=0), n, 2)
        host = vpt.HostScene(one_volume_scene(vpt, tmp_path, (n, n, n), res, frame))
        A = vpt.DeviceScene(host, 0)
        host.bake_volume(0, verts, tris, origin=origin, step=step)
        A.update_volumes(host.update_volumes())
        sent.append(A.update_stats()[1])
        assert np.array_equal(bits(A.get_voxels(0)), bits(vpt.bake_sdf_grid(verts, tris, n, origin, step, device=None)[0]))
    assert sent[0] == sent[1] and sent[0] < 8 ** 3 * 4 + 320 * 200


FAN_REGION = ((7, 5, 3), (10, 9, 14))   # lo and size (x, y, z) in the 21^3 grid: no multiple of a brick, across brick borders, around the fan's inside


@pytest.mark.parametrize("mode", [V.REPLACE, V.UNION])
def test_a_fan_baked_into_a_region_has_the_mirrors_bits_and_the_exact_signs(vpt, tmp_path, mode):
    """fan_spike(8) through HostScene.bake_volume into a region of a resident 21^3 grid that held a sphere's distance field (below the
    baked values in part of the region, above them elsewhere): the mirror combined in numpy with the grid before the bake, bit for
    bit; and in REPLACE mode the region's signs are the winding number's (tests/sdf_exact.py), no voxel within 1e-5 of the surface"""
    verts, tris = TOOTHED["fan_8"][0]()
    n = 21
    origin, step = toothed_grid("fan_8", n)
    origin = np.full(3, origin, F)
    k = np.arange(n, dtype=F)
    z, y, x = np.meshgrid(k, k, k, indexing="ij")
    field = (np.sqrt((x - 10) ** 2 + (y - 10) ** 2 + (z - 8) ** 2) * F(0.1) - F(0.45)).astype(F)
    vpt.save_volume(str(tmp_path / "field.sdf"), field, 0.05)
    write_volume_scene(tmp_path / "scene.json", "field.sdf", np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0]], F), 1.0)
    host = vpt.HostScene(str(tmp_path / "scene.json"))
    A = vpt.DeviceScene(host, 0)
    resident = A.get_voxels(0)
    assert np.array_equal(bits(resident), bits(field))
    host.bake_volume(0, verts, tris, origin=origin, step=step, region=FAN_REGION, mode=mode)
    A.update_volumes(host.update_volumes())
    got = A.get_voxels(0)
    mirror, _ = vpt.bake_sdf_grid(verts, tris, n, origin, step, device=None)
    want = resident.copy()
    box, b = V.box_of(want, *FAN_REGION), V.box_of(mirror, *FAN_REGION)
    assert ((box < b).sum() > 100 and (box > b).sum() > 100)   # a union keeps some voxels and replaces others
    box[...] = V.union(box, b) if mode == V.UNION else b
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(got), bits(resident)) and A.update_stats()[0] == 1
    if mode == V.REPLACE:
        exact, inside = X.signed_distance(X.sample_points(n, origin, step), verts, tris)
        assert np.abs(exact).min() >= 1e-5 and V.box_of(inside, *FAN_REGION).sum() == inside.sum() >= 40
        assert np.array_equal(np.signbit(V.box_of(got, *FAN_REGION)), V.box_of(inside, *FAN_REGION))


def test_a_baked_sphere_renders_as_the_oracle_does(vpt, oracle, tmp_path):
    """an icosphere of radius 0.3 baked at 32^3 into a resident volume that held a flat field, rendered with implicit_normal on the GPU
    and by the oracle over the host mirror: the criterion and the floors of test_bake_sdf_gpu.py's test_baked_grid_renders"""
    from test_gpu_parity import _check_against_reference
    verts, tris = icosphere(2, 0.3)
    res, origin, step, frame = vpt.fit_volume(verts.min(axis=0), verts.max(axis=0), 32, 2)
    scene = vpt.HostScene(one_volume_scene(vpt, tmp_path, (32, 32, 32), res, frame))
    dev = vpt.DeviceScene(scene, 0)
    scene.bake_volume(0, verts, tris, origin=origin, step=step)
    dev.update_volumes(scene.update_volumes())
    assert np.array_equal(bits(dev.get_voxels(0)), bits(vpt.bake_sdf(verts, tris, 32, device=None).voxels))
    spp = 2
    p = vpt.PathtraceParams(resolution=48, samples=spp, shader="implicit_normal", bounces=4)
    g = scene.make_state(p)
    dev.pathtrace_samples(g, p, spp)
    ref = scene.make_state(p)
    oracle.oracle_render(scene, p, ref, spp, nthreads=0)
    _check_against_reference(oracle, scene, p, spp, g, ref.image, ref.rngs, "resident_baked_sphere_normal_48_2", 0.998, 0.998, 0.998)
    assert g.hits[g.height // 2, g.width // 2] == spp


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _inst(vpt, host, index=0, **kw):
    vi = host.volume_instance(index)
    for k, v in kw.items():
        setattr(vi, k, v)
    return vi


def _sdf(vpt, host, index=0, **kw):
    f = host.sdf(index)
    for k, v in kw.items():
        if k in ("whd", "p"):
            getattr(f, k)[:] = v
        else:
            setattr(f, k, v)
    return f


def _nan_frame(vpt, host):
    vi = host.volume_instance(0)
    vi.frame.o[1] = float("nan")
    return vi


def _src(vpt, whd=(40, 40, 40), lo=(0, 0, 0), size=(1, 1, 1), mode=0, res=0.0036, voxels=None, bake=None):
    return vpt.VolumeSource(whd, res, lo, size, mode, np.zeros(size[::-1], F) if voxels is None and bake is None else voxels, bake)


def _bake_of(tris=None, origin=0.0):
    verts, t = icosphere(1, 0.3)
    return (verts, t if tris is None else tris, origin, 0.05)


REFUSALS = {   # one per class of rule in include/vpt.h
    "instance id out of range": lambda vpt, h: vpt.VolumeEdit(vol_instances={99: _inst(vpt, h)}),
    "instance id negative": lambda vpt, h: vpt.VolumeEdit(vol_instances={-1: _inst(vpt, h)}),
    "instance frame NaN": lambda vpt, h: vpt.VolumeEdit(vol_instances={0: _nan_frame(vpt, h)}),
    "instance scalef infinite": lambda vpt, h: vpt.VolumeEdit(vol_instances={0: _inst(vpt, h, scalef=float("inf"))}),
    "instance volume out of range": lambda vpt, h: vpt.VolumeEdit(vol_instances={0: _inst(vpt, h, volume=2)}),
    "instance material out of range": lambda vpt, h: vpt.VolumeEdit(vol_instances={0: _inst(vpt, h, material=1000)}),
    "sdf id out of range": lambda vpt, h: vpt.VolumeEdit(sdfs={99: _sdf(vpt, h)}),
    "sdf type 6": lambda vpt, h: vpt.VolumeEdit(sdfs={0: _sdf(vpt, h, type=6)}),
    "sdf type negative": lambda vpt, h: vpt.VolumeEdit(sdfs={0: _sdf(vpt, h, type=-1)}),
    "sdf material negative": lambda vpt, h: vpt.VolumeEdit(sdfs={0: _sdf(vpt, h, material=-1)}),
    "sdf whd NaN": lambda vpt, h: vpt.VolumeEdit(sdfs={1: _sdf(vpt, h, 1, whd=[float("nan"), 1.0, 1.0])}),
    "sdf parameter infinite": lambda vpt, h: vpt.VolumeEdit(sdfs={1: _sdf(vpt, h, 1, p=[1.0, float("inf"), 0.0, 0.0])}),
    "volume id out of range": lambda vpt, h: vpt.VolumeEdit(volumes={2: _src(vpt)}),
    "volume res NaN": lambda vpt, h: vpt.VolumeEdit(volumes={1: _src(vpt, res=float("nan"))}),
    "volume whd negative": lambda vpt, h: vpt.VolumeEdit(volumes={1: _src(vpt, whd=(-1, 40, 40), size=(0, 0, 0))}),
    "volume of 2^31 voxels": lambda vpt, h: vpt.VolumeEdit(volumes={1: _src(vpt, whd=(2048, 1024, 1024), size=(0, 0, 0))}),
    "region past the grid": lambda vpt, h: vpt.VolumeEdit(volumes={1: _src(vpt, lo=(38, 0, 0), size=(3, 1, 1))}),
    "region lo negative": lambda vpt, h: vpt.VolumeEdit(volumes={1: _src(vpt, lo=(0, -1, 0))}),
    "mode 2": lambda vpt, h: vpt.VolumeEdit(volumes={1: _src(vpt, mode=2)}),
    "a new whd with a partial region": lambda vpt, h: vpt.VolumeEdit(volumes={1: _src(vpt, whd=(8, 8, 8), size=(8, 8, 7))}),
    "a new whd in UNION mode": lambda vpt, h: vpt.VolumeEdit(volumes={1: _src(vpt, whd=(8, 8, 8), size=(8, 8, 8), mode=1)}),
    "bake of another whd": lambda vpt, h: vpt.VolumeEdit(volumes={1: vpt.VolumeSource((40, 40, 40), 0.0036, (0, 0, 0), (40, 40, 40), 0, None, _bake_of())}),
    "bake with a triangle index out of range": lambda vpt, h: vpt.VolumeEdit(volumes={1: _src(vpt, size=(40, 40, 40), bake=_bake_of(np.array([[0, 1, 4000]], np.int32)))}),
    "bake with an infinite origin": lambda vpt, h: vpt.VolumeEdit(volumes={1: _src(vpt, size=(40, 40, 40), bake=_bake_of(None, float("inf")))}),
    "a good entry beside a bad one": lambda vpt, h: vpt.VolumeEdit(sdfs={1: _sdf(vpt, h, 1, whd=[1.0, 1.0, 1.0]), 0: _sdf(vpt, h, type=9)}, volumes={0: _src(vpt, (48, 48, 48), res=1.0)}),
}


@pytest.fixture(scope="module")
def untouched(vpt, originals):
    host = vpt.HostScene(path(V.GRID))
    return vpt.DeviceScene(host, 0), host


@pytest.mark.parametrize("what", list(REFUSALS))
def test_a_refused_edit_leaves_the_scene_untouched(vpt, originals, untouched, what):
    dev, host = untouched
    _, hashes, renders, before = originals[V.GRID]
    edit = REFUSALS[what](vpt, host)
    abi, keep = edit.to_abi()
    if what == "bake of another whd":
        vpt.VptBakeDesc.from_address(C.cast(abi.volumes, C.POINTER(vpt.VptVolumeSource))[0].bake).whd[0] = 39
    rc = vpt.hip.vpt_scene_update_volumes(dev.handle, C.byref(abi))
    message = vpt.hip.vpt_last_error().decode()
    assert rc == -1 and "entry" in message, (what, rc, message)
    assert tables(dev) == before and dev.light_tables_hash() == hashes
    assert same_state(render(vpt, dev, host, "implicit"), renders["implicit"])


def test_offsets_past_the_edits_pool_are_refused(vpt, untouched, originals):
    dev, host = untouched
    abi, keep = vpt.VolumeEdit(volumes={1: _src(vpt, size=(2, 2, 2))}).to_abi()
    for offset, count in ((1, 8), (-2, 8), (0, 7)):
        entries = C.cast(abi.volumes, C.POINTER(vpt.VptVolumeSource))
        entries[0].offset, abi.num_voxels = offset, count
        assert vpt.hip.vpt_scene_update_volumes(dev.handle, C.byref(abi)) == -1 and "entry 0" in vpt.hip.vpt_last_error().decode()
    assert tables(dev) == originals[V.GRID][3]


def _repeated(vpt, host, what):
    """a vpt_volume_edit that names an id twice, filled in by hand: VolumeEdit keeps dictionaries and cannot say it"""
    keep, abi = [], vpt.VptVolumeEdit()
    ids = np.array([1, 1], np.int32)
    keep.append(ids)
    if what == "vol_instance":
        entries = (vpt.VptVolumeInstance * 2)(_inst(vpt, host, 1, scalef=0.5), _inst(vpt, host, 1, scalef=0.25))
        abi.num_vol_instances, abi.vol_instance_ids, abi.vol_instances = 2, ids.ctypes.data, C.cast(entries, C.c_void_p).value
    elif what == "sdf":
        entries = (vpt.VptSdf * 2)(_sdf(vpt, host, 1, whd=[1.0, 1.0, 1.0]), _sdf(vpt, host, 1, whd=[2.0, 2.0, 2.0]))
        abi.num_sdfs, abi.sdf_ids, abi.sdfs = 2, ids.ctypes.data, C.cast(entries, C.c_void_p).value
    else:   # two entries for volume 1, each with a new whd: accepted, they would take two places in the pool for one volume
        voxels = np.full(2 * 8 ** 3, -1.0, F)
        entries = (vpt.VptVolumeSource * 2)()
        for k in range(2):
            e = entries[k]
            e.whd[:], e.res, e.region_lo[:], e.region_whd[:], e.mode, e.offset = [8, 8, 8], 0.5, [0, 0, 0], [8, 8, 8], 0, 8 ** 3 * k
        if what == "volume, host and bake":
            verts, tris = icosphere(1, 0.3)
            desc = vpt.VptBakeDesc(len(verts), verts.ctypes.data, len(tris), tris.ctypes.data)
            desc.whd[:], desc.origin[:], desc.step[:] = [8, 8, 8], [-0.5] * 3, [0.125] * 3
            entries[1].offset, entries[1].bake = -1, C.addressof(desc)
            keep += [verts, tris, desc]
        abi.num_volumes, abi.volume_ids, abi.volumes = 2, ids.ctypes.data, C.cast(entries, C.c_void_p).value
        abi.num_voxels, abi.voxels = len(voxels), voxels.ctypes.data
        keep.append(voxels)
    keep.append(entries)
    return abi, keep


@pytest.mark.parametrize("what", ["vol_instance", "sdf", "volume, two host entries", "volume, host and bake"])
def test_a_repeated_id_is_refused(vpt, untouched, originals, what):
    """ids are not repeated within a list - which is also all that keeps a volume from being named by a host entry and a bake entry,
    or regrown twice, in one call: refused with the entry's number, getters, hashes and a render unchanged"""
    dev, host = untouched
    _, hashes, renders, before = originals[V.GRID]
    abi, keep = _repeated(vpt, host, what)
    rc = vpt.hip.vpt_scene_update_volumes(dev.handle, C.byref(abi))
    message = vpt.hip.vpt_last_error().decode()
    assert rc == -1 and "entry 1" in message and "repeated" in message, (what, rc, message)
    assert tables(dev) == before and dev.light_tables_hash() == hashes
    assert same_state(render(vpt, dev, host, "implicit"), renders["implicit"])
    # each half alone is a good edit (on a handle of its own): it is the repetition that is refused
    abi.num_vol_instances, abi.num_sdfs, abi.num_volumes = min(abi.num_vol_instances, 1), min(abi.num_sdfs, 1), min(abi.num_volumes, 1)
    other = vpt.DeviceScene(host, 0)
    assert vpt.hip.vpt_scene_update_volumes(other.handle, C.byref(abi)) == 0, vpt.hip.vpt_last_error().decode()
    assert tables(other) != before


def test_a_voxel_count_that_overflows_is_refused(vpt, untouched, originals):
    """whd whose product passes 2^63 and wraps must not pass as a small one; an offset near 2^63 must not wrap into the pool"""
    dev, host = untouched
    for whd in ((1 << 21, 1 << 21, 1 << 22), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (65536, 65536, 1)):
        abi, keep = vpt.VolumeEdit(volumes={1: _src(vpt, whd=whd, size=(0, 0, 0))}).to_abi()
        assert vpt.hip.vpt_scene_update_volumes(dev.handle, C.byref(abi)) == -1 and "2^31" in vpt.hip.vpt_last_error().decode(), whd
    abi, keep = vpt.VolumeEdit(volumes={1: _src(vpt, size=(2, 2, 2))}).to_abi()
    C.cast(abi.volumes, C.POINTER(vpt.VptVolumeSource))[0].offset = 2 ** 63 - 4
    assert vpt.hip.vpt_scene_update_volumes(dev.handle, C.byref(abi)) == -1 and "entry 0" in vpt.hip.vpt_last_error().decode()
    assert tables(dev) == originals[V.GRID][3]


def test_a_tree_too_deep_is_unsupported_and_nothing_is_written(vpt, untouched, originals):
    from synth_scenes import chain_geometry
    dev, host = untouched
    verts, tris = chain_geometry(50)
    src = vpt.VolumeSource((40, 40, 40), 1.0, (0, 0, 0), (40, 40, 40), 0, None, (verts, tris, -2.0, 0.5))
    moved = _inst(vpt, host, 0, scalef=2.0)
    abi, keep = vpt.VolumeEdit(vol_instances={0: moved}, volumes={1: src}).to_abi()
    assert vpt.hip.vpt_scene_update_volumes(dev.handle, C.byref(abi)) == -5, vpt.hip.vpt_last_error().decode()
    assert "depth" in vpt.hip.vpt_last_error().decode()
    assert tables(dev) == originals[V.GRID][3]


# ---- beside the other updates, in a session, on a vpt_multi --------------------------------------------------------------------------
KINDS = ("update", "update_lights", "update_textures", "update_volumes")


@pytest.mark.parametrize("first", KINDS)
def test_other_updates_on_the_same_handle(vpt, originals, first):
    """update (the camera), update_lights (a material's emission: the lamp's, so the SDF light goes), update_textures (the sky dimmed)
    and update_volumes on one handle: each kind as the first edit the fresh handle sees, the other three after it in that order"""
    import scene_edits as E
    A = vpt.DeviceScene(vpt.HostScene(path(V.GRID)), 0)
    host = vpt.HostScene(path(V.GRID))

    def update():
        E.edit_camera(host)
        A.update(host.update_bvh())

    def update_lights():
        m = host.material(V.LAMP_MATERIAL)
        m.emission[:] = [0.0, 0.0, 0.0]
        host.set_material(V.LAMP_MATERIAL, m)
        A.update_lights(host.update_lights())

    def update_textures():
        host.set_environment(0, emission=(0.25, 0.25, 0.25))
        A.update_textures(host.update_textures())

    def update_volumes():
        for name in ("region_grid", "inst_turn_grid", "light_on_grid"):
            V.apply(vpt, name, host, after_step=A.update_volumes, original=originals[V.GRID][0])

    steps = {"update": update, "update_lights": update_lights, "update_textures": update_textures, "update_volumes": update_volumes}
    for kind in [first] + [k for k in KINDS if k != first]:
        steps[kind]()
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, f"first={first}")
    V.apply(vpt, "grow_grid", host, after_step=A.update_volumes, original=originals[V.GRID][0])
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, f"first={first}, then grow")


def test_session_edit_volumes(vpt, originals):
    """session bits = make_state + vpt_render on the edited scene"""
    host = vpt.HostScene(path(V.SDFS))
    dev = vpt.DeviceScene(host, 0)
    p = vpt.PathtraceParams(resolution=96, samples=4, shader="implicit", bounces=4)
    session = vpt.RenderSession(dev, p, pratio=8)
    session.advance(2)
    for name in ("sdf_sphere_to_torus", "union_nan_sdfs", "bake_region_sdfs"):
        V.apply(vpt, name, host, after_step=session.edit_volumes, original=originals[V.SDFS][0])
    assert session.samples == 0
    session.advance(3)
    want = host.make_state(p)
    vpt.DeviceScene(host, 0).pathtrace_samples(want, p, 3)
    assert same_state(session.state(), want)
    with pytest.raises(vpt.VptError):
        session.edit_volumes(vpt.VolumeEdit(sdfs={0: _sdf(vpt, host, type=7)}))
    assert session.samples == 3 and same_state(session.state(), want)
    session.close()


def test_multi_update_volumes_on_one_device(vpt, originals):
    host = vpt.HostScene(path(V.GRID))
    multi = vpt.MultiDeviceScene(host, [0])
    for name in ("shrink_grid", "light_whd_grid", "bake_union_grid"):
        V.apply(vpt, name, host, after_step=multi.update_volumes, original=originals[V.GRID][0])
    B = vpt.DeviceScene(host, 0)
    for shader in SHADERS:
        p = vpt.PathtraceParams(resolution=96, samples=2, shader=shader, bounces=4)
        a, b = host.make_state(p), host.make_state(p)
        multi.pathtrace_samples(a, p, 2)
        B.pathtrace_samples(b, p, 2)
        assert same_state(a, b), shader
    with pytest.raises(vpt.VptError):
        multi.update_volumes(vpt.VolumeEdit(sdfs={0: _sdf(vpt, host, type=7)}))
    multi.close()
