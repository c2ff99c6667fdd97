"""vpt_scene_update_volume_set on the GPU (include/vpt.h).  The criterion is equality of bits, no tolerance anywhere:
A = DeviceScene(original) after every step of a case (tests/volume_set_edits.py) was applied to it - update_volume_set, and where the case
has them update_volumes and sculpt_volumes - against B = a DeviceScene made from the host scene after the same steps.  Compared: renders
with implicit and implicit_normal at 96 pixels (volgrid too on 10_volgrid_synth), vpt_scene_get_volumes (offsets included where the edit
laid the pool out anew: the running sum of W*H*D), vpt_scene_get_voxels of every volume, the six hashes of the light tables, the brick
majorants of every volume.  Fresh handles are held to the reference by tests/test_gpu_parity.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import volume_edits as V
import volume_set_edits as W
from bake_meshes import bits
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
F = np.float32
SHADERS = ("implicit", "implicit_normal")


def path(scene_file):
    return os.path.join(GOLDEN, "scenes", scene_file)


def load(vpt, scene_file):
    """the scene; the cloud's medium gets a usable trdepth, as tests/test_volgrid_gpu.py gives it"""
    h = vpt.HostScene(path(scene_file))
    if scene_file == W.CLOUD:
        m = h.material(0)
        m.scattering[:], m.scanisotropy, m.trdepth = [0.8] * 3, 0.6, 0.25
        h.set_material(0, m)
        h.update_bvh()
    return h


def shaders_of(scene_file):
    return SHADERS + (("volgrid",) if scene_file == W.CLOUD else ())


def render(vpt, dev, host, shader, spp=2):
    p = vpt.PathtraceParams(resolution=96, samples=spp, shader=shader, bounces=4)
    st = host.make_state(p)
    dev.pathtrace_samples(st, p, spp)
    return st


def same_state(a, b):
    return (a.samples == b.samples and np.array_equal(a.image.view(np.uint32), b.image.view(np.uint32)) and np.array_equal(a.rngs, b.rngs)
            and np.array_equal(a.hits, b.hits))


def tables(dev, offsets=True):
    """what the getters give: ((whd, res, offset) per volume, instances' bytes, SDFs' bytes, voxels' bits per volume)"""
    vols, insts, sdfs = dev.get_volumes()
    return ([(tuple(v.whd), F(v.res).tobytes(), v.offset if offsets else 0) for v in vols], [bytes(i) for i in insts], [bytes(s) for s in sdfs],
            [bits(dev.get_voxels(k)).tobytes() for k in range(len(vols))])


def applier(A):
    return lambda kind, edit: {"set": A.update_volume_set, "volumes": A.update_volumes, "sculpt": A.sculpt_volumes}[kind](edit)


def assert_same_everything(vpt, A, B, host, what, scene_file, offsets=True):
    ta, tb = tables(A, offsets), tables(B, offsets)
    for part, a, b in zip(("volumes", "vol_instances", "sdfs", "voxels"), ta, tb):
        assert a == b, f"{what}: {part} differ from a fresh handle's"
    if offsets:
        sizes = [w * h * d for (w, h, d), _, _ in ta[0]]
        assert [o for _, _, o in ta[0]] == [sum(sizes[:k]) for k in range(len(sizes))], f"{what}: the pool has gaps"
    mirror = [bits(host.volume(k)[0]).tobytes() for k in range(len(ta[0]))]
    assert ta[3] == mirror, f"{what}: voxels differ from the host mirror's"
    assert A.light_tables_hash() == B.light_tables_hash(), f"{what}: light tables differ from a fresh handle's"
    la, lb = A.get_lights(), host.lights()
    assert la[0].tobytes() == lb[0].tobytes() and la[1].tobytes() == lb[1].tobytes(), f"{what}: lights differ from the host mirror's"
    for k in range(len(ta[0])):
        assert np.array_equal(bits(A.volgrid_majorants(k)), bits(B.volgrid_majorants(k))), f"{what}: majorants of volume {k}"
    for shader in shaders_of(scene_file):
        assert same_state(render(vpt, A, host, shader), render(vpt, B, host, shader)), f"{what}: {shader} differs from a fresh handle's"


@pytest.fixture(scope="module")
def originals(vpt):
    """scene file -> (host scene, its six hashes, its render per shader, its tables) of the unedited scenes, made once and never edited"""
    out = {}
    for scene_file in (W.GRID, W.SDFS, W.CLOUD):
        host = load(vpt, scene_file)
        dev = vpt.DeviceScene(host, 0)
        out[scene_file] = (host, dev.light_tables_hash(), {s: render(vpt, dev, host, s) for s in shaders_of(scene_file)}, tables(dev))
    return out


def updated_pair(vpt, name, originals):
    """(A, B, the edited host scene)"""
    scene_file = W.scene_of(vpt, name)
    A = vpt.DeviceScene(load(vpt, scene_file), 0)
    A.volgrid_majorants(0)   # the brick tables exist before the edit
    host = load(vpt, scene_file)
    W.apply(vpt, name, host, after_step=applier(A), original=originals[scene_file][0])
    assert host.update_volume_set().empty()
    return A, vpt.DeviceScene(host, 0), host


@pytest.mark.parametrize("name", W.NAMES)
def test_update_volume_set_equals_a_fresh_scene(vpt, originals, name):
    scene_file = W.scene_of(vpt, name)
    A, B, host = updated_pair(vpt, name, originals)
    print(f"{name}: {A.update_stats()} (launches, bytes, device ms); lights {A.get_lights()[0].tolist()}; volumes {[(tuple(v.whd), v.offset) for v in A.get_volumes()[0]]}", flush=True)
    assert A.volgrid_stats()["table_builds"] == 1   # the edit itself builds nothing: the next query does
    assert_same_everything(vpt, A, B, host, name, scene_file, offsets=name in W.MOVES_POOL)
    assert A.volgrid_stats()["table_builds"] == 2   # grown by one, however many queries and renders followed
    _, hashes, renders, before = originals[scene_file]
    assert tables(A) != before and any(not same_state(render(vpt, A, host, s), renders[s]) for s in shaders_of(scene_file))


def test_the_brick_tables_are_rebuilt_once(vpt, originals):
    A, B, host = updated_pair(vpt, "second_cloud", originals)
    assert A.volgrid_stats()["table_builds"] == 1
    assert np.array_equal(bits(A.volgrid_majorants(1)), bits(host.volgrid_majorants(1))) and A.volgrid_stats()["table_builds"] == 2
    A.volgrid_majorants(0)
    render(vpt, A, host, "volgrid")
    assert A.volgrid_stats()["table_builds"] == 2


@pytest.mark.parametrize("tag", W.TAGS)
def test_everything_removed_renders_only_misses(vpt, originals, tag):
    scene_file = W.GRID if tag == "grid" else W.SDFS
    A = vpt.DeviceScene(load(vpt, scene_file), 0)
    host = load(vpt, scene_file)
    W.note(vpt, host, W.cases(vpt)[f"empty_then_one_{tag}"][1][0][1])
    A.update_volume_set(host.update_volume_set())
    assert [len(t) for t in A.get_volumes()] == [0, 0, 0] and [int(l["sdf"]) for l in A.get_lights()[0]] == [-1]
    for shader in SHADERS:
        assert same_state(render(vpt, A, host, shader), render(vpt, vpt.DeviceScene(host, 0), host, shader))


@pytest.mark.parametrize("tag", W.TAGS)
def test_the_lights_follow_the_sdf_numbering(vpt, originals, tag):
    scene_file = W.GRID if tag == "grid" else W.SDFS
    hashes = originals[scene_file][1]
    A, _, host = updated_pair(vpt, f"light_shifts_{tag}", originals)
    assert [int(l["sdf"]) for l in A.get_lights()[0]] == [-1, 0] and A.light_tables_hash()[0] != hashes[0] and A.light_tables_hash()[1] == hashes[1]
    A, _, host = updated_pair(vpt, f"light_removed_{tag}", originals)
    assert [int(l["sdf"]) for l in A.get_lights()[0]] == [-1]
    A, _, host = updated_pair(vpt, f"light_added_{tag}", originals)
    lights, cdf = A.get_lights()
    assert [int(l["sdf"]) for l in lights][-2:] == [1, host.count_implicit("sdfs") - 1] and cdf[-1:].tobytes() == np.array([F(0.3) * F(0.2)], F).tobytes()


def test_an_edit_without_light_consequence_leaves_the_light_tables(vpt, originals):
    """a sphere added and a sphere behind the lamp removed: nothing of the lights is sent or launched, no volume is touched: no gather"""
    A = vpt.DeviceScene(load(vpt, W.SDFS), 0)
    host = load(vpt, W.SDFS)
    host.remove_sdfs([5])
    host.add_sdf(type="sphere", p=(0.03,), material=4, frame=W.frame_at(0.2, 0.0, 0.1))
    A.update_volume_set(host.update_volume_set())
    launches, sent, _ = A.update_stats()
    assert launches == 0 and sent == 24 * 2 + (60 + 112) * 2 + (84 + 144) * 10
    assert A.light_tables_hash() == originals[W.SDFS][1] and tables(A)[0] == originals[W.SDFS][3][0]
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, "sdf swapped", W.SDFS, offsets=False)


# ---- bakes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", W.TAGS)
def test_a_baked_addition_has_the_bits_of_vpt_bake_sdf(vpt, originals, tag):
    A, _, host = updated_pair(vpt, f"bake_new_{tag}", originals)
    verts, tris = V.sphere_mesh()
    res, origin, step, _ = V.small_fit(vpt)
    want, _ = vpt.bake_sdf_grid(verts, tris, V.SMALL, origin, step, device=0)
    got = A.get_voxels(2)
    assert got.shape == V.SMALL[::-1] and np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(got), bits(vpt.bake_sdf_grid(verts, tris, V.SMALL, origin, step, device=None)[0]))
    launches, sent, _ = A.update_stats()
    assert launches == 2   # the gather and the bake


def test_a_brute_bake_gives_the_same_bits():
    """VPT_BAKE_BRUTE=1 in a child process, as the existing tests of such switches do"""
    env = dict(os.environ, VPT_BAKE_BRUTE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", f"{__file__}::test_a_baked_addition_has_the_bits_of_vpt_bake_sdf[grid]",
                        f"{__file__}::test_update_volume_set_equals_a_fresh_scene[bake_new_sdfs]"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_the_bytes_do_not_depend_on_a_filled_volumes_size(vpt):
    """the same edit with an 8^3 and a 16^3 FILL volume sends the same bytes: 32 per segment and the small tables, not one voxel"""
    sent = []
    for n in (8, 16):
        host = load(vpt, W.GRID)
        A = vpt.DeviceScene(host, 0)
        host.add_volume(fill=0.5, whd=(n, n, n), res=0.01)
        host.add_volume_instance(W.frame_at(0, 0, 0), 2, 3)
        A.update_volume_set(host.update_volume_set())
        launches, nbytes, _ = A.update_stats()
        sent.append(nbytes)
        assert launches == 1 and np.array_equal(bits(A.get_voxels(2)), bits(np.full((n, n, n), 0.5, F)))
    assert sent[0] == sent[1] == 3 * 32 + 3 * 24 + 5 * (60 + 112) + 2 * (84 + 144)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def untouched(vpt):
    host = load(vpt, W.GRID)
    return vpt.DeviceScene(host, 0), host


def _new(vpt, **kw):
    out = dict(whd=(2, 2, 2), res=0.5, source=vpt.VOLUME_FILL)
    out.update(kw)
    return vpt.VolumeNew(**out)


def _inst(vpt, volume=0, material=0, scalef=1.0, frame=None):
    vi = vpt.VptVolumeInstance(volume=volume, material=material, scalef=scalef)
    C.memmove(C.byref(vi.frame), np.ascontiguousarray(W.frame_at(0, 0, 0) if frame is None else frame, F).ctypes.data, 48)
    return vi


def _sdf(vpt, type=1, material=0, whd=(1, 1, 1), p=(0, 0, 0, 0), frame=None):
    f = vpt.VptSdf(type=type, material=material)
    C.memmove(C.byref(f.frame), np.ascontiguousarray(W.frame_at(0, 0, 0) if frame is None else frame, F).ctypes.data, 48)
    f.whd[:], f.p[:] = [float(v) for v in whd], [float(v) for v in p]
    return f


# (The one class of refusal without an entry below is the pool's new total: 2^43 voxels need 2^12 added volumes of 2^31 - 1 voxels
# each, 8 TiB of payload or of resident sources - no caller can build that edit, here or elsewhere.)
def refusals(vpt):
    """name -> (a VolumeSetEdit, what to do to its struct, a word of the message) on 06_gridsdf_synth (2 volumes, 4 instances, 2 SDFs, 8 materials)"""
    E = vpt.VolumeSetEdit
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    nanf = W.frame_at(0, np.nan, 0)

    def null(field):
        return lambda abi: setattr(abi, field, None)

    def count(field, value):
        return lambda abi: setattr(abi, field, value)

    def offset(value):
        return lambda abi: setattr(C.cast(abi.add_volumes, C.POINTER(vpt.VptVolumeNew))[0], "offset", value)
    return {
        "null remove list": (E(remove_sdfs=[0]), null("remove_sdf_ids"), "null"),
        "null add_volumes": (E(add_volumes=[_new(vpt)]), null("add_volumes"), "null"),
        "null add_vol_instances": (E(add_vol_instances=[_inst(vpt)]), null("add_vol_instances"), "null"),
        "null add_sdfs": (E(add_sdfs=[_sdf(vpt)]), null("add_sdfs"), "null"),
        "null voxels": (E(add_volumes=[_new(vpt, source=0, voxels=np.zeros((2, 2, 2), F))]), null("voxels"), "null"),
        "negative remove count": (E(remove_volumes=[]), count("num_remove_volumes", -1), "negative"),
        "negative add count": (E(), count("num_add_sdfs", -2), "negative"),
        "negative voxel count": (E(add_sdfs=[_sdf(vpt)]), count("num_voxels", -1), "negative"),
        "instance id out of range": (E(remove_vol_instances=[4]), None, "out of range"),
        "sdf id out of range": (E(remove_sdfs=[-1]), None, "out of range"),
        "volume id out of range": (E(remove_volumes=[2], remove_vol_instances=[0, 1, 2, 3]), None, "out of range"),
        "instance id repeated": (E(remove_vol_instances=[1, 1]), None, "repeated"),
        "sdf id repeated": (E(remove_sdfs=[0, 1, 0]), None, "repeated"),
        "volume id repeated": (E(remove_volumes=[0, 0], remove_vol_instances=[0, 1]), None, "repeated"),
        "removed volume named by a survivor": (E(remove_volumes=[1], remove_vol_instances=[2]), None, "still named"),
        "added instance past the new list": (E(remove_volumes=[1], remove_vol_instances=[2, 3], add_vol_instances=[_inst(vpt, volume=1)]), None, "volume 1 out of range"),
        "added instance volume negative": (E(add_vol_instances=[_inst(vpt, volume=-1)]), None, "out of range"),
        "added instance material": (E(add_vol_instances=[_inst(vpt, material=8)]), None, "material 8"),
        "added sdf material": (E(add_sdfs=[_sdf(vpt, material=-1)]), None, "material -1"),
        "instance frame not finite": (E(add_vol_instances=[_inst(vpt, frame=nanf)]), None, "not finite"),
        "instance scalef not finite": (E(add_vol_instances=[_inst(vpt, scalef=np.inf)]), None, "not finite"),
        "sdf frame not finite": (E(add_sdfs=[_sdf(vpt, frame=nanf)]), None, "not finite"),
        "sdf whd not finite": (E(add_sdfs=[_sdf(vpt, whd=(1, np.inf, 1))]), None, "not finite"),
        "sdf p not finite": (E(add_sdfs=[_sdf(vpt, p=(0, 0, np.nan, 0))]), None, "not finite"),
        "sdf type": (E(add_sdfs=[_sdf(vpt, type=6)]), None, "type 6"),
        "res not finite": (E(add_volumes=[_new(vpt, res=np.nan)]), None, "res"),
        "negative whd": (E(add_volumes=[_new(vpt, whd=(2, -1, 2))]), None, "negative whd"),
        "2^31 voxels": (E(add_volumes=[_new(vpt, whd=(2048, 1024, 1024))]), None, "2^31"),
        "a product that wraps": (E(add_volumes=[_new(vpt, whd=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1))]), None, "2^31"),
        "payload too short": (E(add_volumes=[_new(vpt, source=0, voxels=np.zeros((2, 2, 2), F))]), count("num_voxels", 7), "payload"),
        "offset negative": (E(add_volumes=[_new(vpt, source=0, voxels=np.zeros((2, 2, 2), F))]), offset(-1), "payload"),
        "offset that wraps": (E(add_volumes=[_new(vpt, source=0, voxels=np.zeros((2, 2, 2), F))]), offset(2 ** 63 - 4), "payload"),
        "source unknown": (E(add_volumes=[_new(vpt, source=4)]), None, "source 4"),
        "copy_of out of range": (E(add_volumes=[_new(vpt, whd=(48, 48, 48), source=3, copy_of=2)]), None, "copy_of 2"),
        "copy of another size": (E(add_volumes=[_new(vpt, whd=(40, 40, 40), source=3, copy_of=0)]), None, "whd differs"),
        "bake without a descriptor": (E(add_volumes=[_new(vpt, source=1, bake=(tri, [[0, 1, 2]], 0.0, 0.1))]),
                                      lambda abi: setattr(C.cast(abi.add_volumes, C.POINTER(vpt.VptVolumeNew))[0], "bake", None), "bake"),
        "bake vertex index out of range": (E(add_volumes=[_new(vpt, source=1, bake=(tri, [[0, 1, 3]], 0.0, 0.1))]), None, "bake"),
        "bake of another whd": (E(add_volumes=[_new(vpt, source=1, bake=(tri, [[0, 1, 2]], 0.0, 0.1))]),
                                lambda abi: vpt.VptBakeDesc.from_address(C.cast(abi.add_volumes, C.POINTER(vpt.VptVolumeNew))[0].bake).whd.__setitem__(0, 3), "whd"),
    }


def test_every_refused_edit_leaves_getters_and_render_unchanged(vpt, untouched, originals):
    dev, host = untouched
    _, hashes, renders, before = originals[W.GRID]
    for name, (edit, tamper, word) in refusals(vpt).items():
        abi, keep = edit.to_abi()
        if tamper:
            tamper(abi)
        rc = vpt.hip.vpt_scene_update_volume_set(dev.handle, C.byref(abi))
        message = vpt.hip.vpt_last_error().decode()
        assert rc == -1 and word in message and "volume_set" in message, (name, rc, message)
    assert vpt.hip.vpt_scene_update_volume_set(dev.handle, None) == -1 and vpt.hip.vpt_scene_update_volume_set(None, C.byref(abi)) == -1
    assert tables(dev) == before and dev.light_tables_hash() == hashes
    for s in SHADERS:
        assert same_state(render(vpt, dev, host, s), renders[s]), s


def test_the_handle_counts_its_own_lists(vpt, originals):
    """vpt_scene_count_implicit follows the edits, whatever the descriptor the handle was made from held"""
    counts = (C.c_int32 * 3)()
    A = vpt.DeviceScene(load(vpt, W.SDFS), 0)
    assert vpt.hip.vpt_scene_count_implicit(A.handle, C.cast(counts, C.c_void_p)) == 0 and list(counts) == [2, 2, 10]
    A.update_volume_set(vpt.VolumeSetEdit(remove_sdfs=[3, 4], add_volumes=[_new(vpt)], add_vol_instances=[_inst(vpt, volume=2), _inst(vpt, volume=0)]))
    assert vpt.hip.vpt_scene_count_implicit(A.handle, C.cast(counts, C.c_void_p)) == 0 and list(counts) == [3, 4, 8]
    assert [len(t) for t in A.get_volumes()] == [3, 4, 8]
    assert vpt.hip.vpt_scene_count_implicit(A.handle, None) == -1 and vpt.hip.vpt_scene_count_implicit(None, C.cast(counts, C.c_void_p)) == -1


def test_an_empty_edit_does_nothing(vpt, untouched, originals):
    dev, host = untouched
    host.set_sdf(0, material=0)   # an edit whose counters stay: (0 launches, its bytes)
    dev.update_volumes(host.update_volumes())
    stats = dev.update_stats()[:2]
    dev.update_volume_set(vpt.VolumeSetEdit())
    assert dev.update_stats()[:2] == stats and tables(dev) == originals[W.GRID][3] and dev.volgrid_stats()["table_builds"] == 0


def test_a_tree_too_deep_is_unsupported_and_nothing_is_written(vpt, untouched, originals):
    from synth_scenes import chain_geometry
    dev, host = untouched
    verts, tris = chain_geometry(50)
    edit = vpt.VolumeSetEdit(remove_sdfs=[0], add_volumes=[vpt.VolumeNew((40, 40, 40), 1.0, vpt.VOLUME_FROM_BAKE, bake=(verts, tris, -2.0, 0.5))],
                             add_vol_instances=[_inst(vpt, volume=2)])
    abi, keep = edit.to_abi()
    assert vpt.hip.vpt_scene_update_volume_set(dev.handle, C.byref(abi)) == -5, vpt.hip.vpt_last_error().decode()
    assert "depth" in vpt.hip.vpt_last_error().decode()
    assert tables(dev) == originals[W.GRID][3] and dev.light_tables_hash() == originals[W.GRID][1]
    abi, keep = vpt.VolumeSetEdit(remove_sdfs=[0], add_volumes=[_new(vpt)], add_vol_instances=[_inst(vpt, volume=2)]).to_abi()   # a smaller edit works afterwards
    assert vpt.hip.vpt_scene_update_volume_set(dev.handle, C.byref(abi)) == 0, vpt.hip.vpt_last_error().decode()
    assert [len(t) for t in dev.get_volumes()] == [3, 5, 1]
    back = vpt.VolumeSetEdit(remove_volumes=[2], remove_vol_instances=[4], remove_sdfs=[0], add_sdfs=[host.sdf(0), host.sdf(1)])
    dev.update_volume_set(back)   # and back: the lists of the original, the lamp behind the floor again
    assert tables(dev) == originals[W.GRID][3] and dev.light_tables_hash() == originals[W.GRID][1]


# ---- beside the other updates, in a session, on a vpt_multi --------------------------------------------------------------------------
@pytest.mark.parametrize("set_first", [True, False])
def test_interleaved_with_the_other_updates(vpt, originals, set_first):
    """a set edit before and after vpt_scene_update (the camera), _lights (the lamp's emission), _textures (the sky), _volumes (an SDF, a
    regrown volume) and _sculpt_volumes on one handle"""
    import scene_edits as E
    A = vpt.DeviceScene(load(vpt, W.GRID), 0)
    host = load(vpt, W.GRID)

    def others():
        E.edit_camera(host)
        A.update(host.update_bvh())
        m = host.material(W.LAMP_MATERIAL)
        m.emission[:] = [0.0, 0.0, 0.0]
        host.set_material(W.LAMP_MATERIAL, m)
        A.update_lights(host.update_lights())
        host.set_environment(0, emission=(0.25, 0.25, 0.25))
        A.update_textures(host.update_textures())
        last = host.count_implicit("volumes") - 1
        host.set_sdf(0, whd=(1.5, 1e-5, 1.5))
        host.set_volume(last, W.smooth((11, 7, 5), 4, 0.02), 0.02)
        A.update_volumes(host.update_volumes())
        host.sculpt_volume(last, W.sculpt_case(vpt, last)[1])
        A.sculpt_volumes(host.update_sculpts())

    def set_edits():
        for name in ("add_host_grid", "light_added_grid"):
            W.apply(vpt, name, host, after_step=applier(A))
        host.remove_volumes([0])
        host.remove_volume_instances([0, 1])
        host.remove_sdfs([0])
        A.update_volume_set(host.update_volume_set())

    for step in ((set_edits, others) if set_first else (others, set_edits)):
        step()
    B = vpt.DeviceScene(host, 0)
    assert_same_everything(vpt, A, B, host, f"set_first={set_first}", W.GRID, offsets=not set_first)
    host.add_volume(copy_of=0)
    A.update_volume_set(host.update_volume_set())
    assert_same_everything(vpt, A, vpt.DeviceScene(host, 0), host, f"set_first={set_first}, then a copy", W.GRID)


def test_session_edit_volume_set(vpt, originals):
    """session bits = make_state + vpt_render on the edited scene, and pick_sdf reports the new ids"""
    host = load(vpt, W.SDFS)
    dev = vpt.DeviceScene(host, 0)
    p = vpt.PathtraceParams(resolution=96, samples=4, shader="implicit", bounces=4)
    session = vpt.RenderSession(dev, p, pratio=8)
    session.advance(2)
    before, _ = session.sdf_ids()   # an id frame of the old numbering exists before the edit
    assert before[..., 0].max() == 1 and before[..., 1].max() >= 8
    W.apply(vpt, "remove_first_sdfs", host, after_step=lambda kind, e: session.edit_volume_set(e))
    host.remove_sdfs([0])   # the floor: every SDF behind it gets another id
    session.edit_volume_set(host.update_volume_set())
    assert session.samples == 0
    session.advance(2)
    want = host.make_state(p)
    vpt.DeviceScene(host, 0).pathtrace_samples(want, p, 2)
    assert same_state(session.state(), want)
    ids, _ = session.sdf_ids()
    assert ids[..., 0].max() == 0 and 0 < ids[..., 1].max() <= 8   # one grid instance and nine SDFs are left
    y, x = (int(c) for c in np.argwhere(ids[..., 0] == 0)[0])
    pick = session.pick_sdf(x, y)
    assert (pick["vol_instance"], pick["sdf"], pick["volume"], pick["material"]) == (0, -1, 0, host.volume_instance(0).material)
    for k in np.unique(ids[..., 1][ids[..., 1] >= 0]):
        y, x = (int(c) for c in np.argwhere(ids[..., 1] == k)[0])
        pick = session.pick_sdf(x, y)
        assert (pick["vol_instance"], pick["sdf"], pick["volume"], pick["material"]) == (-1, int(k), -1, host.sdf(int(k)).material)
    with pytest.raises(vpt.VptError):
        session.edit_volume_set(vpt.VolumeSetEdit(remove_sdfs=[9]))
    assert session.samples == 2 and same_state(session.state(), want)   # a refused edit leaves the session as it was
    session.close()


def test_a_multi_device_scene_follows(vpt, originals):
    host = load(vpt, W.GRID)
    multi = vpt.MultiDeviceScene(host, [0])
    for name in ("copy_swap_grid", "bake_new_grid", "light_shifts_grid"):
        W.apply(vpt, name, host, after_step=lambda kind, e: multi.update_volume_set(e))
    B = vpt.DeviceScene(host, 0)
    for shader in SHADERS:
        p = vpt.PathtraceParams(resolution=96, samples=2, shader=shader, bounces=4)
        a, b = host.make_state(p), host.make_state(p)
        multi.pathtrace_samples(a, p, 2)
        B.pathtrace_samples(b, p, 2)
        assert same_state(a, b), shader
    with pytest.raises(vpt.VptError):
        multi.update_volume_set(vpt.VolumeSetEdit(remove_volumes=[0]))
    multi.close()
