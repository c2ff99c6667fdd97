"""Edits of volumes, grid instances and SDFs, shared by the volume-update tests (tests/test_volume_update_host.py,
tests/test_volume_update_gpu.py) and the fixture script (tests/golden/make_volume_edit_fixtures.py).  A case is (scene file, [step, ...]): every step takes a HostScene and changes it through
set_volume_instance / set_sdf / set_volume / bake_volume; the caller runs update_volumes() after each step.  What a step writes is
computed here in numpy (a bake: by the host mirror of the bake, combined here), float32 operation by operation, from the scene as loaded - never read back from the scene under test - so
that the same values can be written out as an edited scene file with its .sdf (write_edited_scene) for a fresh load and for the
reference.

06_gridsdf_synth: volume 0 = sackboy (48^3, res 3; instances 0 and 1, scale 0.001), volume 1 = bunny (40^3, res 0.0036; instances 2
and 3); SDF 0 = the floor box (material 0), SDF 1 = an emissive box (material 1), the scene's one SDF light.
07_sdfunction_synth: the same two volumes with one instance each (0: sackboy, 1: bunny) and ten SDFs: the two boxes, then a capped
cone, a torus, spheres 4, 5, 6, a bbox, a plane (8) and sphere 9."""
import os

import numpy as np

import scene_edits as E
from bake_meshes import icosphere

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = os.path.join(HERE, "golden", "scenes")
GRID = "06_gridsdf_synth/gridsdf_synth.json"
SDFS = "07_sdfunction_synth/sdfunction_synth.json"
F = np.float32
SACKBOY, BUNNY = 0, 1        # volumes of both scenes
FLOOR, LAMP = 0, 1           # SDFs of both scenes: the floor box, the emissive box
LAMP_MATERIAL = 1
REPLACE, UNION = 0, 1
REGION = ((1, 2, 3), (5, 3, 2))   # lo and size, each (x, y, z): no multiple of a brick, across brick borders
SMALL = (17, 9, 5)                # whd of the volume the bakes go into


def frame12(f):
    return np.array(list(f.x) + list(f.y) + list(f.z) + list(f.o), F)


def box_of(grid, lo, size):
    """the box lo .. lo + size (x, y, z) of a (d, h, w) grid"""
    return grid[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]]


def union(a, b):
    """op_union (yocto_sdfs.h:82): (a < b) ? a : b - the select; with a NaN on either side the comparison is false and b is taken"""
    with np.errstate(invalid="ignore"):
        return np.where(a < b, a, b).astype(F)


def incoming(shape, seed, nans=0):
    """(d, h, w) incoming voxels in [-0.02, 0.02), `nans` of them NaN"""
    rng = np.random.default_rng(seed)
    v = ((rng.random(shape, dtype=F) - F(0.5)) * F(0.04)).astype(F)
    if nans:
        v.reshape(-1)[rng.choice(v.size, nans, replace=False)] = np.nan
    return v


# ---- what a voxel case makes of a volume: (the grid as loaded, its res) -> (the whole new grid, the new res) ---------------------
def grid_region(old, res, lo=REGION[0], size=REGION[1], seed=5, mode=REPLACE, nans=0):
    new = old.copy()
    box = box_of(new, lo, size)
    b = incoming(box.shape, seed, nans)
    box[...] = union(box, b) if mode == UNION else b
    return new, res


def grid_shifted(old, res, new_res):
    return (old + F(0.5)).astype(F), new_res


def grid_resized(old, res, whd, seed, new_res=None, middle=True):
    """a smooth field of another size: the distance to a sphere in the middle of the grid (or around its first voxel), in voxels times res"""
    w, h, d = whd if middle else (0, 0, 0)
    z, y, x = np.meshgrid(np.arange(whd[2], dtype=F), np.arange(whd[1], dtype=F), np.arange(whd[0], dtype=F), indexing="ij")
    r = F(0.3 * min(whd)) + F(seed % 3)
    dist = np.sqrt(((x - F(w / 2)) ** 2 + (y - F(h / 2)) ** 2 + (z - F(d / 2)) ** 2).astype(F)).astype(F)
    new_res = res if new_res is None else new_res
    return ((dist - r) * F(new_res)).astype(F), new_res


# a voxel case: volume -> (function of (old, res), region or None for the whole grid, mode, seed arguments for the incoming box)
def set_voxels(volume, make, region=None, mode=REPLACE, **kw):
    """step: volume := make(volume as loaded), sent as the region's box (the whole grid when region is None)"""
    def step(h, work, original):
        old, res = original.volume(volume)
        new, new_res = make(old, res)
        if region is None:
            h.set_volume(volume, new, new_res)
        else:   # what crosses is the INCOMING box, not the result: the union happens where the voxels live
            lo, size = region
            h.set_volume(volume, incoming(box_of(old, lo, size).shape, kw.get("seed", 5), kw.get("nans", 0)), new_res, region=region, mode=mode)
    step.volumes = {volume: make}
    return step


def several(*steps):
    def step(h, work, original):
        for s in steps:
            s(h, work, original)
    step.volumes = {k: v for s in steps for k, v in getattr(s, "volumes", {}).items()}
    step.changes = [c for s in steps for c in getattr(s, "changes", [])]
    return step


def instance(index, json_change, **fields):
    """step: fields of a grid instance; frame may be a function of the frame as it is"""
    def step(h, work, original):
        f = dict(fields)
        if callable(f.get("frame")):
            f["frame"] = f["frame"](frame12(h.volume_instance(index).frame))
        h.set_volume_instance(index, **f)
    step.changes = [lambda d: json_change(d["vol_instances"][index])]
    return step


def sdf(index, json_change, **fields):
    def step(h, work, original):
        f = dict(fields)
        if callable(f.get("frame")):
            f["frame"] = f["frame"](frame12(h.sdf(index).frame))
        h.set_sdf(index, **f)
    step.changes = [lambda d: json_change(d["sdfunctions"][index])]
    return step


def turned(frame):
    return E.rotate_frame(frame, 0.4)


def stretched(frame):
    out = np.array(frame, F).copy()
    out[0:3] = (out[0:3] * F(1.5)).astype(F)
    return out


def _set(**values):
    def change(entry):
        for k, v in values.items():
            if v is None:
                entry.pop(k, None)
            else:
                entry[k] = v
    return change


def _frame(make):
    def change(entry):
        entry["frame"] = [float(v) for v in make(np.array(entry.get("frame", [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]), F))]
    return change


def _torus(entry):
    for k in ("radius", "whd", "thickness", "height"):
        entry.pop(k, None)
    entry.update(type="torus", r1=float(F(0.05)), r2=float(F(0.02)))


def _plane(entry):
    for k in ("radius", "whd", "thickness", "height", "r1", "r2"):
        entry.pop(k, None)
    entry["type"] = "plane"


# ---- the bakes: a 320-triangle icosphere into a resident 17 x 9 x 5 volume -----------------------------------------------------
def sphere_mesh():
    return icosphere(2, 0.05, (0.0, 0.06, 0.0))


def small_fit(vpt):
    """(res, origin, step, frame) of the 17 x 9 x 5 grid around the icosphere (fit_volume; one voxel of padding: five deep)"""
    verts, _ = sphere_mesh()
    return vpt.fit_volume(verts.min(axis=0), verts.max(axis=0), SMALL, 1)


def small_resident(vpt):
    return grid_resized(None, None, SMALL, 1, F(small_fit(vpt)[0]), middle=False)


def make_small(vpt, volume=BUNNY, inst=None):
    """step: the volume shrinks to 17 x 9 x 5 (a smooth field, res of the fit: a sphere around the first voxel, below the baked
    distances near it and above them far from it, so that a union keeps some voxels and replaces others) and one instance moves to
    the fit's frame"""
    res, origin, step_, frame = small_fit(vpt)
    shrink = set_voxels(volume, lambda old, r: small_resident(vpt))

    def step(h, work, original):
        shrink(h, work, original)
        i = inst if inst is not None else [k for k in range(h.count_implicit("vol_instances")) if h.volume_instance(k).volume == volume][0]
        h.set_volume_instance(i, frame=frame.reshape(12), scalef=1.0)

    def in_file(d):
        entries = d["vol_instances"]
        entry = entries[inst] if inst is not None else [e for e in entries if e["volume"] == volume][0]
        entry.update(frame=[float(v) for v in frame.reshape(12)], scale=1.0)
    step.volumes, step.changes = shrink.volumes, [in_file]
    return step


def bake(vpt, volume=BUNNY, region=None, mode=REPLACE):
    def step(h, work, original):
        verts, tris = sphere_mesh()
        res, origin, step_, _ = small_fit(vpt)
        h.bake_volume(volume, verts, tris, whd=SMALL, res=res, origin=origin, step=step_, region=region, mode=mode)
    # in a scene file: the host mirror of the bake combined in numpy with the grid the steps before left
    step.volumes = {volume: lambda old, res: (baked_small(vpt, old, region, mode), res)}
    return step


def baked_small(vpt, resident, region=None, mode=REPLACE):
    """what a bake step leaves in the small volume, by the host mirror of the bake combined here: resident is the grid before it"""
    verts, tris = sphere_mesh()
    res, origin, step_, _ = small_fit(vpt)
    grid, _ = vpt.bake_sdf_grid(verts, tris, SMALL, origin, step_, device=None)
    lo, size = ((0, 0, 0), SMALL) if region is None else region
    out = resident.copy()
    box, b = box_of(out, lo, size), box_of(grid, lo, size)
    box[...] = union(box, b) if mode == UNION else b
    return out


def cases(vpt):
    """name -> (scene file, [step, ...]); the names that end in a scene's tag run on that scene"""
    out = {}
    for tag, scene in (("grid", GRID), ("sdfs", SDFS)):
        bunny_inst = 2 if scene == GRID else 1
        out.update({
            f"inst_turn_{tag}": (scene, [instance(0, _frame(turned), frame=turned)]),
            f"inst_scalef_{tag}": (scene, [instance(bunny_inst, _set(scale=1.25), scalef=1.25)]),
            f"inst_material_{tag}": (scene, [instance(0, _set(material=4), material=4)]),
            f"inst_volume_{tag}": (scene, [instance(0, _set(volume=BUNNY, scale=1.0), volume=BUNNY, scalef=1.0)]),
            f"vol_res_{tag}": (scene, [set_voxels(SACKBOY, lambda old, res: grid_shifted(old, res, F(2.5)))]),
            f"sdf_nonrigid_{tag}": (scene, [sdf(LAMP, _frame(stretched), frame=stretched)]),
            f"light_whd_{tag}": (scene, [sdf(LAMP, _set(whd=[float(F(0.3)), float(F(0.6)), float(F(1e-5))]), whd=(0.3, 0.6, 1e-5))]),
            f"light_on_{tag}": (scene, [sdf(FLOOR, _set(material=LAMP_MATERIAL), material=LAMP_MATERIAL)]),
            f"light_off_{tag}": (scene, [sdf(LAMP, _set(material=0), material=0)]),
            f"light_off_on_{tag}": (scene, [sdf(LAMP, _set(material=0), material=0), sdf(LAMP, _set(material=LAMP_MATERIAL), material=LAMP_MATERIAL)]),
            f"region_{tag}": (scene, [set_voxels(BUNNY, grid_region, REGION)]),
            f"region_one_{tag}": (scene, [set_voxels(BUNNY, lambda o, r: grid_region(o, r, (39, 0, 17), (1, 1, 1), 7), ((39, 0, 17), (1, 1, 1)), seed=7)]),
            f"region_all_{tag}": (scene, [set_voxels(BUNNY, lambda o, r: grid_region(o, r, (0, 0, 0), (40, 40, 40), 8), ((0, 0, 0), (40, 40, 40)), seed=8)]),
            f"union_nan_{tag}": (scene, [set_voxels(BUNNY, lambda o, r: grid_region(o, r, (8, 9, 10), (23, 21, 19), 9, UNION, 40),
                                                    ((8, 9, 10), (23, 21, 19)), UNION, seed=9, nans=40)]),
            # NaN on either side: the first step leaves NaN voxels resident, the second unites over them
            f"union_nan_both_{tag}": (scene, [set_voxels(BUNNY, lambda o, r: grid_region(o, r, (8, 9, 10), (23, 21, 19), 11, REPLACE, 30),
                                                         ((8, 9, 10), (23, 21, 19)), REPLACE, seed=11, nans=30),
                                              set_voxels(BUNNY, lambda o, r: grid_region(o, r, (8, 9, 10), (23, 21, 19), 9, UNION, 40),
                                                         ((8, 9, 10), (23, 21, 19)), UNION, seed=9, nans=40)]),
            f"grow_{tag}": (scene, [set_voxels(BUNNY, lambda o, r: grid_resized(o, r, (44, 41, 37), 2))]),
            f"shrink_{tag}": (scene, [set_voxels(SACKBOY, lambda o, r: grid_resized(o, r, (21, 30, 11), 3))]),
            f"regrow_both_{tag}": (scene, [several(set_voxels(SACKBOY, lambda o, r: grid_resized(o, r, (50, 49, 48), 4)),
                                                   set_voxels(BUNNY, lambda o, r: grid_resized(o, r, (33, 35, 31), 5)))]),
            f"bake_whole_{tag}": (scene, [make_small(vpt), bake(vpt)]),
            f"bake_region_{tag}": (scene, [make_small(vpt), bake(vpt, region=REGION)]),
            f"bake_union_{tag}": (scene, [make_small(vpt), bake(vpt, mode=UNION)]),
        })
    out.update({
        "sdf_sphere_to_torus": (SDFS, [sdf(4, _torus, type="torus", p=(0.05, 0.02))]),
        "sdf_to_plane": (SDFS, [sdf(9, _plane, type="plane", p=(0, 0, 0, 0))]),
        "sdf_turned": (SDFS, [sdf(3, _frame(turned), frame=turned)]),
    })
    return out


TAGS = ("grid", "sdfs")
PER_SCENE = ["inst_turn", "inst_scalef", "inst_material", "inst_volume", "vol_res", "sdf_nonrigid", "light_whd", "light_on", "light_off", "light_off_on",
             "region", "region_one", "region_all", "union_nan", "union_nan_both", "grow", "shrink", "regrow_both", "bake_whole", "bake_region", "bake_union"]
NAMES = [f"{n}_{t}" for n in PER_SCENE for t in TAGS] + ["sdf_sphere_to_torus", "sdf_to_plane", "sdf_turned"]
NO_OPS = ("light_off_on_grid", "light_off_on_sdfs")   # constructed to return to the original
BAKES = tuple(n for n in NAMES if n.startswith("bake_"))
# every case can be written out as a scene file with its .sdf; a bake's grid is the host mirror of the bake, combined in numpy
AS_SCENE_FILE = list(NAMES)


def apply(vpt, name, h, work=None, after_step=None, original=None):
    """every step of a case on HostScene h, update_volumes() after each; after_step(edit) sees each VolumeEdit.  Returns the edits."""
    scene_file, steps = cases(vpt)[name]
    original = original or vpt.HostScene(os.path.join(SCENES, scene_file))
    edits = []
    for step in steps:
        step(h, work, original)
        edits.append(h.update_volumes())
        if after_step:
            after_step(edits[-1])
    return edits


def write_edited_scene(vpt, name, out, original=None):
    """the scene file of a case under directory `out` (a pathlib.Path), its edited volumes as binary .sdf files beside it, made from
    the numpy side of the case alone (for a bake step: bake_sdf_grid(device=None) combined here with the grid before it); returns its path"""
    scene_file, steps = cases(vpt)[name]
    original = original or vpt.HostScene(os.path.join(SCENES, scene_file))

    grids = {}   # volume -> (grid, res) as the steps so far leave it

    def change(d):
        for step in steps:
            for c in getattr(step, "changes", []):
                c(d)
            for volume, make in getattr(step, "volumes", {}).items():
                grid, res = grids[volume] = make(*grids.get(volume, original.volume(volume)))
                target = out / os.path.basename(os.path.dirname(scene_file))
                target.mkdir(exist_ok=True)
                vpt.save_volume(str(target / f"edited_{volume}.sdf"), grid, float(res))
                d["volumes"][volume].update(uri=f"edited_{volume}.sdf", binary=True)
    return E.write_scene_variant(out, os.path.join(SCENES, scene_file), change)


# Cases the reference also renders (tests/golden/make_volume_edit_fixtures.py -> volume_edit_states.npz): name -> (shader, resolution,
# samples), resolution 96 with 2 to 4 samples
STATE_CASES = {"inst_turn_grid": ("implicit", 96, 2), "vol_res_grid": ("implicit_normal", 96, 2), "union_nan_grid": ("implicit_normal", 96, 2),
               "sdf_sphere_to_torus": ("implicit", 96, 2), "light_whd_sdfs": ("implicit", 96, 3), "light_on_sdfs": ("implicit", 96, 2)}
