"""Additions and removals of volumes, grid instances and SDFs, shared by the volume-set tests (tests/test_volume_set_host.py,
tests/test_volume_set_gpu.py) and the fixture script (tests/golden/make_volume_set_fixtures.py).  A case is (scene file, [step, ...]).
A step is ("set", [op, ...]) - ops noted on a HostScene through add_volume / remove_volumes / add_volume_instance /
remove_volume_instances / add_sdf / remove_sdfs and handed out by update_volume_set() - or ("regrow", volume, whd, seed) and
("sculpt", volume): one set_volume / sculpt_volume through the existing edits.  Every step is also applied to a Model - the scene file's
dictionary and the grids in numpy, from the scene as loaded, never read back from the scene under test - which write_edited_scene
writes out as a scene file with its .sdf files for a fresh load and for the reference.

06_gridsdf_synth, 07_sdfunction_synth: see tests/volume_edits.py.  10_volgrid_synth/volgrid.json: one 32^3 volume, one instance with
material 0 (the medium), no SDF."""
import json
import os

import numpy as np

import scene_edits as E
import sculpt_cases as S
import volume_edits as V

F = np.float32
GRID, SDFS = V.GRID, V.SDFS
CLOUD = "10_volgrid_synth/volgrid.json"
SCENES = V.SCENES
IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1]
LAMP_MATERIAL = V.LAMP_MATERIAL


def frame_at(x, y, z):
    return np.array(IDENTITY + [x, y, z], F)


def smooth(whd, seed, res):
    """a (d, h, w) distance-like field (volume_edits.grid_resized)"""
    return V.grid_resized(None, None, whd, seed, F(res))[0]


# ---- ops of a "set" step ---------------------------------------------------------------------------------------------------------------
def rm_inst(*ids): return ("rm_inst", ids)
def rm_sdf(*ids): return ("rm_sdf", ids)
def rm_vol(*ids): return ("rm_vol", ids)
def vol_host(whd, seed, res=0.02): return ("vol_host", tuple(whd), seed, float(F(res)))
def vol_fill(whd, value, res=0.01): return ("vol_fill", tuple(whd), value, float(F(res)))
def vol_copy(source): return ("vol_copy", source)
def vol_bake(): return ("vol_bake",)
def inst(frame, volume, material, scalef=1.0): return ("inst", np.asarray(frame, F), volume, material, float(F(scalef)))
def inst_fit(volume, material): return ("inst_fit", volume, material)   # at the frame of the 17 x 9 x 5 fit around the icosphere


def sdf_box(whd, material, at):
    entry = {"type": "box", "whd": [float(F(v)) for v in whd], "material": material, "frame": [float(v) for v in frame_at(*at)]}
    return ("sdf", entry, dict(type="box", whd=whd, material=material, frame=frame_at(*at)))


def sdf_sphere(radius, material, at):
    entry = {"type": "sphere", "radius": float(F(radius)), "material": material, "frame": [float(v) for v in frame_at(*at)]}
    return ("sdf", entry, dict(type="sphere", p=(radius,), material=material, frame=frame_at(*at)))


def note(vpt, h, ops):
    """the ops of one set step through the setters of HostScene h"""
    for op in ops:
        kind = op[0]
        if kind == "rm_inst": h.remove_volume_instances(op[1])
        elif kind == "rm_sdf": h.remove_sdfs(op[1])
        elif kind == "rm_vol": h.remove_volumes(op[1])
        elif kind == "vol_host": h.add_volume(smooth(op[1], op[2], op[3]), res=op[3])
        elif kind == "vol_fill": h.add_volume(fill=op[2], whd=op[1], res=op[3])
        elif kind == "vol_copy": h.add_volume(copy_of=op[1])
        elif kind == "vol_bake":
            verts, tris = V.sphere_mesh()
            res, origin, step, _ = V.small_fit(vpt)
            h.add_volume(bake=(verts, tris, origin, step), whd=V.SMALL, res=res)
        elif kind == "inst": h.add_volume_instance(op[1], op[2], op[3], op[4])
        elif kind == "inst_fit": h.add_volume_instance(V.small_fit(vpt)[3].reshape(12), op[1], op[2], 1.0)
        elif kind == "sdf": h.add_sdf(**op[2])
        else: raise ValueError(kind)


class Model:
    """the numpy side: the scene file's dictionary and (grid, res) per volume"""

    def __init__(self, vpt, scene_file, original=None):
        original = original or vpt.HostScene(os.path.join(SCENES, scene_file))
        self.vpt, self.scene_file = vpt, scene_file
        self.d = json.load(open(os.path.join(SCENES, scene_file)))
        self.d.setdefault("sdfunctions", [])
        self.grids = [original.volume(k) for k in range(original.count_implicit("volumes"))]

    def set_step(self, ops):
        vpt, d = self.vpt, self.d
        gone = {k: set(i for op in ops if op[0] == k for i in op[1]) for k in ("rm_inst", "rm_sdf", "rm_vol")}
        old_grids = list(self.grids)
        new_id, kept = {}, []
        for k, g in enumerate(self.grids):
            if k not in gone["rm_vol"]:
                new_id[k] = len(kept)
                kept.append(g)
        d["vol_instances"] = [dict(e, volume=new_id[e["volume"]]) for i, e in enumerate(d["vol_instances"]) if i not in gone["rm_inst"]]
        d["sdfunctions"] = [e for i, e in enumerate(d["sdfunctions"]) if i not in gone["rm_sdf"]]
        d["volumes"] = [e for i, e in enumerate(d["volumes"]) if i not in gone["rm_vol"]]
        self.grids = kept
        for op in ops:
            kind = op[0]
            if kind == "vol_host": self.grids.append((smooth(op[1], op[2], op[3]), op[3]))
            elif kind == "vol_fill": self.grids.append((np.full(op[1][::-1], op[2], F), op[3]))
            elif kind == "vol_copy": self.grids.append((old_grids[op[1]][0].copy(), old_grids[op[1]][1]))
            elif kind == "vol_bake":
                verts, tris = V.sphere_mesh()
                res, origin, step, _ = V.small_fit(vpt)
                self.grids.append((vpt.bake_sdf_grid(verts, tris, V.SMALL, origin, step, device=None)[0], res))
            elif kind == "inst": d["vol_instances"].append({"volume": op[2], "material": op[3], "scale": op[4], "frame": [float(v) for v in op[1]]})
            elif kind == "inst_fit":
                d["vol_instances"].append({"volume": op[1], "material": op[2], "scale": 1.0, "frame": [float(v) for v in V.small_fit(vpt)[3].reshape(12)]})
            elif kind == "sdf": d["sdfunctions"].append(dict(op[1]))
            if kind.startswith("vol_"):
                d["volumes"].append({"name": f"added{len(d['volumes'])}"})

    def write(self, out):
        """the scene file under directory `out` (a pathlib.Path), every volume as a binary .sdf beside it; returns its path"""
        def change(d):
            d.clear()
            d.update(json.loads(json.dumps(self.d)))
            target = out / os.path.basename(os.path.dirname(self.scene_file))
            target.mkdir(exist_ok=True)
            for k, (grid, res) in enumerate(self.grids):
                self.vpt.save_volume(str(target / f"set_{k}.sdf"), grid, float(res))
                d["volumes"][k].update(uri=f"set_{k}.sdf", binary=True)
            if not d["sdfunctions"]:
                del d["sdfunctions"]
        return E.write_scene_variant(out, os.path.join(SCENES, self.scene_file), change)


def sculpt_case(vpt, volume):
    """one union stamp of a sphere into the 9^3 filled volume: (volume, stamps, region, origin, step) of tests/sculpt_cases.py"""
    return (volume, [vpt.Stamp(S.brush(vpt, "sphere", centre=(0.05, 0.04, 0.05), scale=1.0), S.UNION, 0.0)], None, None, None)


# ---- the named edits --------------------------------------------------------------------------------------------------------------------
def cases(vpt):
    """name -> (scene file, [step, ...])"""
    out = {}
    for tag, scene in (("grid", GRID), ("sdfs", SDFS)):
        sack = (0, 1) if scene == GRID else (0,)          # the instances of volume 0
        every = (0, 1, 2, 3) if scene == GRID else (0, 1)
        bunny_last = (2, 3) if scene == GRID else (1,)
        nsdf = 2 if scene == GRID else 10
        out.update({
            f"remove_first_{tag}": (scene, [("set", [rm_vol(0), rm_inst(*sack)])]),
            f"remove_last_{tag}": (scene, [("set", [rm_inst(*bunny_last), rm_vol(1)])]),
            # 30 voxels: everything behind them is misaligned against its source
            f"add_host_{tag}": (scene, [("set", [vol_host((5, 3, 2), 1), inst(frame_at(0.0, -0.1, 0.1), 2, 4), vol_host((7, 6, 5), 2), inst(frame_at(0.1, -0.1, 0.1), 3, 3)])]),
            f"add_tiny_{tag}": (scene, [("set", [vol_fill((1, 1, 1), 0.25), vol_fill((4, 0, 3), 1.0), inst(frame_at(0.0, -0.1, 0.0), 2, 4)])]),
            f"fill_sculpt_{tag}": (scene, [("set", [vol_fill((9, 9, 9), 1.0), inst(frame_at(0.0, -0.12, 0.1), 2, 4)]), ("sculpt", 2)]),
            f"copy_swap_{tag}": (scene, [("set", [vol_copy(0), rm_vol(0), rm_inst(*sack), inst(frame_at(-0.1, 0.0, 0.1), 1, 3, 0.001)])]),
            f"bake_new_{tag}": (scene, [("set", [vol_bake(), inst_fit(2, 4)])]),
            f"empty_then_one_{tag}": (scene, [("set", [rm_inst(*every), rm_vol(0, 1), rm_sdf(*range(nsdf))]),
                                              ("set", [vol_host((6, 5, 4), 3), inst(frame_at(0.0, 0.0, 0.0), 0, 3), sdf_box((2, 1e-5, 2), 0, (1, 0, 1))])]),
            f"light_added_{tag}": (scene, [("set", [sdf_box((0.3, 0.2, 1e-5), 2, (-0.2, -0.3, -1.0))])]),
            f"light_shifts_{tag}": (scene, [("set", [rm_sdf(0)])]),
            f"light_removed_{tag}": (scene, [("set", [rm_sdf(1), sdf_sphere(0.04, 3, (0.3, -0.05, 0.2))])]),
            f"regrow_then_set_{tag}": (scene, [("regrow", 0, (21, 30, 11), 3), ("set", [vol_fill((3, 3, 3), 0.5), inst(frame_at(0.0, -0.1, 0.0), 2, 4)])]),
        })
    out.update({
        "add_host_cloud": (CLOUD, [("set", [vol_host((5, 3, 2), 1, 0.05), inst(frame_at(-0.3, 0.0, 0.0), 1, 0), vol_host((7, 6, 5), 2, 0.05), inst(frame_at(0.3, 0.0, 0.0), 2, 0)])]),
        "copy_swap_cloud": (CLOUD, [("set", [vol_copy(0), rm_vol(0), rm_inst(0), inst(frame_at(-0.2, 0.0, 0.1), 0, 0)])]),
        "second_cloud": (CLOUD, [("set", [vol_copy(0), inst(frame_at(-0.6, 0.1, 0.0), 1, 0)])]),
        "empty_then_one_cloud": (CLOUD, [("set", [rm_inst(0), rm_vol(0)]), ("set", [vol_fill((6, 5, 4), 0.75, 0.1), inst(frame_at(0.0, 0.0, 0.0), 0, 0), sdf_sphere(0.1, 0, (0, 0, 0))])]),
    })
    return out


TAGS = ("grid", "sdfs")
PER_SCENE = ["remove_first", "remove_last", "add_host", "add_tiny", "fill_sculpt", "copy_swap", "bake_new", "empty_then_one", "light_added", "light_shifts",
             "light_removed", "regrow_then_set"]
CLOUD_NAMES = ["add_host_cloud", "copy_swap_cloud", "second_cloud", "empty_then_one_cloud"]
NAMES = [f"{n}_{t}" for n in PER_SCENE for t in TAGS] + CLOUD_NAMES
# a volume with a zero dimension has no file: the loader refuses an empty grid, as the reference's load_volume does
AS_SCENE_FILE = [n for n in NAMES if not n.startswith("add_tiny_")]
MOVES_POOL = [n for n in NAMES if not n.startswith("light_")]


def scene_of(vpt, name):
    return cases(vpt)[name][0]


def apply(vpt, name, h, after_step=None, original=None, model=None):
    """every step of a case on HostScene h (and on `model`); after_step(kind, edit) sees each edit as it is handed out"""
    scene_file, steps = cases(vpt)[name]
    for step in steps:
        if step[0] == "set":
            note(vpt, h, step[1])
            kind, edit = "set", h.update_volume_set()
            if model: model.set_step(step[1])
        elif step[0] == "regrow":
            _, volume, whd, seed = step
            res = (model.grids[volume][1] if model else h.volume(volume)[1])
            grid = smooth(whd, seed, res)
            h.set_volume(volume, grid, res)
            kind, edit = "volumes", h.update_volumes()
            if model: model.grids[volume] = (grid, res)
        elif step[0] == "sculpt":
            case = sculpt_case(vpt, step[1])
            S.apply(h, case)
            kind, edit = "sculpt", h.update_sculpts()
            if model:
                grid, res = model.grids[step[1]]
                model.grids[step[1]] = (S.replay(vpt, grid, res, case), res)
        else:
            raise ValueError(step[0])
        if after_step:
            after_step(kind, edit)


def write_edited_scene(vpt, name, out, original=None):
    """the scene file of a case under directory `out`, from the numpy side of the case alone; returns its path"""
    scene_file, steps = cases(vpt)[name]
    model = Model(vpt, scene_file, original)
    for step in steps:
        if step[0] == "set":
            model.set_step(step[1])
        elif step[0] == "regrow":
            res = model.grids[step[1]][1]
            model.grids[step[1]] = (smooth(step[2], step[3], res), res)
        elif step[0] == "sculpt":
            grid, res = model.grids[step[1]]
            model.grids[step[1]] = (S.replay(vpt, grid, res, sculpt_case(vpt, step[1])), res)
    return model.write(out)


# Cases the reference also renders (tests/golden/make_volume_set_fixtures.py -> volume_set_states.npz): name -> (shader, resolution, samples)
STATE_CASES = {"remove_first_grid": ("implicit", 96, 2), "add_host_grid": ("implicit_normal", 96, 2), "copy_swap_sdfs": ("implicit", 96, 2),
               "bake_new_grid": ("implicit_normal", 96, 2), "light_shifts_sdfs": ("implicit", 96, 3), "light_added_grid": ("implicit", 96, 2)}
