"""Which change of a HostScene may begin while which other is pending.  A HostScene keeps up to five pending edits - the SceneEdit of
the setters, the InstanceEdit, the ShapeEdit, the TextureEdit and the VolumeEdit - and refuses a call whose ids would name another list
than the pending edit's: the message names the update_*() to call first, and a refused call changes nothing.  The matrix below is what
the package has always done, every cell of it; the scene is 03_volume under a plain sky with the binary grid of 06_gridsdf_synth and one shape no instance
names, so that every call has something to work on."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

F = np.float32
S03 = os.path.join(GOLDEN, "scenes", "03_volume")
GRID = os.path.join(GOLDEN, "scenes", "06_gridsdf_synth")
TRIANGLE = dict(positions=np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), triangles=[[0, 1, 2]])
FRAME = np.array([0.5, 0, 0, 0, 0.5, 0, 0, 0, 0.5, 0.25, 0.125, -0.5], F)
FLOOR, SPARE = 0, 4   # shapes: the floor's four vertices; the shape no instance names


@pytest.fixture(scope="module")
def scene_file(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pending"))
    d, grid = json.load(open(os.path.join(S03, "volume.json"))), json.load(open(os.path.join(GRID, "gridsdf_synth.json")))
    d["shapes"].append({"name": "spare", "uri": "shapes/floor.ply"})
    del d["textures"][1], d["environments"][0]["emission_tex"]   # a plain sky: no CDF over two million texels at every hand-out
    d["volumes"], d["vol_instances"] = grid["volumes"][:1], [v for v in grid["vol_instances"] if v["volume"] == 0]   # the binary grid
    for key, src in (("shapes", S03), ("textures", S03), ("volumes", GRID)):
        for item in d[key]:
            item["uri"] = os.path.relpath(os.path.join(src, item["uri"]), out)
    path = os.path.join(out, "pending.json")
    json.dump(d, open(path, "w"))
    return path


# ---- the sixteen calls that begin or hand out a change ---------------------------------------------------------------------------------
BEGINNERS = {
    "set_instance_frame": lambda h: h.set_instance_frame(1, FRAME),
    "set_shape_positions": lambda h: h.set_shape_positions(FLOOR, h.shape_positions(FLOOR) * F(2)),
    "rebuild_bvh": lambda h: h.rebuild_bvh((FLOOR,), True),
    "add_instance": lambda h: h.add_instance(FRAME, FLOOR, 0),
    "remove_instances": lambda h: h.remove_instances([h.count("instances") - 1]),
    "set_instance": lambda h: h.set_instance(2, material=1),
    "update_instances": lambda h: h.update_instances(),
    "add_shape": lambda h: h.add_shape(**TRIANGLE),
    "set_shape": lambda h: h.set_shape(FLOOR, **TRIANGLE),
    "remove_shapes": lambda h: h.remove_shapes([SPARE]),
    "update_shapes": lambda h: h.update_shapes(),
    "set_camera": lambda h: h.set_camera(0, h.camera(0)),
    "set_material": lambda h: h.set_material(0, h.material(0)),
    "set_environment_frame": lambda h: h.set_environment_frame(0, FRAME),
    "set_texture": lambda h: h.set_texture(0, np.array([[[1, 2, 3, 4], [5, 6, 7, 8]]], np.uint8)),
    "set_volume_instance": lambda h: h.set_volume_instance(0, scalef=0.002),
}
# what is pending, made so in its smallest way: the SceneEdit holding an instance frame, shape vertices, or only a camera, a material or
# an environment frame; the InstanceEdit; the ShapeEdit; the TextureEdit; the VolumeEdit; nothing
LEDGERS = {
    "frame": BEGINNERS["set_instance_frame"], "vertices": BEGINNERS["set_shape_positions"], "camera": BEGINNERS["set_camera"],
    "material": BEGINNERS["set_material"], "envframe": BEGINNERS["set_environment_frame"], "instances": BEGINNERS["add_instance"],
    "shapes": BEGINNERS["add_shape"], "textures": BEGINNERS["set_texture"], "volumes": BEGINNERS["set_volume_instance"], "nothing": lambda h: None,
}
# row: the call; column: what is pending.  '.': the call goes through; B, I, S: VptError, naming update_bvh(), update_instances(),
# update_shapes() as the call to make first.
MATRIX = """
                        frame vertices camera material envframe instances shapes textures volumes nothing
set_instance_frame        .      .       .       .        .         I       S       .        .       .
set_shape_positions       .      .       .       .        .         I       S       .        .       .
rebuild_bvh               B      B       B       B        B         I       S       .        .       .
add_instance              B      B       .       .        .         .       S       .        .       .
remove_instances          B      B       .       .        .         .       S       .        .       .
set_instance              B      B       .       .        .         .       S       .        .       .
update_instances          B      B       .       .        .         .       S       .        .       .
add_shape                 B      B       .       .        .         I       .       .        .       .
set_shape                 B      B       .       .        .         I       .       .        .       .
remove_shapes             B      B       .       .        .         I       .       .        .       .
update_shapes             B      B       .       .        .         I       .       .        .       .
set_camera                .      .       .       .        .         .       .       .        .       .
set_material              .      .       .       .        .         .       .       .        .       .
set_environment_frame     .      .       .       .        .         .       .       .        .       .
set_texture               .      .       .       .        .         .       .       .        .       .
set_volume_instance       .      .       .       .        .         .       .       .        .       .
"""
NAMED = {"B": "update_bvh()", "I": "update_instances()", "S": "update_shapes()"}


def matrix():
    rows = [line.split() for line in MATRIX.strip().splitlines()]
    return {(row[0], ledger): cell for row in rows[1:] for ledger, cell in zip(rows[0], row[1:])}


def test_the_matrix_names_every_call_and_every_ledger():
    cells = matrix()
    assert set(cells) == {(b, l) for b in BEGINNERS for l in LEDGERS} and set(cells.values()) == set(".BIS")


def handed_out(vpt, h):
    """every pending edit handed out - the SceneEdit first, whose ids name the lists as they are, then whichever of the two lists has
    changes pending - as the ids and counts it holds"""
    e = h.update_bvh()
    try:
        i = h.update_instances()
        s = h.update_shapes()
    except vpt.VptError:
        s = h.update_shapes()
        i = h.update_instances()
    t, v = h.update_textures(), h.update_volumes()
    return {"cameras": sorted(e.cameras), "frames": sorted(e.instances), "envframes": sorted(e.environments), "materials": sorted(e.materials),
            "vertices": sorted(e.shapes), "instances": (i.remove, sorted(i.set), len(i.add)), "shapes": (s.remove, sorted(s.set), len(s.add)),
            "textures": (sorted(t.environments), sorted(t.textures)), "volumes": (sorted(v.vol_instances), sorted(v.sdfs), sorted(v.volumes))}


@pytest.mark.parametrize("ledger", list(LEDGERS))
def test_a_refused_call_names_the_update_to_make_first_and_changes_nothing(vpt, scene_file, ledger):
    cells = matrix()
    h, twin = vpt.HostScene(scene_file), vpt.HostScene(scene_file)
    LEDGERS[ledger](h), LEDGERS[ledger](twin)
    stats = h.stats()
    for name, call in BEGINNERS.items():
        if cells[name, ledger] == ".":
            continue
        with pytest.raises(vpt.VptError) as err:
            call(h)
        assert str(err.value).startswith(name + ": ") and NAMED[cells[name, ledger]] + " first" in str(err.value), f"{name} while {ledger}: {err.value}"
    assert h.stats() == stats, f"while {ledger}: a refused call changed the scene"
    assert handed_out(vpt, h) == handed_out(vpt, twin), f"while {ledger}: a refused call changed a pending edit"


# the calls in an order in which each can go through once those before it have: rebuild_bvh while nothing at all is pending, the setters
# that nothing blocks, the instance list and its hand-out, the shape list and its hand-out, then the setters of the SceneEdit's ids
ORDER = ["rebuild_bvh", "set_camera", "set_material", "set_environment_frame", "set_texture", "set_volume_instance", "add_instance",
         "remove_instances", "set_instance", "update_instances", "add_shape", "set_shape", "remove_shapes", "update_shapes",
         "set_instance_frame", "set_shape_positions"]
# what handed_out() gives after every call the matrix lets through has been made, in ORDER, on top of the ledger
C0, M0, E0, T0, V0 = ("cameras", [0]), ("materials", [0]), ("envframes", [0]), ("textures", ([], [0])), ("volumes", ([0], [], []))
ALWAYS = dict([C0, M0, E0, T0, V0])
QUIET = dict(frames=[], vertices=[], instances=((), [], 0), shapes=((), [], 0))
AFTER = {
    "frame": dict(QUIET, **ALWAYS, frames=[1], vertices=[FLOOR]),
    "vertices": dict(QUIET, **ALWAYS, frames=[1], vertices=[FLOOR]),
    "camera": dict(QUIET, **ALWAYS, frames=[1], vertices=[FLOOR]),
    "material": dict(QUIET, **ALWAYS, frames=[1], vertices=[FLOOR]),
    "envframe": dict(QUIET, **ALWAYS, frames=[1], vertices=[FLOOR]),
    "instances": dict(QUIET, **ALWAYS),
    "shapes": dict(QUIET, **ALWAYS),
    "textures": dict(QUIET, **ALWAYS, frames=[1], vertices=[FLOOR]),
    "volumes": dict(QUIET, **ALWAYS, frames=[1], vertices=[FLOOR]),
    "nothing": dict(QUIET, **ALWAYS, frames=[1], vertices=[FLOOR]),
}


@pytest.mark.parametrize("ledger", list(LEDGERS))
def test_every_call_the_matrix_lets_through_goes_through(vpt, scene_file, ledger):
    cells = matrix()
    assert sorted(ORDER) == sorted(BEGINNERS)
    h = vpt.HostScene(scene_file)
    LEDGERS[ledger](h)
    counts = (h.count("instances"), h.count("shapes"))
    results = {name: BEGINNERS[name](h) for name in ORDER if cells[name, ledger] == "."}
    if "update_instances" in results:   # one added (two where the ledger is that), one removed, one set
        edit = results["update_instances"]
        assert isinstance(edit, vpt.InstanceEdit) and (len(edit.remove), sorted(edit.set), len(edit.add)) == (1, [2], 2 if ledger == "instances" else 1)
        assert h.count("instances") == counts[0] + len(edit.add) - 1
    if "update_shapes" in results:
        edit = results["update_shapes"]
        assert isinstance(edit, vpt.ShapeEdit) and (edit.remove, sorted(edit.set), len(edit.add)) == ((SPARE,), [FLOOR], 2 if ledger == "shapes" else 1)
        assert h.count("shapes") == counts[1] + len(edit.add) - 1
    if "rebuild_bvh" in results:
        assert isinstance(results["rebuild_bvh"], vpt.BvhRebuild) and results["rebuild_bvh"].shapes == (FLOOR,)
    assert handed_out(vpt, h) == AFTER[ledger], f"while {ledger}"
