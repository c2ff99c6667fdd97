"""Scene edits shared by the scene-update tests (tests/test_scene_update_host.py, tests/test_scene_update_gpu.py): each takes a
HostScene and changes it through its setters.  Every formula is evaluated in float32, step by step, so that a replay elsewhere
(C++, another script) gives the same vertex bits."""
import json
import os

import numpy as np

F = np.float32


def write_scene_variant(tmp_path, scene_path, change, name="edited.json"):
    """a copy of the scene file at `scene_path` with change(its dictionary) applied, in a folder of `tmp_path` that links to the
    original's assets (and to the sibling scenes: scenes share assets through ../<scene>/).  Returns the new file's path."""
    src = os.path.dirname(scene_path)
    d = json.load(open(scene_path))
    change(d)
    out = tmp_path / os.path.basename(src)
    out.mkdir(exist_ok=True)
    for entry in os.listdir(src):
        if not entry.endswith(".json") and not (out / entry).exists():
            os.symlink(os.path.join(src, entry), out / entry)
    for sibling in os.listdir(os.path.dirname(src)):
        if not (tmp_path / sibling).exists():
            os.symlink(os.path.join(os.path.dirname(src), sibling), tmp_path / sibling)
    (out / name).write_text(json.dumps(d))
    return str(out / name)


def translate(h, instance, dx=0.0, dy=0.0, dz=0.0):
    """frame.o += (dx, dy, dz), each a float32 addition"""
    f = h.instance_frame(instance)
    f[9], f[10], f[11] = f[9] + F(dx), f[10] + F(dy), f[11] + F(dz)
    h.set_instance_frame(instance, f)


def rotation_y(angle):
    """the 3x3 part of a frame turned by `angle` about y, columns x, y, z (float32 of the double sine and cosine)"""
    c, s = F(np.cos(angle)), F(np.sin(angle))
    return np.array([c, 0, -s, 0, 1, 0, s, 0, c], F)


def rotate_frame(frame, angle):
    """frame with its axes replaced by rotation * axes (float32 products summed left to right); the origin stays"""
    r = rotation_y(angle).reshape(3, 3)   # rows: columns x, y, z of the rotation
    out = np.array(frame, F).copy()
    for col in range(3):
        v = out[3 * col:3 * col + 3].copy()
        out[3 * col:3 * col + 3] = [F(F(F(r[0][k] * v[0]) + F(r[1][k] * v[1])) + F(r[2][k] * v[2])) for k in range(3)]
    return out


def rotate_instance(h, instance, angle):
    h.set_instance_frame(instance, rotate_frame(h.instance_frame(instance), angle))


def rotate_environment(h, environment, angle):
    h.set_environment_frame(environment, rotate_frame(h.environment_frame(environment), angle))


def nudge(p):
    """p.y += 1e-3f * (p.x * 37 - floorf(p.x * 37)) on an (n, 3) float32 array"""
    p = np.array(p, F).copy()
    t = (p[:, 0] * F(37)).astype(F)
    p[:, 1] = (p[:, 1] + (F(1e-3) * (t - np.floor(t)).astype(F)).astype(F)).astype(F)
    return p


def times2(p):
    """every coordinate times 2 (exact in float32)"""
    return (np.array(p, F) * F(2)).astype(F)


def emissive(m):
    return any(float(c) != 0.0 for c in m.emission)


def lit_shapes(h):
    """shapes used by an instance with an emissive material (a superset of the shapes of mesh lights)"""
    out = set()
    for i in range(h.count("instances")):
        shape, material = h.instance_ids(i)
        if emissive(h.material(material)):
            out.add(shape)
    return out


def light_instances(h):
    """instances with an emissive material"""
    return [i for i in range(h.count("instances")) if emissive(h.material(h.instance_ids(i)[1]))]


def move_vertices(h, formula, with_normals=False):
    """formula over the positions of every shape that is not a light's; with_normals: the normals are sent along unchanged
    where the shape has them.  Returns the shapes edited."""
    skip, done = lit_shapes(h), []
    for s in range(h.count("shapes")):
        p = h.shape_positions(s)
        if s in skip or len(p) == 0:
            continue
        n = h.shape_normals(s)
        h.set_shape_positions(s, formula(p), n.copy() if with_normals and len(n) else None)
        done.append(s)
    return done


def flip_normals(h):
    """positions nudged and normals negated on every shape with normals that is not a light's: shading changes with them"""
    skip, done = lit_shapes(h), []
    for s in range(h.count("shapes")):
        p, n = h.shape_positions(s), h.shape_normals(s)
        if s in skip or len(p) == 0 or len(n) == 0:
            continue
        h.set_shape_positions(s, nudge(p), (-n).astype(F))
        done.append(s)
    return done


def edit_camera(h, camera=0):
    """frame moved and turned, lens, aperture and focus changed, orthographic toggled"""
    c = h.camera(camera)
    f = rotate_frame(np.array(list(c.frame.x) + list(c.frame.y) + list(c.frame.z) + list(c.frame.o), F), 0.1)
    f[9] = f[9] + F(0.05)
    for name, k in (("x", 0), ("y", 3), ("z", 6), ("o", 9)):
        for j in range(3):
            getattr(c.frame, name)[j] = float(f[k + j])
    c.lens = float(F(c.lens) * F(1.25))
    c.aperture = float(F(0.01))
    c.focus = float(F(1.5))
    h.set_camera(camera, c)


def toggle_orthographic(h, camera=0):
    c = h.camera(camera)
    c.orthographic = 0 if c.orthographic else 1
    h.set_camera(camera, c)


def edit_material(h, material):
    """colour, roughness, and matte -> glossy (any other type stays)"""
    m = h.material(material)
    m.color[0], m.color[1], m.color[2] = 0.8, 0.3, 0.2
    m.roughness = 0.15
    if m.type == 0:
        m.type = 1
    h.set_material(material, m)


def first_plain_material(h):
    """the first non-emissive matte material bound to an instance"""
    for i in range(h.count("instances")):
        m = h.instance_ids(i)[1]
        if not emissive(h.material(m)) and h.material(m).type == 0:
            return m
    raise AssertionError("no matte material")


def move_all_vertices(h, formula):
    """formula over the positions of EVERY shape (host side only: the device refuses the shapes of lights)"""
    for s in range(h.count("shapes")):
        if len(h.shape_positions(s)):
            h.set_shape_positions(s, formula(h.shape_positions(s)))


# Edits after which a fresh make_bvh of the edited scene has the ORIGINAL's topology, so the reference's own build of the edited scene
# pins the refitted boxes (tests/golden/make_update_fixtures.py checks that and writes tests/golden/update_stats.json):
# name -> (scene file under tests/golden/scenes, edit(host scene)).  (All positions times 2 keeps every SHAPE's topology but not the
# scene BVH's on 03_volume and curves.json: the script refuses those; 05_head1ss_sub keeps both.)
PINNED = {
    "vol_inst1_x001": ("03_volume/volume.json", lambda h: translate(h, 1, dx=0.01)),
    "vol_inst1_x02": ("03_volume/volume.json", lambda h: translate(h, 1, dx=0.2)),
    "curves_last_y005": ("09_curves_synth/curves.json", lambda h: translate(h, h.count("instances") - 1, dy=0.05)),
    "curves_last_y03": ("09_curves_synth/curves.json", lambda h: translate(h, h.count("instances") - 1, dy=0.3)),
    "curves_inst1_x001": ("09_curves_synth/curves.json", lambda h: translate(h, 1, dx=0.01)),
    "curves_inst1_x02": ("09_curves_synth/curves.json", lambda h: translate(h, 1, dx=0.2)),
    "curves_nudge": ("09_curves_synth/curves.json", lambda h: move_all_vertices(h, nudge)),
    "head_times2": ("05_head1ss_sub/head1ss_sub.json", lambda h: move_all_vertices(h, times2)),
    "surf_times2": ("01_surface_min/surface_min.json", lambda h: move_all_vertices(h, times2)),
}

# Pinned cases the reference also renders: name -> (shader, resolution, samples, bounces), the non-volumetric path tracer at the sizes
# of tests/cases.py (path_64_4, and 96 for the substitute scenes).  Only edits the DEVICE takes too (curves_nudge moves the vertices
# of a light's shape, which vpt_scene_update refuses) and whose scene file the reference loads bit for bit (surf_times2 goes through
# re-written texcoords).  tests/golden/make_update_fixtures.py measures, on the reference's arithmetic, the share of pixels that are
# stable under 1-ulp nudges of libm and records it in update_stats.json; a case under 0.8 is recorded as "state_refused" and has no
# state (curves.json: both shaders tried stay far under it).
STATE_CANDIDATES = {
    "vol_inst1_x001": ("pathtrace", 64, 4, 4), "vol_inst1_x02": ("pathtrace", 64, 4, 4),
    "head_times2": ("pathtrace", 96, 4, 4),
    "curves_last_y005": ("pathtrace", 96, 4, 8), "curves_inst1_x02": ("eyelight", 96, 4, 8),
}
STATE_CASES = {k: v for k, v in STATE_CANDIDATES.items() if not k.startswith("curves")}   # those whose share reached 0.8
