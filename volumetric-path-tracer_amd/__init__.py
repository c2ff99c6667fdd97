"""vpt-mi355x: ctypes bindings over the C-ABI of ``include/vpt.h`` (libvpt_hip.so, the HIP
path) and over the host library (libvpt_host.so: scene.json loader, BVH / light / state builders
that mirror ``libs/yocto_pathtrace/yocto_pathtrace.h:119-139`` of the reference).

Nothing in this package computes radiance on the CPU and nothing here touches ``oracle/``: if
the HIP library is missing or no GPU is present, rendering raises ``VptError``.

The directory name contains a dash, so import it with ``vpt_loader.load()`` (repo root) or
``importlib``; inside, everything is ordinary Python.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional
from dataclasses import dataclass, field

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

SHADER_NAMES = ["volpathtrace", "pathtrace", "naive", "eyelight", "normal", "texcoord", "color",
                "implicit", "implicit_normal"]  # yocto_pathtrace.h:101-103


class VptError(RuntimeError):
    pass


def _lib(name: str) -> C.CDLL:
    path = os.path.join(_HERE, name)
    if not os.path.exists(path):
        raise VptError(f"{path} is not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


hip = _lib("libvpt_hip.so")    # must load first: libvpt_host.so links against it
host = _lib("libvpt_host.so")


class VptParams(C.Structure):  # vpt_params
    _fields_ = [("camera", C.c_int32), ("resolution", C.c_int32), ("shader", C.c_int32),
                ("samples", C.c_int32), ("bounces", C.c_int32), ("noparallel", C.c_int32),
                ("noimplicit_mis", C.c_int32), ("spheretrace_maxiter", C.c_int32)]


class VptLayout(C.Structure):  # vpt_layout
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("tile_w", C.c_int32),
                ("tile_h", C.c_int32), ("rank", C.c_int32), ("nranks", C.c_int32)]


class VptAdaptive(C.Structure):  # vpt_adaptive
    _fields_ = [("threshold", C.c_float), ("min_samples", C.c_int32), ("step", C.c_int32)]


class VptDenoise(C.Structure):  # vpt_denoise_params
    _fields_ = [("iterations", C.c_int32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_albedo", C.c_float)]


class VptDisplay(C.Structure):  # vpt_display_params
    _fields_ = [("exposure", C.c_float), ("filmic", C.c_int32), ("srgb", C.c_int32)]


class VptSessionParams(C.Structure):  # vpt_session_params
    _fields_ = [("render", VptParams), ("pratio", C.c_int32), ("display", VptDisplay), ("denoise", C.c_int32), ("filter", VptDenoise),
                ("guide_samples", C.c_int32)]


AOV_PLANES = ("normal", "albedo", "texcoord", "depth", "ids", "uvt")


class VptAovPlanes(C.Structure):  # vpt_aov_planes: any of them None
    _fields_ = [(name, C.c_void_p) for name in AOV_PLANES]


class VptPick(C.Structure):  # vpt_pick
    _fields_ = [("hit", C.c_int32), ("instance", C.c_int32), ("element", C.c_int32), ("shape", C.c_int32), ("material", C.c_int32),
                ("u", C.c_float), ("v", C.c_float), ("distance", C.c_float)]


class VptFrame(C.Structure):  # vpt_frame: x, y, z, o
    _fields_ = [("x", C.c_float * 3), ("y", C.c_float * 3), ("z", C.c_float * 3), ("o", C.c_float * 3)]


class VptCamera(C.Structure):  # vpt_camera
    _fields_ = [("frame", VptFrame), ("orthographic", C.c_int32), ("lens", C.c_float), ("film", C.c_float), ("aspect", C.c_float),
                ("focus", C.c_float), ("aperture", C.c_float)]


class VptMaterial(C.Structure):  # vpt_material
    _fields_ = [("type", C.c_int32), ("emission", C.c_float * 3), ("color", C.c_float * 3), ("roughness", C.c_float),
                ("metallic", C.c_float), ("ior", C.c_float), ("scattering", C.c_float * 3), ("scanisotropy", C.c_float),
                ("trdepth", C.c_float), ("opacity", C.c_float), ("emission_tex", C.c_int32), ("color_tex", C.c_int32),
                ("roughness_tex", C.c_int32), ("scattering_tex", C.c_int32), ("normal_tex", C.c_int32)]


class VptSceneEdit(C.Structure):  # vpt_scene_edit
    _fields_ = [("num_cameras", C.c_int32), ("camera_ids", C.c_void_p), ("cameras", C.c_void_p),
                ("num_instances", C.c_int32), ("instance_ids", C.c_void_p), ("instance_frames", C.c_void_p),
                ("num_environments", C.c_int32), ("environment_ids", C.c_void_p), ("environment_frames", C.c_void_p),
                ("num_materials", C.c_int32), ("material_ids", C.c_void_p), ("materials", C.c_void_p),
                ("num_shapes", C.c_int32), ("shape_ids", C.c_void_p), ("shape_positions", C.c_void_p), ("shape_normals", C.c_void_p)]


class VptEnvironment(C.Structure):  # vpt_environment
    _fields_ = [("frame", VptFrame), ("emission", C.c_float * 3), ("emission_tex", C.c_int32)]


class VptTexture(C.Structure):  # vpt_texture
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("linear", C.c_int32), ("is_float", C.c_int32), ("offset", C.c_int64)]


class VptTextureEdit(C.Structure):  # vpt_texture_edit
    _fields_ = [("num_environments", C.c_int32), ("environment_ids", C.c_void_p), ("environments", C.c_void_p),
                ("num_textures", C.c_int32), ("texture_ids", C.c_void_p), ("textures", C.c_void_p),
                ("num_texels_f", C.c_int64), ("texels_f", C.c_void_p), ("num_texels_b", C.c_int64), ("texels_b", C.c_void_p)]


class VptVolume(C.Structure):  # vpt_volume
    _fields_ = [("whd", C.c_int32 * 3), ("res", C.c_float), ("offset", C.c_int64)]


class VptVolumeInstance(C.Structure):  # vpt_volume_instance
    _fields_ = [("frame", VptFrame), ("volume", C.c_int32), ("material", C.c_int32), ("scalef", C.c_float)]


class VptSdf(C.Structure):  # vpt_sdf
    _fields_ = [("frame", VptFrame), ("type", C.c_int32), ("material", C.c_int32), ("whd", C.c_float * 3), ("p", C.c_float * 4)]


class VptVolumeSource(C.Structure):  # vpt_volume_source
    _fields_ = [("whd", C.c_int32 * 3), ("res", C.c_float), ("region_lo", C.c_int32 * 3), ("region_whd", C.c_int32 * 3), ("mode", C.c_int32),
                ("offset", C.c_int64), ("bake", C.c_void_p)]


class VptVolumeEdit(C.Structure):  # vpt_volume_edit
    _fields_ = [("num_vol_instances", C.c_int32), ("vol_instance_ids", C.c_void_p), ("vol_instances", C.c_void_p),
                ("num_sdfs", C.c_int32), ("sdf_ids", C.c_void_p), ("sdfs", C.c_void_p),
                ("num_volumes", C.c_int32), ("volume_ids", C.c_void_p), ("volumes", C.c_void_p),
                ("num_voxels", C.c_int64), ("voxels", C.c_void_p)]


SDF_TYPES = ["bbox", "box", "capped_cone", "plane", "sphere", "torus"]
VOXELS_REPLACE, VOXELS_UNION = 0, 1
MATERIAL_TYPES = ["matte", "glossy", "reflective", "transparent", "refractive", "subsurface", "volumetric", "gltfpbr"]


class VptBakeDesc(C.Structure):  # vpt_bake_desc
    _fields_ = [("num_vertices", C.c_int32), ("positions", C.c_void_p), ("num_triangles", C.c_int32), ("triangles", C.c_void_p),
                ("whd", C.c_int32 * 3), ("origin", C.c_float * 3), ("step", C.c_float * 3)]


class VptBakeStats(C.Structure):  # vpt_bake_stats
    _fields_ = [("dropped_triangles", C.c_int32), ("bvh_nodes", C.c_int32), ("bvh_depth", C.c_int32), ("launches", C.c_int32),
                ("device_ms", C.c_float)]


class VptBvhRebuild(C.Structure):  # vpt_bvh_rebuild
    _fields_ = [("num_shapes", C.c_int32), ("shape_ids", C.POINTER(C.c_int32)), ("scene", C.c_int32)]


class BvhRebuild:
    """What vpt_scene_rebuild_bvh takes (include/vpt.h: vpt_bvh_rebuild): the shapes whose BVHs are built anew, and whether the scene
    BVH is (it is whenever a shape is named).  HostScene.rebuild_bvh makes one; DeviceScene.rebuild_bvh / MultiDeviceScene.rebuild_bvh /
    RenderSession.rebuild_bvh apply it.  quality: BVH_MIDDLE (0, the reference's highquality = false) or BVH_SAH (1, split_sah: the rule
    at vpt_build_bvh_quality in include/vpt.h), carried to the device with the request."""

    def __init__(self, shapes=(), scene: bool = True, *, quality: int = 0):
        self.shapes, self.scene, self.quality = tuple(int(i) for i in shapes), bool(scene), int(quality)

    def empty(self) -> bool:
        return not self.shapes and not self.scene

    def to_abi(self):
        """(VptBvhRebuild, the array it points into: keep it alive across the call)"""
        ids = (C.c_int32 * max(1, len(self.shapes)))(*self.shapes)
        return VptBvhRebuild(len(self.shapes), C.cast(ids, C.POINTER(C.c_int32)) if self.shapes else None, int(self.scene)), ids


class VptInstance(C.Structure):  # vpt_instance
    _fields_ = [("frame", VptFrame), ("shape", C.c_int32), ("material", C.c_int32)]


class VptInstanceEdit(C.Structure):  # vpt_instance_edit
    _fields_ = [("num_remove", C.c_int32), ("remove_ids", C.c_void_p), ("num_set", C.c_int32), ("set_ids", C.c_void_p), ("set", C.c_void_p),
                ("num_add", C.c_int32), ("add", C.c_void_p)]


INSTANCE = np.dtype([("frame", np.float32, 12), ("shape", np.int32), ("material", np.int32)])   # vpt_instance
assert INSTANCE.itemsize == C.sizeof(VptInstance) == 56


class InstanceEdit:
    """What vpt_scene_update_instances takes (include/vpt.h: vpt_instance_edit): `set`, a dictionary current id -> (frame (12,) float32,
    shape, material) that replaces those instances; `remove`, current ids erased after that (ids close up); `add`, a list of (frame,
    shape, material) appended after the survivors.  HostScene.update_instances makes one; DeviceScene.update_instances /
    MultiDeviceScene.update_instances / RenderSession.edit_instances apply it."""

    def __init__(self, remove=(), set=None, add=()):
        item = lambda v: (np.ascontiguousarray(v[0], np.float32).reshape(12).copy(), int(v[1]), int(v[2]))
        self.remove = tuple(int(i) for i in remove)
        self.set = {int(k): item(v) for k, v in dict(set or {}).items()}
        self.add = [item(v) for v in add]

    def empty(self) -> bool:
        return not (self.remove or self.set or self.add)

    @staticmethod
    def _records(items) -> np.ndarray:
        out = np.zeros(len(items), INSTANCE)
        for i, (frame, shape, material) in enumerate(items):
            out[i] = (frame, shape, material)
        return out

    def to_abi(self):
        """(VptInstanceEdit, the arrays it points into: keep them alive across the call)"""
        remove, set_ids = np.array(self.remove, np.int32), np.array(list(self.set.keys()), np.int32)
        set_rec, add_rec = self._records(list(self.set.values())), self._records(self.add)
        ptr = lambda a: a.ctypes.data if len(a) else None
        abi = VptInstanceEdit(len(remove), ptr(remove), len(set_ids), ptr(set_ids), ptr(set_rec), len(add_rec), ptr(add_rec))
        return abi, [remove, set_ids, set_rec, add_rec]


class VptShapeData(C.Structure):  # vpt_shape_data
    _fields_ = [("num_vertices", C.c_int32), ("positions", C.c_void_p), ("normals", C.c_void_p), ("texcoords", C.c_void_p), ("colors", C.c_void_p),
                ("radius", C.c_void_p), ("num_triangles", C.c_int32), ("triangles", C.c_void_p), ("num_quads", C.c_int32), ("quads", C.c_void_p),
                ("num_points", C.c_int32), ("points", C.c_void_p), ("num_lines", C.c_int32), ("lines", C.c_void_p)]


class VptShapeEdit(C.Structure):  # vpt_shape_edit
    _fields_ = [("num_remove", C.c_int32), ("remove_ids", C.c_void_p), ("num_set", C.c_int32), ("set_ids", C.c_void_p), ("set", C.c_void_p),
                ("num_add", C.c_int32), ("add", C.c_void_p)]


assert C.sizeof(VptShapeData) == 112 and C.sizeof(VptShapeEdit) == 56

MESH_FLOATS = {"positions": 3, "normals": 3, "texcoords": 2, "colors": 4, "radius": 0}     # floats per vertex (0: a plain array)
MESH_ELEMENTS = {"triangles": 3, "quads": 4, "points": 0, "lines": 2}                        # indices per element


def mesh(positions, triangles=None, quads=None, points=None, lines=None, normals=None, texcoords=None, colors=None, radius=None) -> dict:
    """one shape as vpt_shape_data takes it: a dictionary of contiguous float32 / int32 arrays, None (or empty) for what the shape has not"""
    given = dict(positions=positions, triangles=triangles, quads=quads, points=points, lines=lines, normals=normals, texcoords=texcoords, colors=colors, radius=radius)
    out = {}
    for key, width in MESH_FLOATS.items():
        a = given[key]
        out[key] = None if a is None or len(a) == 0 else np.ascontiguousarray(a, np.float32).reshape((-1, width) if width else (-1,)).copy()
    for key, width in MESH_ELEMENTS.items():
        a = given[key]
        out[key] = None if a is None or len(a) == 0 else np.ascontiguousarray(a, np.int32).reshape((-1, width) if width else (-1,)).copy()
    return out


class ShapeEdit:
    """What vpt_scene_update_shapes takes (include/vpt.h: vpt_shape_edit): `set`, a dictionary current id -> mesh (the dictionary mesh()
    makes) that replaces those shapes whole; `remove`, current ids erased after that (ids close up, the instances' shape ids follow; no
    instance may name a removed shape); `add`, a list of meshes appended after the survivors.  HostScene.update_shapes makes one;
    DeviceScene.update_shapes / MultiDeviceScene.update_shapes / RenderSession.edit_shapes apply it.
    Importing an object into a running scene is a ShapeEdit followed by an InstanceEdit: add_shape(...) returns the id the shape has after
    update_shapes(); once that edit is handed out, add_instance(frame, id, material) and update_instances() put it in place."""

    def __init__(self, remove=(), set=None, add=()):
        self.remove = tuple(int(i) for i in remove)
        self.set = {int(k): mesh(**v) for k, v in dict(set or {}).items()}
        self.add = [mesh(**v) for v in add]

    def empty(self) -> bool:
        return not (self.remove or self.set or self.add)

    @staticmethod
    def _records(meshes):
        out = (VptShapeData * max(len(meshes), 1))()
        ptr = lambda a: None if a is None else a.ctypes.data
        for rec, m in zip(out, meshes):
            rec.num_vertices = 0 if m["positions"] is None else len(m["positions"])
            for key in MESH_FLOATS:
                setattr(rec, key, ptr(m[key]))
            for key in MESH_ELEMENTS:
                setattr(rec, "num_" + key, 0 if m[key] is None else len(m[key]))
                setattr(rec, key, ptr(m[key]))
        return out

    def to_abi(self):
        """(VptShapeEdit, the arrays it points into: keep them alive across the call)"""
        remove, set_ids = np.array(self.remove, np.int32), np.array(list(self.set.keys()), np.int32)
        set_rec, add_rec = self._records(list(self.set.values())), self._records(self.add)
        ptr = lambda a: a.ctypes.data if len(a) else None
        abi = VptShapeEdit(len(remove), ptr(remove), len(set_ids), ptr(set_ids), C.addressof(set_rec) if self.set else None, len(self.add),
                           C.addressof(add_rec) if self.add else None)
        return abi, [remove, set_ids, set_rec, add_rec, self.set, self.add]


class SceneEdit:
    """What vpt_scene_update takes (include/vpt.h: vpt_scene_edit), as dictionaries id -> value: cameras (VptCamera), instances and
    environments ((12,) float32 frames x, y, z, o), materials (VptMaterial), shapes ((positions, normals or None) as (n, 3) float32).
    HostScene's setters fill one; DeviceScene.update / MultiDeviceScene.update apply it."""

    def __init__(self, cameras=None, instances=None, environments=None, materials=None, shapes=None):
        self.cameras, self.instances, self.environments = dict(cameras or {}), dict(instances or {}), dict(environments or {})
        self.materials, self.shapes = dict(materials or {}), dict(shapes or {})

    def empty(self) -> bool:
        return not (self.cameras or self.instances or self.environments or self.materials or self.shapes)

    def merge(self, other: "SceneEdit") -> "SceneEdit":
        """this edit followed by `other` (later values win)"""
        out = SceneEdit(self.cameras, self.instances, self.environments, self.materials, self.shapes)
        for name in ("cameras", "instances", "environments", "materials"):
            getattr(out, name).update(getattr(other, name))
        for k, (pos, nrm) in other.shapes.items():
            out.shapes[k] = (pos, nrm if nrm is not None or k not in out.shapes else out.shapes[k][1])
        return out

    def to_abi(self):
        """(VptSceneEdit, objects that keep its arrays alive)"""
        keep, abi = [], VptSceneEdit()

        def ids(d):
            a = np.array(list(d.keys()), np.int32)
            keep.append(a)
            return a.ctypes.data

        def structs(d, T):
            a = (T * max(1, len(d)))(*d.values())
            keep.append(a)
            return C.cast(a, C.c_void_p).value

        def frames(d):
            a = np.ascontiguousarray(np.array([np.asarray(f, np.float32).reshape(12) for f in d.values()], np.float32).reshape(-1, 12))
            keep.append(a)
            return a.ctypes.data

        abi.num_cameras, abi.camera_ids, abi.cameras = len(self.cameras), ids(self.cameras), structs(self.cameras, VptCamera)
        abi.num_instances, abi.instance_ids, abi.instance_frames = len(self.instances), ids(self.instances), frames(self.instances)
        abi.num_environments, abi.environment_ids, abi.environment_frames = len(self.environments), ids(self.environments), frames(self.environments)
        abi.num_materials, abi.material_ids, abi.materials = len(self.materials), ids(self.materials), structs(self.materials, VptMaterial)
        n = len(self.shapes)
        pos, nrm = (C.c_void_p * max(1, n))(), (C.c_void_p * max(1, n))()
        for i, (p, q) in enumerate(self.shapes.values()):
            p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
            keep.append(p)
            pos[i] = p.ctypes.data
            if q is not None:
                q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
                if q.shape != p.shape:
                    raise VptError("normals of a shape edit must match its positions")
                keep.append(q)
                nrm[i] = q.ctypes.data
        keep += [pos, nrm]
        abi.num_shapes, abi.shape_ids = n, ids(self.shapes)
        abi.shape_positions, abi.shape_normals = C.cast(pos, C.c_void_p).value, C.cast(nrm, C.c_void_p).value
        return abi, keep


class TextureEdit:
    """What vpt_scene_update_textures takes (include/vpt.h: vpt_texture_edit), as dictionaries id -> value: environments
    (VptEnvironment: frame, emission, emission_tex) and textures ((texels (h, w, 4) float32 or uint8, linear)).  HostScene's
    set_environment / set_texture fill one; DeviceScene.update_textures / MultiDeviceScene.update_textures apply it."""

    def __init__(self, environments=None, textures=None):
        self.environments, self.textures = dict(environments or {}), dict(textures or {})

    def empty(self) -> bool:
        return not (self.environments or self.textures)

    def payload_bytes(self) -> int:
        """bytes of the edit itself as vpt_scene_update_stats counts them: texels, 24 per texture entry, 112 per environment entry"""
        return sum(np.asarray(t).nbytes + 24 for t, _ in self.textures.values()) + 112 * len(self.environments)

    def to_abi(self):
        """(VptTextureEdit, objects that keep its arrays alive)"""
        keep, abi = [], VptTextureEdit()
        env_ids = np.array(list(self.environments.keys()), np.int32)
        envs = (VptEnvironment * max(1, len(self.environments)))(*self.environments.values())
        tex_ids = np.array(list(self.textures.keys()), np.int32)
        entries = (VptTexture * max(1, len(self.textures)))()
        pool = {True: [], False: []}
        count = {True: 0, False: 0}
        for k, (texels, linear) in enumerate(self.textures.values()):
            texels = np.ascontiguousarray(texels)
            if texels.ndim != 3 or texels.shape[2] != 4 or texels.dtype not in (np.float32, np.uint8):
                raise VptError("texels of a texture edit are (h, w, 4) float32 or uint8")
            is_float = texels.dtype == np.float32
            entries[k] = VptTexture(texels.shape[1], texels.shape[0], int(bool(linear)), int(is_float), count[is_float])
            pool[is_float].append(texels.reshape(-1, 4))
            count[is_float] += texels.shape[0] * texels.shape[1]
        texels_f = np.ascontiguousarray(np.concatenate(pool[True])) if pool[True] else np.zeros((0, 4), np.float32)
        texels_b = np.ascontiguousarray(np.concatenate(pool[False])) if pool[False] else np.zeros((0, 4), np.uint8)
        keep += [env_ids, envs, tex_ids, entries, texels_f, texels_b]
        abi.num_environments, abi.environment_ids, abi.environments = len(self.environments), env_ids.ctypes.data, C.cast(envs, C.c_void_p).value
        abi.num_textures, abi.texture_ids, abi.textures = len(self.textures), tex_ids.ctypes.data, C.cast(entries, C.c_void_p).value
        abi.num_texels_f, abi.texels_f = len(texels_f), texels_f.ctypes.data
        abi.num_texels_b, abi.texels_b = len(texels_b), texels_b.ctypes.data
        return abi, keep


@dataclass
class VolumeSource:
    """One volume entry of a VolumeEdit (include/vpt.h: vpt_volume_source): whd (w, h, d) and res of the volume AFTER the edit, the box
    region_lo .. region_lo + region_whd it writes, the mode, and where the values come from: voxels (a float32 array of shape region
    (d, h, w)), or a bake (positions (n, 3), triangles (m, 3), origin, step: the grid of bake_sdf_grid over whd)."""
    whd: tuple
    res: float
    region_lo: tuple
    region_whd: tuple
    mode: int = VOXELS_REPLACE
    voxels: Optional[np.ndarray] = None
    bake: Optional[tuple] = None   # (positions, triangles, origin, step)


class VolumeEdit:
    """What vpt_scene_update_volumes takes (include/vpt.h: vpt_volume_edit), as dictionaries id -> value: vol_instances
    (VptVolumeInstance), sdfs (VptSdf) and volumes (VolumeSource).  HostScene's set_volume_instance / set_sdf / set_volume /
    bake_volume fill one; DeviceScene.update_volumes / MultiDeviceScene.update_volumes / RenderSession.edit_volumes apply it."""

    def __init__(self, vol_instances=None, sdfs=None, volumes=None):
        self.vol_instances, self.sdfs, self.volumes = dict(vol_instances or {}), dict(sdfs or {}), dict(volumes or {})

    def empty(self) -> bool:
        return not (self.vol_instances or self.sdfs or self.volumes)

    def to_abi(self):
        """(VptVolumeEdit, objects that keep its arrays alive)"""
        keep, abi = [], VptVolumeEdit()
        inst_ids = np.array(list(self.vol_instances.keys()), np.int32)
        insts = (VptVolumeInstance * max(1, len(self.vol_instances)))(*self.vol_instances.values())
        sdf_ids = np.array(list(self.sdfs.keys()), np.int32)
        sdfs = (VptSdf * max(1, len(self.sdfs)))(*self.sdfs.values())
        vol_ids = np.array(list(self.volumes.keys()), np.int32)
        entries = (VptVolumeSource * max(1, len(self.volumes)))()
        pool, count = [], 0
        for k, src in enumerate(self.volumes.values()):
            e = entries[k]
            e.whd[:], e.res = [int(v) for v in src.whd], float(src.res)
            e.region_lo[:], e.region_whd[:], e.mode = [int(v) for v in src.region_lo], [int(v) for v in src.region_whd], int(src.mode)
            if src.bake is not None:
                positions, triangles, origin, step = src.bake
                positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
                triangles = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
                desc = VptBakeDesc(len(positions), positions.ctypes.data, len(triangles), triangles.ctypes.data)
                desc.whd[:] = [int(v) for v in src.whd]
                desc.origin[:] = [float(v) for v in np.broadcast_to(np.asarray(origin, np.float32), (3,))]
                desc.step[:] = [float(v) for v in np.broadcast_to(np.asarray(step, np.float32), (3,))]
                keep += [positions, triangles, desc]
                e.offset, e.bake = -1, C.addressof(desc)
            else:
                voxels = np.ascontiguousarray(src.voxels, np.float32)
                if voxels.shape != tuple(int(v) for v in src.region_whd)[::-1]:
                    raise VptError(f"voxels of a volume edit have the region's shape (d, h, w) = {tuple(src.region_whd)[::-1]}, got {voxels.shape}")
                e.offset, e.bake = count, None
                pool.append(voxels.reshape(-1))
                count += voxels.size
        voxels = np.ascontiguousarray(np.concatenate(pool)) if pool else np.zeros(0, np.float32)
        keep += [inst_ids, insts, sdf_ids, sdfs, vol_ids, entries, voxels]
        abi.num_vol_instances, abi.vol_instance_ids, abi.vol_instances = len(self.vol_instances), inst_ids.ctypes.data, C.cast(insts, C.c_void_p).value
        abi.num_sdfs, abi.sdf_ids, abi.sdfs = len(self.sdfs), sdf_ids.ctypes.data, C.cast(sdfs, C.c_void_p).value
        abi.num_volumes, abi.volume_ids, abi.volumes = len(self.volumes), vol_ids.ctypes.data, C.cast(entries, C.c_void_p).value
        abi.num_voxels, abi.voxels = len(voxels), voxels.ctypes.data
        return abi, keep


# defaults of the denoising filter (include/vpt.h: VPT_DENOISE_DEFAULT_*)
DENOISE_ITERATIONS, DENOISE_SIGMA_LUMINANCE, DENOISE_SIGMA_NORMAL, DENOISE_SIGMA_ALBEDO = 5, 4.0, 0.35, 0.1


@dataclass
class PathtraceParams:
    """pathtrace_params, yocto_pathtrace.h:87-99 (same names, same defaults)."""
    camera: int = 0
    resolution: int = 720
    shader: str = "pathtrace"
    samples: int = 512
    bounces: int = 4
    noparallel: bool = False
    noimplicit_mis: bool = False
    spheretrace_maxiter: int = 450

    def to_abi(self) -> VptParams:
        if self.shader not in SHADER_NAMES:
            raise VptError("sampler unknown")  # reference: get_shader throws (cpp:947-950)
        return VptParams(self.camera, self.resolution, SHADER_NAMES.index(self.shader), self.samples,
                         self.bounces, int(self.noparallel), int(self.noimplicit_mis),
                         self.spheretrace_maxiter)


@dataclass
class DisplayParams:
    """vpt_display_params: the tone map of a display (pathtrace_params::exposure, filmic; tonemap's srgb flag)."""
    exposure: float = 0.0
    filmic: bool = False
    srgb: bool = True

    def to_abi(self) -> VptDisplay:
        return VptDisplay(self.exposure, int(self.filmic), int(self.srgb))


@dataclass
class PathtraceState:
    """pathtrace_state, yocto_pathtrace.h:57-64: row-major host arrays."""
    width: int
    height: int
    samples: int = 0
    image: np.ndarray = field(default=None)  # (h, w, 4) float32 running sums
    hits: np.ndarray = field(default=None)   # (h, w) int32
    rngs: np.ndarray = field(default=None)   # (h, w, 2) uint64 {state, inc}

    def copy(self) -> "PathtraceState":
        return PathtraceState(self.width, self.height, self.samples, self.image.copy(), self.hits.copy(),
                              self.rngs.copy())


# ---- prototypes -----------------------------------------------------------------------------
_p = C.c_void_p
hip.vpt_last_error.restype = C.c_char_p
hip.vpt_version.restype = C.c_char_p
hip.vpt_device_count.restype = C.c_int
hip.vpt_scene_create.argtypes = [_p, C.c_int, C.POINTER(_p)]
hip.vpt_scene_create_curves.argtypes = [_p, _p, C.c_int, C.POINTER(_p)]
hip.vpt_scene_destroy.argtypes = [_p]
hip.vpt_scene_destroy.restype = None
hip.vpt_scene_update.argtypes = [_p, C.POINTER(VptSceneEdit)]
hip.vpt_multi_update.argtypes = [_p, C.POINTER(VptSceneEdit)]
hip.vpt_scene_update_lights.argtypes = [_p, C.POINTER(VptSceneEdit)]
hip.vpt_multi_update_lights.argtypes = [_p, C.POINTER(VptSceneEdit)]
hip.vpt_session_edit_lights.argtypes = [_p, C.POINTER(VptSceneEdit)]
hip.vpt_scene_update_textures.argtypes = [_p, C.POINTER(VptTextureEdit)]
hip.vpt_multi_update_textures.argtypes = [_p, C.POINTER(VptTextureEdit)]
hip.vpt_session_edit_textures.argtypes = [_p, C.POINTER(VptTextureEdit)]
hip.vpt_scene_update_volumes.argtypes = [_p, C.POINTER(VptVolumeEdit)]
hip.vpt_multi_update_volumes.argtypes = [_p, C.POINTER(VptVolumeEdit)]
hip.vpt_session_edit_volumes.argtypes = [_p, C.POINTER(VptVolumeEdit)]
hip.vpt_scene_get_volumes.argtypes = [_p, _p, C.c_int, _p, C.c_int, _p, C.c_int]
hip.vpt_scene_get_voxels.argtypes = [_p, C.c_int, _p, C.c_int64]
hip.vpt_scene_get_lights.argtypes = [_p, _p, C.c_int, C.POINTER(C.c_int), _p, C.c_int64, C.POINTER(C.c_int64)]
hip.vpt_scene_light_tables_hash.argtypes = [_p, _p]
hip.vpt_scene_get_media.argtypes = [_p, _p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
hip.vpt_scene_get_bvh.argtypes = [_p, _p, C.c_int, _p, C.c_int64]
hip.vpt_scene_rebuild_bvh.argtypes = [_p, C.POINTER(VptBvhRebuild)]
hip.vpt_multi_rebuild_bvh.argtypes = [_p, C.POINTER(VptBvhRebuild)]
hip.vpt_session_rebuild_bvh.argtypes = [_p, C.POINTER(VptBvhRebuild)]
hip.vpt_scene_rebuild_bvh_quality.argtypes = [_p, C.POINTER(VptBvhRebuild), C.c_int]
hip.vpt_multi_rebuild_bvh_quality.argtypes = [_p, C.POINTER(VptBvhRebuild), C.c_int]
hip.vpt_session_rebuild_bvh_quality.argtypes = [_p, C.POINTER(VptBvhRebuild), C.c_int]
hip.vpt_scene_update_instances.argtypes = [_p, C.POINTER(VptInstanceEdit)]
hip.vpt_multi_update_instances.argtypes = [_p, C.POINTER(VptInstanceEdit)]
hip.vpt_session_edit_instances.argtypes = [_p, C.POINTER(VptInstanceEdit)]
hip.vpt_scene_get_instances.argtypes = [_p, _p, C.c_int, C.POINTER(C.c_int)]
hip.vpt_scene_instance_tables_hash.argtypes = [_p, _p]
hip.vpt_scene_update_shapes.argtypes = [_p, C.POINTER(VptShapeEdit)]
hip.vpt_multi_update_shapes.argtypes = [_p, C.POINTER(VptShapeEdit)]
hip.vpt_session_edit_shapes.argtypes = [_p, C.POINTER(VptShapeEdit)]
hip.vpt_scene_shape_tables_hash.argtypes = [_p, _p]
hip.vpt_scene_get_shape_counts.argtypes = [_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
hip.vpt_scene_get_bvh_counts.argtypes = [_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), _p]
hip.vpt_scene_get_bvh_prims.argtypes = [_p, _p, C.c_int, _p, C.c_int64]
hip.vpt_scene_update_stats.argtypes = [_p, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_float)]
hip.vpt_render.argtypes = [_p, C.POINTER(VptParams), C.c_int, C.c_int, C.c_int, _p, _p, _p, C.POINTER(C.c_int)]
hip.vpt_layout_slots.argtypes = [C.POINTER(VptLayout)]
hip.vpt_layout_slots.restype = C.c_int64
hip.vpt_state_upload.argtypes = [C.POINTER(VptLayout), _p, _p, _p, _p, _p, _p, _p]
hip.vpt_state_download.argtypes = [C.POINTER(VptLayout), _p, _p, _p, _p, _p, _p, _p]
hip.vpt_render_device.argtypes = [_p, C.POINTER(VptParams), C.POINTER(VptLayout), C.c_int, _p, _p, _p, _p]
hip.vpt_resolve_device.argtypes = [C.POINTER(VptLayout), _p, C.c_int, _p, _p]
hip.vpt_render_adaptive.argtypes = [_p, C.POINTER(VptParams), C.POINTER(VptAdaptive), C.c_int, C.c_int, _p, _p, _p, C.POINTER(C.c_int),
                                    C.POINTER(C.c_int64)]
hip.vpt_render_device_adaptive.argtypes = [_p, C.POINTER(VptParams), C.POINTER(VptAdaptive), C.POINTER(VptLayout), _p, _p, _p, _p,
                                           C.POINTER(C.c_int), C.POINTER(C.c_int64)]
hip.vpt_resolve_hits_device.argtypes = [C.POINTER(VptLayout), _p, _p, _p, _p]
hip.vpt_denoise_scratch_bytes.argtypes = [C.c_int, C.c_int]
hip.vpt_denoise_scratch_bytes.restype = C.c_int64
hip.vpt_denoise_device.argtypes = [C.POINTER(VptDenoise), C.c_int, C.c_int, _p, _p, _p, _p, _p, _p, _p]
hip.vpt_half_variance_device.argtypes = [C.c_int, C.c_int, _p, C.c_int, _p, C.c_int, _p, _p]
hip.vpt_denoise.argtypes = [C.POINTER(VptDenoise), C.c_int, C.c_int, C.c_int, _p, _p, _p, _p, _p]
hip.vpt_half_variance.argtypes = [C.c_int, C.c_int, C.c_int, _p, C.c_int, _p, C.c_int, _p]
hip.vpt_state_init_device.argtypes = [C.POINTER(VptLayout), _p, _p, _p, _p]
hip.vpt_tonemap_device.argtypes = [C.POINTER(VptDisplay), C.c_int, C.c_int, _p, _p, _p, _p]
hip.vpt_upscale_device.argtypes = [C.c_int, C.c_int, C.c_int, _p, C.c_int, C.c_int, _p, _p]
hip.vpt_tonemap.argtypes = [C.POINTER(VptDisplay), C.c_int, C.c_int, C.c_int, _p, _p, _p]
hip.vpt_scene_get_camera.argtypes = [_p, C.c_int, C.POINTER(VptCamera)]
hip.vpt_scene_get_device.argtypes = [_p]
hip.vpt_session_create.argtypes = [_p, C.POINTER(VptSessionParams), C.POINTER(_p)]
hip.vpt_session_destroy.argtypes = [_p]
hip.vpt_session_destroy.restype = None
hip.vpt_session_reset.argtypes = [_p, C.POINTER(VptSessionParams)]
hip.vpt_session_advance.argtypes = [_p, C.c_int]
hip.vpt_session_set_display.argtypes = [_p, C.POINTER(VptDisplay)]
hip.vpt_session_edit.argtypes = [_p, C.POINTER(VptSceneEdit)]
hip.vpt_session_get_display.argtypes = [_p, _p, _p]
hip.vpt_session_get_image.argtypes = [_p, _p]
hip.vpt_session_get_denoised.argtypes = [_p, _p]
hip.vpt_session_get_state.argtypes = [_p, _p, _p, _p, C.POINTER(C.c_int)]
hip.vpt_session_size.argtypes = [_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
hip.vpt_session_samples.argtypes = [_p]
hip.vpt_session_stats.argtypes = [_p, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
hip.vpt_adaptive_run_create.argtypes = [_p, C.POINTER(VptParams), C.POINTER(VptAdaptive), C.POINTER(VptLayout), _p, _p, _p, _p, C.POINTER(_p)]
hip.vpt_adaptive_run_rounds.argtypes = [_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
hip.vpt_adaptive_run_progress.argtypes = [_p, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int)]
hip.vpt_adaptive_run_noise_device.argtypes = [_p, _p, _p, _p]
hip.vpt_adaptive_run_stats_device.argtypes = [_p, _p, _p, _p]
hip.vpt_adaptive_run_destroy.argtypes = [_p]
hip.vpt_adaptive_run_destroy.restype = None
hip.vpt_box3_device.argtypes = [C.c_int, C.c_int, _p, _p, _p]
hip.vpt_session_set_adaptive.argtypes = [_p, C.POINTER(VptAdaptive)]
hip.vpt_session_progress.argtypes = [_p, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int)]
hip.vpt_session_get_hits.argtypes = [_p, _p]
hip.vpt_session_get_noise.argtypes = [_p, _p, _p]
hip.vpt_session_get_adaptive_stats.argtypes = [_p, _p, _p]
hip.vpt_render_aov_device.argtypes = [_p, C.POINTER(VptParams), C.POINTER(VptLayout), C.c_int, C.POINTER(VptAovPlanes), _p, _p, _p]
hip.vpt_resolve_ids_device.argtypes = [C.POINTER(VptLayout), _p, _p, _p, _p, _p]
hip.vpt_render_aov.argtypes = [_p, C.POINTER(VptParams), C.c_int, C.c_int, C.c_int, C.POINTER(VptAovPlanes), _p, _p, C.POINTER(C.c_int)]
hip.vpt_session_get_guides.argtypes = [_p, _p, _p]
hip.vpt_session_pick.argtypes = [_p, C.c_int, C.c_int, C.POINTER(VptPick)]
hip.vpt_session_get_ids.argtypes = [_p, _p, _p]
hip.vpt_last_kernel_ms.argtypes = [_p, C.POINTER(C.c_float)]
hip.vpt_intersect.argtypes = [_p, C.c_int, _p, C.c_int, _p, _p]
hip.vpt_build_bvh.argtypes = [C.c_int, _p, C.c_int, _p, C.c_int, C.POINTER(C.c_int), _p]
hip.vpt_build_bvh_quality.argtypes = [C.c_int, _p, C.c_int, C.c_int, _p, C.c_int, C.POINTER(C.c_int), _p]
hip.vpt_bake_sdf.argtypes = [C.c_int, C.POINTER(VptBakeDesc), _p, C.POINTER(VptBakeStats)]
hip.vpt_bake_feature_normals.argtypes = [C.POINTER(VptBakeDesc), _p, _p]
hip.vpt_last_wave_costs.argtypes = [_p, _p, C.c_int, C.POINTER(C.c_int)]
hip.vpt_scene_record_bytes.argtypes = [_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
hip.vpt_multi_create.argtypes = [_p, C.POINTER(C.c_int), C.c_int, C.POINTER(_p)]
hip.vpt_multi_create_curves.argtypes = [_p, _p, C.POINTER(C.c_int), C.c_int, C.POINTER(_p)]
hip.vpt_multi_destroy.argtypes = [_p]
hip.vpt_multi_destroy.restype = None
hip.vpt_multi_device_count.argtypes = [_p]
hip.vpt_multi_render.argtypes = [_p, C.POINTER(VptParams), C.c_int, C.c_int, C.c_int, _p, _p, _p, C.POINTER(C.c_int)]
hip.vpt_multi_get_render.argtypes = [_p, _p]
hip.vpt_multi_uploaded_parts.argtypes = [_p]
hip.vpt_multi_transport.argtypes = [_p]
hip.vpt_multi_transport.restype = C.c_char_p
hip.vpt_multi_set_state.argtypes = [_p, C.c_int, C.c_int, _p, _p, _p, C.c_int]
hip.vpt_multi_get_state.argtypes = [_p, _p, _p, _p, C.POINTER(C.c_int)]
hip.vpt_check_watchdog.argtypes = [_p]
hip.vpt_resolve_srgb8_device.argtypes = [C.POINTER(VptLayout), _p, C.c_int, _p, _p]
hip.vpt_selftest_reciprocal.argtypes = [C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
hip.vpt_selftest_light_cdf.argtypes = [_p, C.c_int, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_int)]
hip.vpt_kat_strides.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
hip.vpt_kat.argtypes = [_p, C.c_int, C.c_int, C.c_int, _p, _p]
hip.vpt_spheretrace.argtypes = [_p, C.c_int, _p, C.c_int, C.c_int, _p, _p]
hip.vpt_eval_lobes.argtypes = [_p, C.c_int, _p, _p]
hip.vpt_split_plan.argtypes = [C.c_int, _p, C.c_int, C.c_int, C.c_int, _p, C.POINTER(C.c_int)]
host.vpth_scene_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
host.vpth_scene_load.restype = _p
host.vpth_scene_load_ex.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int]
host.vpth_scene_load_ex.restype = _p
host.vpth_vertex_normals.argtypes = [_p, C.c_int, _p, C.c_int, C.c_int, C.c_int, _p, C.c_char_p, C.c_int]
host.vpth_displace_vertices.argtypes = [_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _p, _p, _p, C.c_int, C.c_int, _p, C.c_char_p, C.c_int]
host.vpth_catmullclark.argtypes = [_p, C.c_int, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, C.POINTER(C.c_int), _p, C.POINTER(C.c_int), C.c_char_p, C.c_int]
host.vpth_scene_free.argtypes = [_p]
host.vpth_scene_count.argtypes = [_p, C.c_int]
host.vpth_scene_get_item.argtypes = [_p, C.c_int, C.c_int, _p, C.c_int64]
host.vpth_scene_get_item.restype = C.c_int64
host.vpth_scene_set_item.argtypes = [_p, C.c_int, C.c_int, _p, C.c_int64, C.c_char_p, C.c_int]
host.vpth_scene_update_bvh.argtypes = [_p, C.c_char_p, C.c_int]
host.vpth_scene_rebuild_bvh.argtypes = [_p, _p, C.c_int, C.c_int, C.c_char_p, C.c_int]
host.vpth_scene_rebuild_bvh_quality.argtypes = [_p, _p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
host.vpth_scene_edit_instances.argtypes = [_p, _p, C.c_int, _p, _p, C.c_int, _p, C.c_int, C.c_char_p, C.c_int]
host.vpth_scene_edit_shapes.argtypes = [_p, _p, C.c_int, _p, _p, C.c_int, _p, C.c_int, C.c_char_p, C.c_int]
host.vpth_scene_update_lights.argtypes = [_p, C.c_char_p, C.c_int]
host.vpth_scene_free.restype = None
host.vpth_scene_get_environment.argtypes = [_p, C.c_int, C.POINTER(VptEnvironment)]
host.vpth_scene_set_environment.argtypes = [_p, C.c_int, C.POINTER(VptEnvironment), C.c_char_p, C.c_int]
host.vpth_scene_get_texture.argtypes = [_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _p, C.c_int64]
host.vpth_scene_set_texture.argtypes = [_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _p, C.c_char_p, C.c_int]
host.vpth_scene_update_textures.argtypes = [_p, C.c_char_p, C.c_int]
host.vpth_scene_count_implicit.argtypes = [_p, C.c_int]
host.vpth_scene_get_vol_instance.argtypes = [_p, C.c_int, C.POINTER(VptVolumeInstance)]
host.vpth_scene_set_vol_instance.argtypes = [_p, C.c_int, C.POINTER(VptVolumeInstance), C.c_char_p, C.c_int]
host.vpth_scene_get_sdf.argtypes = [_p, C.c_int, C.POINTER(VptSdf)]
host.vpth_scene_set_sdf.argtypes = [_p, C.c_int, C.POINTER(VptSdf), C.c_char_p, C.c_int]
host.vpth_scene_set_volume.argtypes = [_p, C.c_int, _p, C.c_float, _p, _p, C.c_int, _p, C.c_char_p, C.c_int]
host.vpth_scene_update_volumes.argtypes = [_p, C.c_char_p, C.c_int]
host.vpth_scene_desc.argtypes = [_p]
host.vpth_scene_desc.restype = _p
host.vpth_scene_curves.argtypes = [_p]
host.vpth_scene_curves.restype = _p
host.vpth_state_size.argtypes = [_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
host.vpth_make_state.argtypes = [_p, C.c_int, C.c_int, _p, _p, _p]
host.vpth_scene_stats.argtypes = [_p, C.c_char_p, C.c_int]
host.vpth_scene_rebuild_bvh_device.argtypes = [_p, C.c_int, C.c_char_p, C.c_int]
host.vpth_build_bvh_host.argtypes = [_p, C.c_int, _p, C.POINTER(C.c_int), _p]
host.vpth_scene_rebuild_bvh_device_quality.argtypes = [_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
host.vpth_build_bvh_host_quality.argtypes = [_p, C.c_int, C.c_int, _p, C.POINTER(C.c_int), _p]
host.vpth_denoise.argtypes = [C.c_int, C.c_int, _p, _p, _p, _p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, _p, C.c_char_p, C.c_int]
host.vpth_half_variance.argtypes = [C.c_int, C.c_int, _p, C.c_int, _p, C.c_int, C.c_int, _p, C.c_char_p, C.c_int]
host.vpth_bake_triangles.argtypes = [_p, C.c_int, C.c_int, _p, C.POINTER(C.c_int)]
host.vpth_bake_grid.argtypes = [_p, C.c_int, _p, C.c_int, _p, _p, _p, C.c_int, _p, C.POINTER(VptBakeStats), C.c_char_p, C.c_int]
host.vpth_fit_volume.argtypes = [_p, _p, _p, C.c_int, C.POINTER(C.c_float), _p, _p, _p, C.c_char_p, C.c_int]
host.vpth_bake_volume.argtypes = [_p, C.c_int, _p, C.c_int, _p, C.c_int, C.c_int, _p, C.POINTER(C.c_float), _p, C.POINTER(VptBakeStats),
                                  C.c_char_p, C.c_int]
host.vpth_scene_get_volume.argtypes = [_p, C.c_int, _p, C.POINTER(C.c_float), _p, C.c_int64]
host.vpth_scene_get_volume.restype = C.c_int64
host.vpth_save_volume.argtypes = [C.c_char_p, _p, C.c_float, _p, C.c_char_p, C.c_int]
host.vpth_tonemap.argtypes = [C.c_int64, _p, C.c_float, C.c_int, C.c_int, _p, _p]
host.vpth_upscale_preview.argtypes = [C.c_int, C.c_int, C.c_int, _p, C.c_int, C.c_int, _p]
host.vpth_make_state_jump.argtypes = [C.c_int, C.c_int, _p]
host.vpth_linear_to_srgb8.argtypes = [C.c_int, C.c_int, _p, C.c_int, _p]
host.vpth_linear_to_srgb8.restype = None
host.vpth_encode_jpeg_q75.argtypes = [C.c_int, C.c_int, _p, _p, C.c_int64]
host.vpth_encode_jpeg_q75.restype = C.c_int64


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise VptError(f"{what} failed ({rc}): {hip.vpt_last_error().decode()}")


def device_count() -> int:
    return hip.vpt_device_count()


BVH_NODE = np.dtype([("bbox_min", np.float32, 3), ("bbox_max", np.float32, 3), ("start", np.int32), ("num", np.int16), ("axis", np.int8),
                     ("internal", np.uint8)])
assert BVH_NODE.itemsize == 32


class VptSceneDescBvh(C.Structure):
    """the last four tables of vpt_scene_desc (the two-level BVH); OFFSET: where they start (10 int32 + pointer tables, then 10
    int64 + pointer pools: every pair takes 16 bytes)"""
    _fields_ = [("num_scene_bvh_nodes", C.c_int32), ("scene_bvh_nodes", C.c_void_p), ("num_scene_bvh_prims", C.c_int32),
                ("scene_bvh_prims", C.c_void_p), ("num_shape_bvh_nodes", C.c_int64), ("shape_bvh_nodes", C.c_void_p),
                ("num_shape_bvh_prims", C.c_int64), ("shape_bvh_prims", C.c_void_p)]
    OFFSET = 20 * 16


LIGHT = np.dtype([("instance", np.int32), ("environment", np.int32), ("sdf", np.int32), ("cdf_len", np.int32), ("cdf_offset", np.int64)])   # vpt_light
assert LIGHT.itemsize == 24


class VptSceneDescImplicit(C.Structure):
    """the three tables of vpt_scene_desc behind the implicit shaders: its seventh to ninth {int32 count, pointer} pairs"""
    _fields_ = [("num_volumes", C.c_int32), ("volumes", C.c_void_p), ("num_vol_instances", C.c_int32), ("vol_instances", C.c_void_p),
                ("num_sdfs", C.c_int32), ("sdfs", C.c_void_p)]
    OFFSET = 6 * 16


class VptSceneDescVoxels(C.Structure):
    """the voxel pool of vpt_scene_desc: its ninth {int64 count, pointer} pool"""
    _fields_ = [("num_voxels", C.c_int64), ("voxels", C.c_void_p)]
    OFFSET = 10 * 16 + 8 * 16


class VptSceneDescLights(C.Structure):
    """vpt_scene_desc up to its CDF pool, for the two tables of the lights: the tenth {int32 count, pointer} pair and the tenth
    {int64 count, pointer} pool"""
    _fields_ = [("tables", C.c_byte * (9 * 16)), ("num_lights", C.c_int32), ("lights", C.c_void_p), ("pools", C.c_byte * (9 * 16)),
                ("num_light_cdf", C.c_int64), ("light_cdf", C.c_void_p)]


BVH_MIDDLE, BVH_SAH = 0, 1   # VPT_BVH_MIDDLE, VPT_BVH_SAH


def build_bvh(bboxes: np.ndarray, device: Optional[int] = 0, *, quality: int = 0):
    """build_bvh(bvh, bboxes, highquality = quality) of the reference over n boxes {min.xyz, max.xyz}: (nodes, primitives).  device = GPU
    index (vpt_build_bvh_quality) or None for the host build the loader uses (same arrays).  quality: BVH_MIDDLE or BVH_SAH."""
    if quality not in (BVH_MIDDLE, BVH_SAH):
        raise VptError(f"build_bvh: unknown quality {quality!r}")
    bboxes = np.ascontiguousarray(bboxes, np.float32).reshape(-1, 6)
    n = len(bboxes)
    nodes = np.zeros(max(1, 2 * n), BVH_NODE)
    prims = np.zeros(max(1, n), np.int32)
    count = C.c_int()
    if device is None:
        if host.vpth_build_bvh_host_quality(bboxes.ctypes.data, n, quality, nodes.ctypes.data, C.byref(count), prims.ctypes.data) != 0:
            raise VptError("vpth_build_bvh_host_quality: bad argument")
    else:
        _check(hip.vpt_build_bvh_quality(device, bboxes.ctypes.data, n, quality, nodes.ctypes.data, len(nodes), C.byref(count), prims.ctypes.data), "vpt_build_bvh_quality")
    return nodes[:count.value].copy(), prims[:n].copy()


def catmullclark(quads: np.ndarray, verts: np.ndarray, lock_boundary: bool = False, device: Optional[int] = None):
    """one level of the reference's tesselate_catmullclark (yocto_pathtrace.cpp:1119-1226) on an (n, 4) int32 quad array (z == w: a
    triangle) and an (m, 2 | 3) float32 vertex array: (new quads, new vertices).  device: GPU index for the vertex arithmetic."""
    quads = np.ascontiguousarray(quads, np.int32).reshape(-1, 4)
    verts = np.ascontiguousarray(verts, np.float32)
    n, (m, dim) = len(quads), verts.shape
    qo, vo = np.zeros((4 * n, 4), np.int32), np.zeros((m + 5 * n, dim), np.float32)
    nq, nv = C.c_int(), C.c_int()
    err = C.create_string_buffer(512)
    if host.vpth_catmullclark(quads.ctypes.data, n, verts.ctypes.data, m, dim, int(lock_boundary), -1 if device is None else device,
                              qo.ctypes.data, C.byref(nq), vo.ctypes.data, C.byref(nv), err, len(err)) != 0:
        raise VptError(err.value.decode())
    return qo[:nq.value].copy(), vo[:nv.value].copy()


def vertex_normals(positions: np.ndarray, faces: np.ndarray, device: Optional[int] = None) -> np.ndarray:
    """quads_normals ((n, 4) faces; z == w: a triangle) / triangles_normals ((n, 3)) of yocto_shape.cpp:1478-1512 over (m, 3) float32
    positions: area-weighted face normals added per vertex in face order, normalised.  device: GPU index (vpt_vertex_normals)."""
    positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32)
    out = np.zeros_like(positions)
    err = C.create_string_buffer(512)
    if host.vpth_vertex_normals(positions.ctypes.data, len(positions), faces.ctypes.data, len(faces), faces.shape[1], -1 if device is None else device,
                                out.ctypes.data, err, len(err)) != 0:
        raise VptError(err.value.decode())
    return out


def displace_vertices(texels: np.ndarray, linear: bool, displacement: float, positions: np.ndarray, normals: np.ndarray, texcoords: np.ndarray,
                      device: Optional[int] = None) -> np.ndarray:
    """the displacement step of tesselate_surface (yocto_pathtrace.cpp:1259-1265): positions + normals * displacement * (mean(rgb of
    eval_texture(uv, as_linear)) [- 0.5 for uint8 texels]).  texels: (h, w, 4) uint8 or float32.  device: GPU index (vpt_displace_vertices)."""
    texels = np.ascontiguousarray(texels)
    assert texels.ndim == 3 and texels.shape[2] == 4 and texels.dtype in (np.uint8, np.float32)
    positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    texcoords = np.ascontiguousarray(texcoords, np.float32).reshape(-1, 2)
    out = np.zeros_like(positions)
    err = C.create_string_buffer(512)
    if host.vpth_displace_vertices(texels.ctypes.data, texels.shape[1], texels.shape[0], int(texels.dtype == np.float32), int(linear), C.c_float(displacement),
                                   positions.ctypes.data, normals.ctypes.data, texcoords.ctypes.data, len(positions), -1 if device is None else device,
                                   out.ctypes.data, err, len(err)) != 0:
        raise VptError(err.value.decode())
    return out


def bake_triangles(faces: np.ndarray) -> np.ndarray:
    """the (m, 3) int32 triangles a bake takes from (n, 3) triangles or (n, 4) quads: a quad is split as the reference's geometry code
    does, (x, y, w) and (z, w, y); a quad with z == w is the triangle (x, y, z)"""
    faces = np.ascontiguousarray(faces, np.int32)
    if faces.ndim != 2 or faces.shape[1] not in (3, 4):
        raise VptError(f"expected (n, 3) or (n, 4) faces, got {faces.shape}")
    out = np.zeros((max(1, 2 * len(faces)), 3), np.int32)
    count = C.c_int()
    if host.vpth_bake_triangles(faces.ctypes.data, len(faces), faces.shape[1], out.ctypes.data, C.byref(count)) != 0:
        raise VptError("bake_triangles: bad faces")
    return out[:count.value].copy()


def _bake_stats(st: VptBakeStats) -> dict:
    return {name: getattr(st, name) for name, _ in VptBakeStats._fields_}


def _whd3(whd) -> np.ndarray:
    whd = np.ascontiguousarray(np.broadcast_to(np.asarray(whd), (3,)), np.int32)
    return whd


def bake_sdf_grid(positions: np.ndarray, triangles: np.ndarray, whd, origin, step, device: Optional[int] = 0):
    """vpt_bake_sdf (include/vpt.h) over an explicit grid: voxel (i, j, k) of whd = (w, h, d) is sampled at origin + (i, j, k) * step in the
    mesh's space.  (voxels of shape (d, h, w) float32, stats).  device None: the host mirror (16 CPU threads, every triangle per voxel);
    else that GPU - the same bits."""
    positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    triangles = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    whd = _whd3(whd)
    origin = np.ascontiguousarray(np.broadcast_to(np.asarray(origin, np.float32), (3,)), np.float32)
    step = np.ascontiguousarray(np.broadcast_to(np.asarray(step, np.float32), (3,)), np.float32)
    n = int(whd[0]) * int(whd[1]) * int(whd[2])
    voxels = np.zeros(n if (whd >= 1).all() and n < 2 ** 31 else 1, np.float32)
    st = VptBakeStats()
    err = C.create_string_buffer(512)
    if host.vpth_bake_grid(positions.ctypes.data, len(positions), triangles.ctypes.data, len(triangles), whd.ctypes.data, origin.ctypes.data,
                           step.ctypes.data, -1 if device is None else device, voxels.ctypes.data, C.byref(st), err, len(err)) != 0:
        raise VptError(err.value.decode())
    return voxels.reshape(int(whd[2]), int(whd[1]), int(whd[0])), _bake_stats(st)


def fit_volume(bmin, bmax, whd, padding: int = 2):
    """the grid of whd voxels around the box [bmin, bmax] that the renderer's lookup reads back in place (vpt_host.h: fit_volume):
    (res, origin, step, frame) - step = res * W / (W - 1) per axis, the box centred with `padding` voxels to spare on each side,
    frame the (4, 3) instance frame with o = -origin."""
    bmin = np.ascontiguousarray(bmin, np.float32).reshape(3)
    bmax = np.ascontiguousarray(bmax, np.float32).reshape(3)
    whd = _whd3(whd)
    res = C.c_float()
    origin, step, frame = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros((4, 3), np.float32)
    err = C.create_string_buffer(512)
    if host.vpth_fit_volume(bmin.ctypes.data, bmax.ctypes.data, whd.ctypes.data, padding, C.byref(res), origin.ctypes.data, step.ctypes.data,
                            frame.ctypes.data, err, len(err)) != 0:
        raise VptError(err.value.decode())
    return res.value, origin, step, frame


def save_volume(path: str, voxels: np.ndarray, res: float) -> None:
    """the binary .sdf file the scene loader reads ("binary": true): int32 w h d, float res, 16 floats, the voxels; voxels of shape (d, h, w)"""
    voxels = np.ascontiguousarray(voxels, np.float32)
    if voxels.ndim != 3:
        raise VptError(f"expected (d, h, w) voxels, got {voxels.shape}")
    whd = np.array(voxels.shape[::-1], np.int32)
    err = C.create_string_buffer(512)
    if host.vpth_save_volume(os.fsencode(path), whd.ctypes.data, C.c_float(res), voxels.ctypes.data, err, len(err)) != 0:
        raise VptError(err.value.decode())


@dataclass
class BakedVolume:
    """bake_sdf's result: the grid and the vol_instances entry that puts it back where the mesh was"""
    voxels: np.ndarray   # (d, h, w) float32
    res: float
    frame: np.ndarray    # (4, 3) float32: x, y, z, o
    scalef: float
    stats: dict

    def save(self, path: str) -> None:
        save_volume(path, self.voxels, self.res)


def bake_sdf(positions: np.ndarray, faces: np.ndarray, whd, padding: int = 2, device: Optional[int] = 0) -> BakedVolume:
    """A mesh ((m, 3) float32 positions, (n, 3) triangles or (n, 4) quads) baked into a signed-distance grid of whd = (w, h, d) voxels (one
    int: a cube) fitted around it with `padding` voxels to spare (fit_volume), by the rule of include/vpt.h (vpt_bake_sdf): negative
    inside.  device: GPU index, or None for the host mirror - the same bits."""
    positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    triangles = bake_triangles(faces)
    whd = _whd3(whd)
    n = int(whd[0]) * int(whd[1]) * int(whd[2])
    voxels = np.zeros(n if (whd >= 1).all() and n < 2 ** 31 else 1, np.float32)
    res, frame, st = C.c_float(), np.zeros((4, 3), np.float32), VptBakeStats()
    err = C.create_string_buffer(512)
    if host.vpth_bake_volume(positions.ctypes.data, len(positions), triangles.ctypes.data, len(triangles), whd.ctypes.data, padding,
                             -1 if device is None else device, voxels.ctypes.data, C.byref(res), frame.ctypes.data, C.byref(st), err, len(err)) != 0:
        raise VptError(err.value.decode())
    return BakedVolume(voxels.reshape(int(whd[2]), int(whd[1]), int(whd[0])), res.value, frame, 1.0, _bake_stats(st))


class HostScene:
    """load_scene + tesselate_surfaces + make_bvh + make_lights, flattened for the C-ABI."""

    def __init__(self, filename: str, bvh_device: Optional[int] = None, tess_device: Optional[int] = None, *, bvh_quality: int = 0):
        """bvh_device: build the BVHs on that GPU (make_bvh_device / vpt_build_bvh_quality) instead of on the host - same arrays;
        tess_device: the vertex arithmetic of tesselate_surfaces on that GPU (vpt_subdivide_vertices) - same mesh;
        bvh_quality: BVH_MIDDLE, or BVH_SAH for make_bvh(..., highquality = true) - every tree is built at that quality after loading"""
        if bvh_quality not in (BVH_MIDDLE, BVH_SAH):
            raise VptError(f"HostScene: unknown bvh_quality {bvh_quality!r}")
        err = C.create_string_buffer(1024)
        self.handle = host.vpth_scene_load_ex(os.fsencode(filename), -1 if tess_device is None else tess_device, err, len(err))
        if not self.handle:
            raise VptError(err.value.decode())
        self.filename = filename
        if bvh_device is not None and host.vpth_scene_rebuild_bvh_device_quality(self.handle, bvh_device, bvh_quality, err, len(err)) != 0:
            raise VptError(err.value.decode())
        if bvh_device is None and bvh_quality != BVH_MIDDLE:
            self.rebuild_bvh("all", quality=bvh_quality)

    @property
    def desc(self) -> int:
        """address of the vpt_scene_desc (valid while this object lives)"""
        self._run_bakes()
        return host.vpth_scene_desc(self.handle)

    @property
    def curves(self) -> Optional[int]:
        """address of the vpt_scene_curves beside the descriptor, None when no shape has points or lines"""
        return host.vpth_scene_curves(self.handle)

    def stats(self) -> str:
        self._run_bakes()
        buf = C.create_string_buffer(1 << 20)
        n = host.vpth_scene_stats(self.handle, buf, len(buf))
        if n < 0:
            raise VptError("stats buffer too small")
        return buf.value.decode()

    # -- editing (the host side of vpt_scene_update, include/vpt.h).  Getters return copies; setters replace an item in the scene and
    #    in the descriptor and note it in the pending SceneEdit; update_bvh() refits the BVHs and hands that edit out --------------
    _CAMERA, _INSTANCE, _ENVIRONMENT, _MATERIAL, _POSITIONS, _NORMALS = range(6)

    def count(self, kind: str) -> int:
        """number of "cameras", "instances", "environments", "materials" or "shapes"""
        return host.vpth_scene_count(self.handle, {"cameras": 0, "instances": 1, "environments": 2, "materials": 3, "shapes": 4}[kind])

    def _get(self, kind: int, index: int, out, nbytes=None):
        n = host.vpth_scene_get_item(self.handle, kind, index, None, 0)
        if n < 0:
            raise VptError(f"item {index} out of range")
        if out is None:
            out = np.zeros(n // 4, np.float32)
        ptr = out.ctypes.data if isinstance(out, np.ndarray) else C.addressof(out)
        host.vpth_scene_get_item(self.handle, kind, index, ptr, n)
        return out

    def _set(self, kind: int, index: int, value) -> None:
        if isinstance(value, np.ndarray):
            ptr, n = value.ctypes.data, value.nbytes
        else:
            ptr, n = C.addressof(value), C.sizeof(value)
        err = C.create_string_buffer(512)
        if host.vpth_scene_set_item(self.handle, kind, index, ptr, n, err, len(err)) != 0:
            raise VptError(err.value.decode())

    def _pending(self) -> SceneEdit:
        if getattr(self, "_edit", None) is None:
            self._edit = SceneEdit()
        return self._edit

    def camera(self, index: int) -> VptCamera:
        return self._get(self._CAMERA, index, VptCamera())

    def instance_frame(self, index: int) -> np.ndarray:
        """(12,) float32: x, y, z, o"""
        return self._get(self._INSTANCE, index, np.zeros(12, np.float32))

    def environment_frame(self, index: int) -> np.ndarray:
        return self._get(self._ENVIRONMENT, index, np.zeros(12, np.float32))

    def material(self, index: int) -> VptMaterial:
        return self._get(self._MATERIAL, index, VptMaterial())

    def instance_ids(self, index: int):
        """(shape, material) of an instance"""
        a = self._get(6, index, np.zeros(2, np.int32))
        return int(a[0]), int(a[1])

    def shape_positions(self, index: int) -> np.ndarray:
        return self._get(self._POSITIONS, index, None).reshape(-1, 3)

    def shape_normals(self, index: int) -> np.ndarray:
        """(n, 3) float32; (0, 3) for a shape without normals"""
        return self._get(self._NORMALS, index, None).reshape(-1, 3)

    def shape_arrays(self, index: int) -> dict:
        """every array of a shape as loaded and tesselated: positions, normals (n, 3), texcoords (n, 2), colors (n, 4), radius (n,)
        float32; triangles (m, 3), quads (m, 4), points (m,), lines (m, 2) int32 (empty where the shape has none)"""
        f = lambda kind, width: self._get(kind, index, None).reshape(-1, width) if width else self._get(kind, index, None)
        i = lambda kind, width: self._get(kind, index, None).view(np.int32).reshape((-1, width) if width else (-1,))
        return {"positions": f(4, 3), "normals": f(5, 3), "texcoords": f(7, 2), "colors": f(8, 4), "radius": f(9, 0),
                "triangles": i(10, 3), "quads": i(11, 4), "points": i(12, 0), "lines": i(13, 2)}

    def volume(self, index: int):
        """volume `index` as the scene holds it: (voxels of shape (d, h, w) float32, res)"""
        self._run_bakes()
        whd, res = np.zeros(3, np.int32), C.c_float()
        n = host.vpth_scene_get_volume(self.handle, index, whd.ctypes.data, C.byref(res), None, 0)
        if n < 0:
            raise VptError(f"volume {index} out of range")
        voxels = np.zeros(n, np.float32)
        host.vpth_scene_get_volume(self.handle, index, whd.ctypes.data, C.byref(res), voxels.ctypes.data, n)
        return voxels.reshape(int(whd[2]), int(whd[1]), int(whd[0])), res.value

    def set_camera(self, index: int, camera: VptCamera) -> None:
        self._set(self._CAMERA, index, camera)
        self._pending().cameras[index] = self.camera(index)

    def set_instance_frame(self, index: int, frame) -> None:
        self._no_pending_instances("set_instance_frame")
        frame = np.ascontiguousarray(frame, np.float32).reshape(12)
        self._set(self._INSTANCE, index, frame)
        self._pending().instances[index] = frame.copy()

    def set_environment_frame(self, index: int, frame) -> None:
        frame = np.ascontiguousarray(frame, np.float32).reshape(12)
        self._set(self._ENVIRONMENT, index, frame)
        self._pending().environments[index] = frame.copy()

    def set_material(self, index: int, material: VptMaterial) -> None:
        self._set(self._MATERIAL, index, material)
        self._pending().materials[index] = self.material(index)

    def set_shape_positions(self, index: int, positions, normals=None) -> None:
        """the vertices of a shape (same count), and its normals when given"""
        self._no_pending_instances("set_shape_positions")
        positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        self._set(self._POSITIONS, index, positions)
        if normals is not None:
            normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
            self._set(self._NORMALS, index, normals)
            normals = normals.copy()
        elif index in self._pending().shapes:
            normals = self._pending().shapes[index][1]
        self._pending().shapes[index] = (positions.copy(), normals)

    def update_bvh(self) -> SceneEdit:
        """update_bvh of the reference over what the setters changed since the last call (a refit: topology and primitive order stay);
        desc / stats() describe the edited scene afterwards.  Returns the SceneEdit for DeviceScene.update."""
        err = C.create_string_buffer(512)
        if host.vpth_scene_update_bvh(self.handle, err, len(err)) != 0:
            raise VptError(err.value.decode())
        edit, self._edit = self._pending(), None
        return edit

    def update_lights(self) -> SceneEdit:
        """update_bvh(), then make_lights of the edited scene (an emission switched on or off, an emitter's vertices moved): desc /
        stats() carry the new light list and CDFs.  Returns the SceneEdit for DeviceScene.update_lights."""
        edit = self.update_bvh()
        err = C.create_string_buffer(512)
        if host.vpth_scene_update_lights(self.handle, err, len(err)) != 0:
            raise VptError(err.value.decode())
        return edit

    def rebuild_bvh(self, shapes=None, scene: bool = True, *, quality: int = 0) -> "BvhRebuild":
        """make_bvh of the reference again, on the scene as it is now, for the shapes named (ids; "all": every shape; None: none) and
        - `scene`, or whenever a shape is named - for the scene BVH: topology, node counts and primitive orders change; desc / stats()
        describe the rebuilt scene afterwards.  A pending edit is handed out with update_bvh() first.  Returns the BvhRebuild for
        DeviceScene.rebuild_bvh.  quality: BVH_MIDDLE or BVH_SAH for every tree this call builds; the others keep theirs."""
        if quality not in (BVH_MIDDLE, BVH_SAH):
            raise VptError(f"rebuild_bvh: unknown quality {quality!r}")
        if getattr(self, "_edit", None) is not None and not self._edit.empty():
            raise VptError("rebuild_bvh: hand the pending edit out with update_bvh() first")
        self._no_pending_instances("rebuild_bvh")
        ids = list(range(self.count("shapes"))) if isinstance(shapes, str) and shapes == "all" else [int(i) for i in (shapes or ())]
        arr = np.ascontiguousarray(ids, np.int32)
        err = C.create_string_buffer(512)
        if host.vpth_scene_rebuild_bvh_quality(self.handle, arr.ctypes.data if len(arr) else None, len(arr), int(bool(scene)), quality, err, len(err)) != 0:
            raise VptError(err.value.decode())
        return BvhRebuild(ids, scene, quality=quality)

    # -- the set of instances (the host side of vpt_scene_update_instances): add_instance / remove_instances / set_instance note a
    #    change, ids naming the list as it is now; update_instances() applies them to the scene - set, then remove, then add - builds
    #    the scene BVH and the lights anew and hands the InstanceEdit out.  The ids of a pending SceneEdit name the old list, so the
    #    two kinds of change do not mix: each is handed out before the other begins ------------------------------------------------
    def _pending_instances(self) -> InstanceEdit:
        if getattr(self, "_inst_edit", None) is None:
            self._inst_edit = InstanceEdit()
        return self._inst_edit

    def _no_pending_instances(self, what: str) -> None:
        if getattr(self, "_inst_edit", None) is not None and not self._inst_edit.empty():
            raise VptError(f"{what}: hand the pending instance changes out with update_instances() first")
        if getattr(self, "_shape_edit", None) is not None and not self._shape_edit.empty():
            raise VptError(f"{what}: hand the pending shape changes out with update_shapes() first")

    def _begin_instance_change(self, what: str) -> InstanceEdit:
        if getattr(self, "_edit", None) is not None and (self._edit.instances or self._edit.shapes):
            raise VptError(f"{what}: hand the pending edit out with update_bvh() first (its ids name the instances as they are now)")
        if getattr(self, "_shape_edit", None) is not None and not self._shape_edit.empty():
            raise VptError(f"{what}: hand the pending shape changes out with update_shapes() first")
        return self._pending_instances()

    def _check_instance(self, what: str, frame, shape: int, material: int):
        frame = np.ascontiguousarray(frame, np.float32).reshape(-1)
        if frame.size != 12 or not np.all(np.isfinite(frame)):
            raise VptError(f"{what}: a frame is twelve finite floats (x, y, z, o)")
        if not 0 <= int(shape) < self.count("shapes"):
            raise VptError(f"{what}: shape {shape} out of range")
        if not 0 <= int(material) < self.count("materials"):
            raise VptError(f"{what}: material {material} out of range")
        return frame.copy(), int(shape), int(material)

    def add_instance(self, frame, shape: int, material: int) -> int:
        """notes a new instance, appended at update_instances(); returns the id it has afterwards (given the removals noted so far)"""
        pend = self._begin_instance_change("add_instance")
        pend.add.append(self._check_instance("add_instance", frame, shape, material))
        return self.count("instances") - len(pend.remove) + len(pend.add) - 1

    def remove_instances(self, ids) -> None:
        """notes instances (current ids) to erase at update_instances(): the survivors keep their order, the ids close up"""
        pend = self._begin_instance_change("remove_instances")
        ids = [int(i) for i in ids]
        for i in ids:
            if not 0 <= i < self.count("instances"):
                raise VptError(f"remove_instances: instance {i} out of range")
            if i in pend.set:
                raise VptError(f"remove_instances: instance {i} is also set")
        if len(set(ids)) != len(ids) or set(ids) & set(pend.remove):
            raise VptError("remove_instances: an id is repeated")
        pend.remove = pend.remove + tuple(ids)

    def set_instance(self, index: int, frame=None, shape: Optional[int] = None, material: Optional[int] = None) -> None:
        """notes another frame, shape or material (None: as it is) for instance `index` (current id), applied at update_instances()"""
        pend = self._begin_instance_change("set_instance")
        index = int(index)
        if not 0 <= index < self.count("instances"):
            raise VptError(f"set_instance: instance {index} out of range")
        if index in pend.remove:
            raise VptError(f"set_instance: instance {index} is also removed")
        was = pend.set[index] if index in pend.set else (self.instance_frame(index),) + self.instance_ids(index)
        pend.set[index] = self._check_instance("set_instance", was[0] if frame is None else frame, was[1] if shape is None else shape,
                                               was[2] if material is None else material)

    def update_instances(self) -> InstanceEdit:
        """edit_instances of the host library over what add_instance / remove_instances / set_instance noted since the last call:
        erase / replace / push_back on the scene's instances, the scene BVH built anew (make_bvh's scene level), make_lights; desc /
        stats() describe the edited scene afterwards.  Returns the InstanceEdit for DeviceScene.update_instances."""
        if getattr(self, "_edit", None) is not None and (self._edit.instances or self._edit.shapes):
            raise VptError("update_instances: hand the pending edit out with update_bvh() first")
        if getattr(self, "_shape_edit", None) is not None and not self._shape_edit.empty():
            raise VptError("update_instances: hand the pending shape changes out with update_shapes() first")
        edit, self._inst_edit = self._pending_instances(), None
        if edit.empty():
            return edit
        abi, keep = edit.to_abi()
        err = C.create_string_buffer(512)
        if host.vpth_scene_edit_instances(self.handle, abi.remove_ids, abi.num_remove, abi.set_ids, abi.set, abi.num_set, abi.add, abi.num_add,
                                          err, len(err)) != 0:
            raise VptError(err.value.decode())
        del keep
        return edit

    # -- the shape list (the host side of vpt_scene_update_shapes): add_shape / set_shape / remove_shapes note a change, ids naming the
    #    list as it is now; update_shapes() applies them to the scene - set, then remove, then add - builds the new shapes' BVHs (and the
    #    scene BVH when a shape was replaced) and the lights anew and hands the ShapeEdit out.  The ids of a pending SceneEdit or
    #    InstanceEdit name the old list, so the kinds of change do not mix: each is handed out before another begins ---------------------
    def _begin_shape_change(self, what: str) -> ShapeEdit:
        if getattr(self, "_edit", None) is not None and (self._edit.instances or self._edit.shapes):
            raise VptError(f"{what}: hand the pending edit out with update_bvh() first (its ids name the shapes as they are now)")
        if getattr(self, "_inst_edit", None) is not None and not self._inst_edit.empty():
            raise VptError(f"{what}: hand the pending instance changes out with update_instances() first")
        if getattr(self, "_shape_edit", None) is None:
            self._shape_edit = ShapeEdit()
        return self._shape_edit

    @staticmethod
    def _check_mesh(what: str, m: dict) -> dict:
        nv = 0 if m["positions"] is None else len(m["positions"])
        kinds = [k for k in MESH_ELEMENTS if m[k] is not None]
        if len(kinds) > 1:
            raise VptError(f"{what}: a shape holds one kind of element, not {' and '.join(kinds)}")
        for key in MESH_FLOATS:
            if m[key] is not None and (len(m[key]) != nv or not np.all(np.isfinite(m[key]))):
                raise VptError(f"{what}: {key} must be finite and one per vertex")
        for key in kinds:
            if m[key].min() < 0 or m[key].max() >= nv:
                raise VptError(f"{what}: a vertex index of {key} is out of range")
        if (m["points"] is not None or m["lines"] is not None) and m["radius"] is None:
            raise VptError(f"{what}: a shape of points or lines needs one radius per vertex")
        return m

    def add_shape(self, positions, triangles=None, quads=None, points=None, lines=None, normals=None, texcoords=None, colors=None, radius=None) -> int:
        """notes a new shape, appended at update_shapes(); returns the id it has afterwards (given the removals noted so far)"""
        pend = self._begin_shape_change("add_shape")
        pend.add.append(self._check_mesh("add_shape", mesh(positions, triangles, quads, points, lines, normals, texcoords, colors, radius)))
        return self.count("shapes") - len(pend.remove) + len(pend.add) - 1

    def set_shape(self, index: int, positions, triangles=None, quads=None, points=None, lines=None, normals=None, texcoords=None, colors=None,
                  radius=None) -> None:
        """notes another mesh - the whole of it - for shape `index` (current id), applied at update_shapes()"""
        pend = self._begin_shape_change("set_shape")
        index = int(index)
        if not 0 <= index < self.count("shapes"):
            raise VptError(f"set_shape: shape {index} out of range")
        if index in pend.remove:
            raise VptError(f"set_shape: shape {index} is also removed")
        pend.set[index] = self._check_mesh("set_shape", mesh(positions, triangles, quads, points, lines, normals, texcoords, colors, radius))

    def remove_shapes(self, ids) -> None:
        """notes shapes (current ids) to erase at update_shapes(): the survivors keep their order, the ids close up and the instances'
        shape ids follow.  No instance may name a removed shape: remove or re-point its instances first (update_instances)."""
        pend = self._begin_shape_change("remove_shapes")
        ids = [int(i) for i in ids]
        for i in ids:
            if not 0 <= i < self.count("shapes"):
                raise VptError(f"remove_shapes: shape {i} out of range")
            if i in pend.set:
                raise VptError(f"remove_shapes: shape {i} is also set")
        if len(set(ids)) != len(ids) or set(ids) & set(pend.remove):
            raise VptError("remove_shapes: an id is repeated")
        named = {self.instance_ids(i)[0] for i in range(self.count("instances"))}
        if named & set(ids):
            raise VptError(f"remove_shapes: shapes {sorted(named & set(ids))} are still named by instances")
        pend.remove = pend.remove + tuple(ids)

    def update_shapes(self) -> ShapeEdit:
        """edit_shapes of the host library over what add_shape / set_shape / remove_shapes noted since the last call: replace / erase /
        push_back on the scene's shapes, the instances' shape ids renumbered, make_bvh of the new shapes (the scene BVH too when a shape
        was replaced), make_lights; desc / stats() describe the edited scene afterwards.  Returns the ShapeEdit for
        DeviceScene.update_shapes."""
        if getattr(self, "_edit", None) is not None and (self._edit.instances or self._edit.shapes):
            raise VptError("update_shapes: hand the pending edit out with update_bvh() first")
        self._no_pending_instances_only("update_shapes")
        edit, self._shape_edit = (self._shape_edit if getattr(self, "_shape_edit", None) is not None else ShapeEdit()), None
        if edit.empty():
            return edit
        abi, keep = edit.to_abi()
        err = C.create_string_buffer(512)
        if host.vpth_scene_edit_shapes(self.handle, abi.remove_ids, abi.num_remove, abi.set_ids, abi.set, abi.num_set, abi.add, abi.num_add,
                                       err, len(err)) != 0:
            raise VptError(err.value.decode())
        del keep
        return edit

    def _no_pending_instances_only(self, what: str) -> None:
        if getattr(self, "_inst_edit", None) is not None and not self._inst_edit.empty():
            raise VptError(f"{what}: hand the pending instance changes out with update_instances() first")

    # -- environments and textures (the host side of vpt_scene_update_textures): the setters change the scene and note the change in
    #    the pending TextureEdit; desc, lights() and stats() follow at update_textures(), which hands that edit out ----------------
    def environment(self, index: int) -> VptEnvironment:
        out = VptEnvironment()
        if host.vpth_scene_get_environment(self.handle, index, C.byref(out)) != 0:
            raise VptError(f"environment {index} out of range")
        return out

    def set_environment(self, index: int, emission=None, emission_tex=None) -> None:
        """emission (three floats) and / or emission_tex (-1: none) of an environment; its frame is set_environment_frame's"""
        env = self.environment(index)
        if emission is not None:
            env.emission[0], env.emission[1], env.emission[2] = [float(c) for c in emission]
        if emission_tex is not None:
            env.emission_tex = int(emission_tex)
        err = C.create_string_buffer(512)
        if host.vpth_scene_set_environment(self.handle, index, C.byref(env), err, len(err)) != 0:
            raise VptError(err.value.decode())
        self._pending_textures().environments[index] = self.environment(index)

    def texture(self, index: int):
        """(texels (h, w, 4) float32 or uint8, linear) of a texture (a copy)"""
        w, h, linear, is_float = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        if host.vpth_scene_get_texture(self.handle, index, C.byref(w), C.byref(h), C.byref(linear), C.byref(is_float), None, 0) != 0:
            raise VptError(f"texture {index} out of range")
        texels = np.zeros((h.value, w.value, 4), np.float32 if is_float.value else np.uint8)
        host.vpth_scene_get_texture(self.handle, index, C.byref(w), C.byref(h), C.byref(linear), C.byref(is_float), texels.ctypes.data, texels.nbytes)
        return texels, bool(linear.value)

    def set_texture(self, index: int, texels, linear=None) -> None:
        """all texels of a texture: an (h, w, 4) array, float32 or uint8 - any size, either format; linear None: as it was"""
        texels = np.ascontiguousarray(texels)
        if texels.ndim != 3 or texels.shape[2] != 4 or texels.dtype not in (np.float32, np.uint8):
            raise VptError("texels are (h, w, 4) float32 or uint8")
        if linear is None:
            linear = self.texture(index)[1]
        err = C.create_string_buffer(512)
        if host.vpth_scene_set_texture(self.handle, index, texels.shape[1], texels.shape[0], int(bool(linear)), int(texels.dtype == np.float32),
                                       texels.ctypes.data, err, len(err)) != 0:
            raise VptError(err.value.decode())
        self._pending_textures().textures[index] = (texels.copy(), bool(linear))

    def _pending_textures(self) -> TextureEdit:
        if getattr(self, "_texture_edit", None) is None:
            self._texture_edit = TextureEdit()
        return self._texture_edit

    def update_textures(self) -> TextureEdit:
        """make_lights of the scene as set_environment / set_texture left it: desc, lights() and stats() carry the edited textures,
        environments, light list and CDFs.  Returns the TextureEdit for DeviceScene.update_textures."""
        err = C.create_string_buffer(512)
        if host.vpth_scene_update_textures(self.handle, err, len(err)) != 0:
            raise VptError(err.value.decode())
        edit, self._texture_edit = self._pending_textures(), None
        for index in edit.environments:   # an entry carries the frame too: the one the scene holds now, not the one it held at the setter
            edit.environments[index] = self.environment(index)
        return edit

    # -- volumes, grid instances and SDFs (the host side of vpt_scene_update_volumes): the setters change the scene and note the change
    #    in the pending VolumeEdit; desc, lights() and stats() follow at update_volumes(), which hands that edit out -------------------
    def count_implicit(self, kind: str) -> int:
        """number of "volumes", "vol_instances" or "sdfs"""
        return host.vpth_scene_count_implicit(self.handle, {"volumes": 0, "vol_instances": 1, "sdfs": 2}[kind])

    def volume_instance(self, index: int) -> VptVolumeInstance:
        out = VptVolumeInstance()
        if host.vpth_scene_get_vol_instance(self.handle, index, C.byref(out)) != 0:
            raise VptError(f"volume instance {index} out of range")
        return out

    def set_volume_instance(self, index: int, frame=None, volume=None, material=None, scalef=None) -> None:
        """frame ((12,) float32: x, y, z, o), volume, material and / or scalef of a grid instance; None: as it was"""
        vi = self.volume_instance(index)
        if frame is not None:
            C.memmove(C.byref(vi.frame), np.ascontiguousarray(frame, np.float32).reshape(12).ctypes.data, 48)
        if volume is not None:
            vi.volume = int(volume)
        if material is not None:
            vi.material = int(material)
        if scalef is not None:
            vi.scalef = float(scalef)
        err = C.create_string_buffer(512)
        if host.vpth_scene_set_vol_instance(self.handle, index, C.byref(vi), err, len(err)) != 0:
            raise VptError(err.value.decode())
        self._pending_volumes().vol_instances[index] = self.volume_instance(index)

    def sdf(self, index: int) -> VptSdf:
        out = VptSdf()
        if host.vpth_scene_get_sdf(self.handle, index, C.byref(out)) != 0:
            raise VptError(f"sdf {index} out of range")
        return out

    def set_sdf(self, index: int, sdf: Optional[VptSdf] = None, frame=None, type=None, material=None, whd=None, p=None) -> None:
        """an analytic SDF: a whole VptSdf, or the named fields of the one the scene holds (type: an index into SDF_TYPES or its name)"""
        f = self.sdf(index) if sdf is None else sdf
        if frame is not None:
            C.memmove(C.byref(f.frame), np.ascontiguousarray(frame, np.float32).reshape(12).ctypes.data, 48)
        if type is not None:
            f.type = SDF_TYPES.index(type) if isinstance(type, str) else int(type)
        if material is not None:
            f.material = int(material)
        if whd is not None:
            f.whd[:] = [float(v) for v in whd]
        if p is not None:
            f.p[:] = ([float(v) for v in p] + [0.0] * 4)[:4]
        err = C.create_string_buffer(512)
        if host.vpth_scene_set_sdf(self.handle, index, C.byref(f), err, len(err)) != 0:
            raise VptError(err.value.decode())
        self._pending_volumes().sdfs[index] = self.sdf(index)

    def _write_volume(self, index: int, src: VolumeSource, voxels: np.ndarray) -> None:
        whd, lo, size = (np.array([int(v) for v in a], np.int32) for a in (src.whd, src.region_lo, src.region_whd))
        voxels = np.ascontiguousarray(voxels, np.float32)
        err = C.create_string_buffer(512)
        if host.vpth_scene_set_volume(self.handle, index, whd.ctypes.data, C.c_float(src.res), lo.ctypes.data, size.ctypes.data, int(src.mode),
                                      voxels.ctypes.data, err, len(err)) != 0:
            raise VptError(err.value.decode())

    def _note_volume(self, index: int, src: VolumeSource) -> None:
        if index in self._pending_volumes().volumes:
            raise VptError(f"volume {index} is already in the pending edit: hand it out with update_volumes() first")
        self._pending_volumes().volumes[index] = src

    def set_volume(self, index: int, voxels, res: Optional[float] = None, region=None, mode: int = VOXELS_REPLACE) -> None:
        """voxels of a volume, float32 of shape (d, h, w).  region None: all of them - any size (a new size moves the volume to fresh
        room on the device); region = (lo, whd), each (x, y, z): that box of the grid as it is, voxels of the box's shape.  mode
        VOXELS_UNION: (resident < incoming) ? resident : incoming, the reference's op_union.  res None: as it was."""
        self._run_bakes()
        voxels = np.ascontiguousarray(voxels, np.float32)
        if voxels.ndim != 3:
            raise VptError(f"expected (d, h, w) voxels, got {voxels.shape}")
        old, old_res = self.volume(index)
        whd = voxels.shape[::-1] if region is None else old.shape[::-1]
        lo, size = ((0, 0, 0), whd) if region is None else region
        src = VolumeSource(tuple(whd), old_res if res is None else float(res), tuple(lo), tuple(size), mode, voxels.copy())
        if voxels.shape != tuple(int(v) for v in src.region_whd)[::-1]:
            raise VptError(f"voxels of region {tuple(size)} have shape {tuple(size)[::-1]}, got {voxels.shape}")
        self._note_volume(index, src)
        try:
            self._write_volume(index, src, voxels)
        except VptError:
            del self._pending_volumes().volumes[index]   # refused: nothing was written, nothing is pending
            raise

    def bake_volume(self, index: int, positions, faces, whd=None, res: Optional[float] = None, origin=None, step=None, region=None,
                    mode: int = VOXELS_REPLACE) -> None:
        """a mesh ((n, 3) positions, triangles or quads) baked into volume `index` by the rule of vpt_bake_sdf - on the device, into
        the resident pool, at DeviceScene.update_volumes; the host copy runs bake_sdf_grid(device=None) only when it is read.  whd None:
        the volume's; origin / step None: the grid the renderer's lookup reads back in place with the volume at the origin of its
        instance (origin 0, step = res * W / (W - 1) per axis); region and mode as in set_volume."""
        self._run_bakes()
        old, old_res = self.volume(index)
        whd = tuple(int(v) for v in (old.shape[::-1] if whd is None else _whd3(whd)))
        res = old_res if res is None else float(res)
        if origin is None:
            origin = np.zeros(3, np.float32)
        if step is None:
            step = np.array([np.float32(res) * np.float32(w) / np.float32(max(1, w - 1)) for w in whd], np.float32)
        lo, size = ((0, 0, 0), whd) if region is None else region
        positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3).copy()
        src = VolumeSource(whd, res, tuple(lo), tuple(size), mode, None, (positions, bake_triangles(faces), np.asarray(origin, np.float32).copy(),
                                                                      np.asarray(step, np.float32).copy()))
        self._note_volume(index, src)
        self._lazy_bakes = getattr(self, "_lazy_bakes", []) + [(index, src)]

    def _run_bakes(self) -> None:
        """the host copy of the volumes bake_volume named: the host mirror of the bake, run when the copy is read"""
        todo, self._lazy_bakes = getattr(self, "_lazy_bakes", []), []
        for index, src in todo:
            positions, triangles, origin, step = src.bake
            grid, _ = bake_sdf_grid(positions, triangles, src.whd, origin, step, device=None)
            lo, size = src.region_lo, src.region_whd
            box = grid[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]]
            self._write_volume(index, src, box)
        if todo:
            err = C.create_string_buffer(512)
            if host.vpth_scene_update_volumes(self.handle, err, len(err)) != 0:
                raise VptError(err.value.decode())

    def _pending_volumes(self) -> VolumeEdit:
        if getattr(self, "_volume_edit", None) is None:
            self._volume_edit = VolumeEdit()
        return self._volume_edit

    def update_volumes(self) -> VolumeEdit:
        """make_lights of the scene as set_volume_instance / set_sdf / set_volume / bake_volume left it: desc, lights() and stats() carry
        the edited volumes, instances, SDFs, light list and CDFs.  Returns the VolumeEdit for DeviceScene.update_volumes."""
        err = C.create_string_buffer(512)
        if host.vpth_scene_update_volumes(self.handle, err, len(err)) != 0:
            raise VptError(err.value.decode())
        edit, self._volume_edit = self._pending_volumes(), None
        return edit

    def lights(self):
        """(light list as a LIGHT array, CDF pool as float32) of the descriptor (copies)"""
        d = VptSceneDescLights.from_address(self.desc)
        grab = lambda ptr, n, dtype: np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (n * dtype.itemsize,)).view(dtype).copy() if n else np.zeros(0, dtype)
        return grab(d.lights, d.num_lights, LIGHT), grab(d.light_cdf, d.num_light_cdf, np.dtype(np.float32))

    def bvh_nodes(self):
        """(scene nodes, pooled shape nodes) of the descriptor as BVH_NODE arrays (copies)"""
        d = VptSceneDescBvh.from_address(self.desc + VptSceneDescBvh.OFFSET)
        grab = lambda ptr, n: np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (n * 32,)).view(BVH_NODE).copy() if n else np.zeros(0, BVH_NODE)
        return grab(d.scene_bvh_nodes, d.num_scene_bvh_nodes), grab(d.shape_bvh_nodes, d.num_shape_bvh_nodes)

    def bvh_prims(self):
        """(scene primitive order, pooled shape primitive orders) of the descriptor as int32 arrays (copies)"""
        d = VptSceneDescBvh.from_address(self.desc + VptSceneDescBvh.OFFSET)
        grab = lambda ptr, n: np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int32)), (n,)).copy() if n else np.zeros(0, np.int32)
        return grab(d.scene_bvh_prims, d.num_scene_bvh_prims), grab(d.shape_bvh_prims, d.num_shape_bvh_prims)

    def make_state(self, params: PathtraceParams) -> PathtraceState:
        """make_state, yocto_pathtrace.cpp:960-980"""
        w, h = C.c_int(), C.c_int()
        if host.vpth_state_size(self.handle, params.camera, params.resolution, C.byref(w), C.byref(h)) != 0:
            raise VptError("camera index out of range")
        st = PathtraceState(w.value, h.value, 0, np.zeros((h.value, w.value, 4), np.float32),
                            np.zeros((h.value, w.value), np.int32), np.zeros((h.value, w.value, 2), np.uint64))
        if host.vpth_make_state(self.handle, params.camera, params.resolution, st.image.ctypes.data,
                                st.hits.ctypes.data, st.rngs.ctypes.data) != 0:
            raise VptError("make_state failed")
        return st

    def close(self) -> None:
        if getattr(self, "handle", None) and host is not None:   # at interpreter shutdown the module globals may be gone
            host.vpth_scene_free(self.handle)
        self.handle = None

    def __del__(self):
        self.close()


class DeviceScene:
    """vpt_scene: the scene resident in one GPU's HBM."""

    def __init__(self, scene: HostScene, device: int = 0):
        self.host_scene = scene  # keep the flattened arrays alive until the upload finished
        out = _p()
        _check(hip.vpt_scene_create_curves(scene.desc, scene.curves, device, C.byref(out)), "vpt_scene_create")
        self.handle = out
        self.device = device

    # -- the drop-in for pathtrace_samples(): host state in, host state out ---------------------
    def pathtrace_samples(self, state: PathtraceState, params: PathtraceParams, count: int = 1) -> None:
        abi = params.to_abi()
        samples = C.c_int(state.samples)
        for a in (state.image, state.hits, state.rngs):
            assert a.flags["C_CONTIGUOUS"]
        _check(hip.vpt_render(self.handle, C.byref(abi), count, state.width, state.height, state.image.ctypes.data,
                              state.hits.ctypes.data, state.rngs.ctypes.data, C.byref(samples)), "vpt_render")
        state.samples = samples.value

    def pathtrace_adaptive(self, state: PathtraceState, params: PathtraceParams, threshold: float, min_samples: int = 16,
                           step: int = 32):
        """adaptive sampling (vpt_render_adaptive, include/vpt.h): every pixel renders in rounds of `step` samples until the relative
        standard error of its mean luminance is within `threshold` (0: never stops early), never below `min_samples` and at most
        params.samples; state.hits must be equal on entry.  state.samples becomes max(hits).  Returns (rounds, samples taken)."""
        abi, ad = params.to_abi(), VptAdaptive(threshold, min_samples, step)
        samples, rendered = C.c_int(state.samples), C.c_int64(0)
        for a in (state.image, state.hits, state.rngs):
            assert a.flags["C_CONTIGUOUS"]
        entry = int(state.hits.flat[0]) if state.hits.size else 0
        _check(hip.vpt_render_adaptive(self.handle, C.byref(abi), C.byref(ad), state.width, state.height, state.image.ctypes.data,
                                       state.hits.ctypes.data, state.rngs.ctypes.data, C.byref(samples), C.byref(rendered)),
               "vpt_render_adaptive")
        state.samples = samples.value
        # the pixel that rendered longest was in every round; each of its rounds but the last took `step` samples
        return -(-max(0, state.samples - entry) // step), rendered.value

    # -- device-resident state (pointers are raw device addresses, e.g. torch.Tensor.data_ptr()) ----
    def render_device_adaptive(self, params: PathtraceParams, layout: VptLayout, d_image: int, d_hits: int, d_rng: int, threshold: float,
                               min_samples: int = 16, step: int = 32, stream: int = 0):
        """vpt_render_device_adaptive on this rank's tile-major state: returns (rounds, samples taken)"""
        abi, ad = params.to_abi(), VptAdaptive(threshold, min_samples, step)
        rounds, rendered = C.c_int(0), C.c_int64(0)
        _check(hip.vpt_render_device_adaptive(self.handle, C.byref(abi), C.byref(ad), C.byref(layout), d_image, d_hits, d_rng, stream,
                                              C.byref(rounds), C.byref(rendered)), "vpt_render_device_adaptive")
        return rounds.value, rendered.value

    def adaptive_run(self, params: PathtraceParams, layout: VptLayout, d_image: int, d_hits: int, d_rng: int, threshold: float,
                     min_samples: int = 16, step: int = 32, stream: int = 0) -> "AdaptiveRun":
        """vpt_adaptive_run_create: render_device_adaptive as an object whose rounds() can stop and go on.  Any edit or rebuild of this
        scene ends the run's validity: close it first."""
        return AdaptiveRun(self, params, layout, d_image, d_hits, d_rng, threshold, min_samples, step, stream)

    def render_device(self, params: PathtraceParams, layout: VptLayout, nsamples: int, d_image: int, d_hits: int,
                      d_rng: int, stream: int = 0) -> None:
        abi = params.to_abi()
        _check(hip.vpt_render_device(self.handle, C.byref(abi), C.byref(layout), nsamples, d_image, d_hits, d_rng,
                                     stream), "vpt_render_device")

    def render_aov_device(self, params: PathtraceParams, layout: VptLayout, nsamples: int, planes: dict, d_hits: int, d_rng: int,
                          stream: int = 0) -> None:
        """vpt_render_aov_device on this rank's tile-major slots: `planes` maps names of AOV_PLANES to raw device pointers"""
        unknown = set(planes) - set(AOV_PLANES)
        if unknown:
            raise VptError(f"unknown AOV plane {sorted(unknown)[0]!r}: expected one of {AOV_PLANES}")
        abi, pl = params.to_abi(), VptAovPlanes(**{k: v for k, v in planes.items() if v})
        _check(hip.vpt_render_aov_device(self.handle, C.byref(abi), C.byref(layout), nsamples, C.byref(pl), d_hits, d_rng, stream),
               "vpt_render_aov_device")

    def render_aovs(self, state: PathtraceState, params: PathtraceParams, count: int = 1, planes=AOV_PLANES, into: Optional[dict] = None) -> dict:
        """the first-hit pass (vpt_render_aov, include/vpt.h) over the hits / rngs of `state` (its image is left alone): `count` more
        samples, at most params.samples in all, traced once for every plane named in `planes`.  Returns {name: array}: the sums
        normal / albedo / texcoord / depth as (h, w, 4) float32 - divide by state.samples, as get_render does - and ids (h, w, 2) int32,
        uvt (h, w, 3) float32 of the state's first sample.  `into`: the dict an earlier call returned, to go on from (batching is exact)."""
        shapes = {"ids": ((2,), np.int32), "uvt": ((3,), np.float32)}
        out = {}
        for name in planes:
            if name not in AOV_PLANES:
                raise VptError(f"unknown AOV plane {name!r}: expected one of {AOV_PLANES}")
            tail, dtype = shapes.get(name, ((4,), np.float32))
            shape = (state.height, state.width) + tail
            a = into.get(name) if into else None
            if a is None:
                a = np.zeros(shape, dtype)
            elif a.shape != shape or a.dtype != dtype or not a.flags["C_CONTIGUOUS"]:
                raise VptError(f"plane {name!r}: expected a contiguous {np.dtype(dtype).name} array of shape {shape}")
            out[name] = a
        for a in (state.hits, state.rngs):
            assert a.flags["C_CONTIGUOUS"]
        abi, pl, samples = params.to_abi(), VptAovPlanes(**{k: a.ctypes.data for k, a in out.items()}), C.c_int(state.samples)
        _check(hip.vpt_render_aov(self.handle, C.byref(abi), count, state.width, state.height, C.byref(pl), state.hits.ctypes.data,
                                  state.rngs.ctypes.data, C.byref(samples)), "vpt_render_aov")
        state.samples = samples.value
        return out

    def _edit(self, name: str, edit, *extra) -> None:
        """the C-ABI's edit entry point `name` on this handle, the arrays `edit` points into kept alive across the call"""
        abi, keep = edit.to_abi()
        _check(getattr(hip, name)(self.handle, C.byref(abi), *extra), name)
        del keep

    def update(self, edit: SceneEdit) -> None:
        """vpt_scene_update (include/vpt.h): the edit applied to the resident scene, BVHs refitted on the device.  Afterwards the
        handle renders the bits of a DeviceScene made from the host scene after the same edit and update_bvh()."""
        self._edit("vpt_scene_update", edit)

    def update_lights(self, edit: SceneEdit) -> None:
        """vpt_scene_update_lights (include/vpt.h): update() for an edit that may switch a material's emission between zero and non-zero
        or move the vertices of an emitter; the light tables are rebuilt on the device.  Afterwards the handle renders the bits of a
        DeviceScene made from the host scene after the same edit and update_lights()."""
        self._edit("vpt_scene_update_lights", edit)

    def update_textures(self, edit: TextureEdit) -> None:
        """vpt_scene_update_textures (include/vpt.h): environments' emission and texture, and textures' texels; an environment's CDF
        is rebuilt on the device from the texels.  Afterwards the handle renders the bits of a DeviceScene made from the host scene
        after the same edit and update_textures()."""
        self._edit("vpt_scene_update_textures", edit)

    def update_volumes(self, edit: VolumeEdit) -> None:
        """vpt_scene_update_volumes (include/vpt.h): grid instances, SDFs and volumes' voxels, from the host or baked on the device into
        the resident pool.  Afterwards the handle renders the bits of a DeviceScene made from the host scene after the same edit and
        update_volumes()."""
        self._edit("vpt_scene_update_volumes", edit)

    def get_volumes(self):
        """(volumes, vol_instances, sdfs) as the device holds them, ctypes arrays of VptVolume, VptVolumeInstance, VptSdf
        (vpt_scene_get_volumes); a volume's offset is the resident pool's"""
        nv, ni, ns = (self.host_scene.count_implicit(k) for k in ("volumes", "vol_instances", "sdfs"))
        vols, insts, sdfs = (VptVolume * max(1, nv))(), (VptVolumeInstance * max(1, ni))(), (VptSdf * max(1, ns))()
        _check(hip.vpt_scene_get_volumes(self.handle, C.cast(vols, _p), nv, C.cast(insts, _p), ni, C.cast(sdfs, _p), ns), "vpt_scene_get_volumes")
        return list(vols)[:nv], list(insts)[:ni], list(sdfs)[:ns]

    def get_voxels(self, index: int) -> np.ndarray:
        """the voxels of a volume as the device holds them, float32 of shape (d, h, w) (vpt_scene_get_voxels)"""
        vols, _, _ = self.get_volumes()
        if not 0 <= index < len(vols):
            raise VptError(f"volume {index} out of range")
        w, h, d = vols[index].whd
        out = np.zeros((d, h, w), np.float32)
        _check(hip.vpt_scene_get_voxels(self.handle, index, out.ctypes.data, out.size), "vpt_scene_get_voxels")
        return out

    def get_lights(self):
        """(light list as a LIGHT array, CDF pool as float32) as the device holds them (vpt_scene_get_lights)"""
        n, m = C.c_int(0), C.c_int64(0)
        _check(hip.vpt_scene_get_lights(self.handle, None, 0, C.byref(n), None, 0, C.byref(m)), "vpt_scene_get_lights")
        lights, cdf = np.zeros(n.value, LIGHT), np.zeros(m.value, np.float32)
        _check(hip.vpt_scene_get_lights(self.handle, lights.ctypes.data, len(lights), None, cdf.ctypes.data, len(cdf), None), "vpt_scene_get_lights")
        return lights, cdf

    def get_media(self):
        """the medium records of the device, float32 [materials, 12] (vpt_scene_get_media): density, scattering, emission, scanisotropy, 0, 0"""
        n = C.c_int(0)
        _check(hip.vpt_scene_get_media(self.handle, None, 0, C.byref(n), None), "vpt_scene_get_media")
        out = np.zeros((n.value, 12), np.float32)
        _check(hip.vpt_scene_get_media(self.handle, out.ctypes.data, len(out), None, None), "vpt_scene_get_media")
        return out

    def media_vary(self) -> bool:
        """the scene's media vary over the surface (vpt_scene_get_media): it renders with K1's general instance"""
        v = C.c_int(0)
        _check(hip.vpt_scene_get_media(self.handle, None, 0, None, C.byref(v)), "vpt_scene_get_media")
        return bool(v.value)

    def light_tables_hash(self):
        """FNV-1a of the six light tables on the device (vpt_scene_light_tables_hash): lights, cdf, records, prims, index + pool, guide"""
        out = np.zeros(6, np.uint64)
        _check(hip.vpt_scene_light_tables_hash(self.handle, out.ctypes.data), "vpt_scene_light_tables_hash")
        return tuple(int(x) for x in out)

    def rebuild_bvh(self, rebuild: "BvhRebuild") -> None:
        """vpt_scene_rebuild_bvh (include/vpt.h): the named shapes' BVHs and the scene BVH built anew on the device from what is
        resident.  Afterwards the handle renders the bits of a DeviceScene made from the host scene after the same
        HostScene.rebuild_bvh()."""
        self._edit("vpt_scene_rebuild_bvh_quality", rebuild, rebuild.quality)

    def update_instances(self, edit: InstanceEdit) -> None:
        """vpt_scene_update_instances (include/vpt.h): instances re-pointed, removed and added on the device; the scene BVH and the
        lights follow.  Afterwards the handle renders the bits of a DeviceScene made from the host scene after the same
        HostScene.update_instances()."""
        self._edit("vpt_scene_update_instances", edit)

    def update_shapes(self, edit: ShapeEdit) -> None:
        """vpt_scene_update_shapes (include/vpt.h): shapes replaced, removed and added on the device; pools, BVHs, instances and lights
        follow.  Afterwards the handle renders the bits of a DeviceScene made from the host scene after the same
        HostScene.update_shapes()."""
        self._edit("vpt_scene_update_shapes", edit)

    def shape_tables_hash(self):
        """FNV-1a of the eight groups of tables laid out in shape order (vpt_scene_shape_tables_hash): shapes, vertex pools, elems,
        leaf_prims, leaf_attrs, the compact records (0: none), shape nodes, shape quad nodes"""
        out = np.zeros(8, np.uint64)
        _check(hip.vpt_scene_shape_tables_hash(self.handle, out.ctypes.data), "vpt_scene_shape_tables_hash")
        return tuple(int(x) for x in out)

    def get_shape_counts(self):
        """(shapes, pooled elements, pooled vertices) as the device holds them (vpt_scene_get_shape_counts)"""
        a, b, c = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        _check(hip.vpt_scene_get_shape_counts(self.handle, C.byref(a), C.byref(b), C.byref(c)), "vpt_scene_get_shape_counts")
        return a.value, b.value, c.value

    def get_instances(self) -> np.ndarray:
        """the instances as the device holds them, an INSTANCE array: forward frame, shape, material (vpt_scene_get_instances)"""
        n = C.c_int(0)
        _check(hip.vpt_scene_get_instances(self.handle, None, 0, C.byref(n)), "vpt_scene_get_instances")
        out = np.zeros(n.value, INSTANCE)
        _check(hip.vpt_scene_get_instances(self.handle, out.ctypes.data if len(out) else None, len(out), None), "vpt_scene_get_instances")
        return out

    def instance_tables_hash(self):
        """FNV-1a of the four tables keyed by instance id (vpt_scene_instance_tables_hash): instances, enter records, slots, scene prims"""
        out = np.zeros(4, np.uint64)
        _check(hip.vpt_scene_instance_tables_hash(self.handle, out.ctypes.data), "vpt_scene_instance_tables_hash")
        return tuple(int(x) for x in out)

    def get_bvh_counts(self):
        """(scene nodes, pooled shape nodes, first node of every shape as int64) as the device holds them (vpt_scene_get_bvh_counts)"""
        a, b = C.c_int32(0), C.c_int64(0)
        shapes = self.get_shape_counts()[0]   # the device's count: update_shapes changes it
        offsets = np.zeros(max(1, shapes), np.int64)
        _check(hip.vpt_scene_get_bvh_counts(self.handle, C.byref(a), C.byref(b), offsets.ctypes.data), "vpt_scene_get_bvh_counts")
        return a.value, b.value, offsets[:shapes]

    def get_bvh(self):
        """(scene nodes, pooled shape nodes) as the device holds them, BVH_NODE arrays at the current counts (vpt_scene_get_bvh)"""
        na, nb, _ = self.get_bvh_counts()
        a, b = np.zeros(na, BVH_NODE), np.zeros(nb, BVH_NODE)
        _check(hip.vpt_scene_get_bvh(self.handle, a.ctypes.data, len(a), b.ctypes.data, len(b)), "vpt_scene_get_bvh")
        return a, b

    def get_bvh_prims(self):
        """(scene primitive order, pooled shape primitive orders) as the device holds them, int32 (vpt_scene_get_bvh_prims)"""
        n = C.c_int(0)                                 # the counts are the device's: update_instances and update_shapes change them
        _check(hip.vpt_scene_get_instances(self.handle, None, 0, C.byref(n)), "vpt_scene_get_instances")
        a, b = np.zeros(n.value, np.int32), np.zeros(self.get_shape_counts()[1], np.int32)
        _check(hip.vpt_scene_get_bvh_prims(self.handle, a.ctypes.data, len(a), b.ctypes.data, len(b)), "vpt_scene_get_bvh_prims")
        return a, b

    def update_stats(self):
        """(kernel launches, payload bytes, device ms of the refit) of the last update"""
        n, b, ms = C.c_int(0), C.c_int64(0), C.c_float(0)
        _check(hip.vpt_scene_update_stats(self.handle, C.byref(n), C.byref(b), C.byref(ms)), "vpt_scene_update_stats")
        return n.value, b.value, ms.value

    def intersect(self, rays: np.ndarray, instance: int = -1):
        """intersect_bvh for an (n, 6) float32 array of rays {o, d}: returns (ids (n, 2) int32, uvt (n, 3) float32)"""
        rays = np.ascontiguousarray(rays, np.float32)
        n = rays.shape[0]
        ids, uvt = np.zeros((n, 2), np.int32), np.zeros((n, 3), np.float32)
        _check(hip.vpt_intersect(self.handle, n, rays.ctypes.data, instance, ids.ctypes.data, uvt.ctypes.data), "vpt_intersect")
        return ids, uvt

    def kat(self, op: int, records: np.ndarray, iparam: int = 0) -> np.ndarray:
        """vpt_kat (include/vpt_kat.h): run known-answer-test op `op` on an (n, in_stride) float32 array"""
        si, so = C.c_int(), C.c_int()
        _check(hip.vpt_kat_strides(op, C.byref(si), C.byref(so)), "vpt_kat_strides")
        records = np.ascontiguousarray(records, np.float32)
        if records.ndim != 2 or records.shape[1] != si.value:
            raise VptError(f"KAT op {op} takes records of {si.value} floats")
        out = np.zeros((records.shape[0], so.value), np.float32)
        _check(hip.vpt_kat(self.handle, op, iparam, records.shape[0], records.ctypes.data, out.ctypes.data), "vpt_kat")
        return out

    def spheretrace(self, rays: np.ndarray, sdf: int = -1, maxiter: int = 450):
        """vpt_spheretrace for an (n, 6) float32 array of rays {o, d}: (ids (n, 3) int32 {hit, instance, sdf}, t (n,) float32)"""
        rays = np.ascontiguousarray(rays, np.float32)
        n = rays.shape[0]
        ids, t = np.zeros((n, 3), np.int32), np.zeros((n,), np.float32)
        _check(hip.vpt_spheretrace(self.handle, n, rays.ctypes.data, sdf, maxiter, ids.ctypes.data, t.ctypes.data), "vpt_spheretrace")
        return ids, t

    def selftest_light_cdf(self, light: int, n: int = 1 << 20):
        """(mismatches, indexed) of the light-CDF search structure against the plain binary search (include/vpt.h)"""
        bad, indexed = C.c_ulonglong(0), C.c_int(0)
        _check(hip.vpt_selftest_light_cdf(self.handle, light, n, C.byref(bad), C.byref(indexed)), "vpt_selftest_light_cdf")
        return bad.value, indexed.value

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        _check(hip.vpt_last_kernel_ms(self.handle, C.byref(ms)), "vpt_last_kernel_ms")
        return ms.value

    def record_bytes(self):
        """(leaf record bytes, attribute record bytes) per primitive: (64, 96), or (48, 64) on a scene of triangles (include/vpt.h)"""
        a, b = C.c_int(0), C.c_int(0)
        _check(hip.vpt_scene_record_bytes(self.handle, C.byref(a), C.byref(b)), "vpt_scene_record_bytes")
        return a.value, b.value

    def last_wave_costs(self) -> np.ndarray:
        """ticks (100 MHz) every wave of the last launch ran, indexed by wave (include/vpt.h)"""
        n = C.c_int(0)
        _check(hip.vpt_last_wave_costs(self.handle, None, 0, C.byref(n)), "vpt_last_wave_costs")
        out = np.zeros(n.value, np.uint32)
        _check(hip.vpt_last_wave_costs(self.handle, out.ctypes.data, n.value, C.byref(n)), "vpt_last_wave_costs")
        return out

    def close(self) -> None:
        if getattr(self, "handle", None) and hip is not None:   # see HostScene.close
            hip.vpt_scene_destroy(self.handle)
        self.handle = None

    def __del__(self):
        self.close()


class AdaptiveRun:
    """vpt_adaptive_run (include/vpt.h): the round loop of an adaptive render on device-resident tile-major state, resumable.  The
    pointers are raw device addresses and stay the caller's."""

    def __init__(self, dev: "DeviceScene", params: PathtraceParams, layout: VptLayout, d_image: int, d_hits: int, d_rng: int,
                 threshold: float, min_samples: int = 16, step: int = 32, stream: int = 0):
        self.dev, self.handle = dev, None
        abi, ad, out = params.to_abi(), VptAdaptive(threshold, min_samples, step), _p()
        _check(hip.vpt_adaptive_run_create(dev.handle, C.byref(abi), C.byref(ad), C.byref(layout), d_image, d_hits, d_rng, stream,
                                           C.byref(out)), "vpt_adaptive_run_create")
        self.handle = out

    def rounds(self, max_rounds: int = 2**31 - 1):
        """up to max_rounds more rounds: (rounds run, samples taken, pixels still rendering); (0, 0, active) when there is nothing to do"""
        done, rendered, active = C.c_int(0), C.c_int64(0), C.c_int(0)
        _check(hip.vpt_adaptive_run_rounds(self.handle, min(max_rounds, 2**31 - 1), C.byref(done), C.byref(rendered), C.byref(active)),
               "vpt_adaptive_run_rounds")
        return done.value, rendered.value, active.value

    def progress(self):
        """(rounds, samples taken, pixels still rendering, hits of the pixels that rendered every round) so far"""
        n, rendered, active, hits = C.c_int(0), C.c_int64(0), C.c_int(0), C.c_int(0)
        _check(hip.vpt_adaptive_run_progress(self.handle, C.byref(n), C.byref(rendered), C.byref(active), C.byref(hits)),
               "vpt_adaptive_run_progress")
        return n.value, rendered.value, active.value, hits.value

    def noise_device(self, d_se2: int, d_hits: Optional[int] = None, stream: int = 0) -> None:
        """the squared standard error (and the hits) as row-major planes on the device"""
        _check(hip.vpt_adaptive_run_noise_device(self.handle, d_se2, d_hits, stream), "vpt_adaptive_run_noise_device")

    def stats_device(self, d_mean: int, d_m2: int, stream: int = 0) -> None:
        _check(hip.vpt_adaptive_run_stats_device(self.handle, d_mean, d_m2, stream), "vpt_adaptive_run_stats_device")

    def close(self) -> None:
        if getattr(self, "handle", None) and hip is not None:
            hip.vpt_adaptive_run_destroy(self.handle)
        self.handle = None

    def __del__(self):
        self.close()


def box3_device(width: int, height: int, d_in: int, d_out: int, stream: int = 0) -> None:
    """vpt_box3_device: the denoiser's box3 of a row-major float plane"""
    _check(hip.vpt_box3_device(width, height, d_in, d_out, stream), "vpt_box3_device")


class MultiDeviceScene:
    """vpt_multi: the scene on several GPUs of this process, tiles dealt round-robin (include/vpt.h)."""

    def __init__(self, scene: HostScene, devices):
        self.host_scene = scene
        devs = (C.c_int * len(devices))(*devices)
        out = _p()
        _check(hip.vpt_multi_create_curves(scene.desc, scene.curves, devs, len(devices), C.byref(out)), "vpt_multi_create")
        self.handle = out

    def _edit(self, name: str, edit, *extra) -> None:
        """the C-ABI's edit entry point `name` on this handle, the arrays `edit` points into kept alive across the call"""
        abi, keep = edit.to_abi()
        _check(getattr(hip, name)(self.handle, C.byref(abi), *extra), name)
        del keep

    def update(self, edit: SceneEdit) -> None:
        """vpt_multi_update: the same edit on every device; the resident tile state is left as it is"""
        self._edit("vpt_multi_update", edit)

    def update_lights(self, edit: SceneEdit) -> None:
        """vpt_multi_update_lights: DeviceScene.update_lights with the same edit on every device"""
        self._edit("vpt_multi_update_lights", edit)

    def update_textures(self, edit: TextureEdit) -> None:
        """vpt_multi_update_textures: DeviceScene.update_textures with the same edit on every device"""
        self._edit("vpt_multi_update_textures", edit)

    def update_volumes(self, edit: VolumeEdit) -> None:
        """vpt_multi_update_volumes: DeviceScene.update_volumes with the same edit on every device"""
        self._edit("vpt_multi_update_volumes", edit)

    def rebuild_bvh(self, rebuild: "BvhRebuild") -> None:
        """vpt_multi_rebuild_bvh: DeviceScene.rebuild_bvh on every device (each builds its own trees: equal by construction)"""
        self._edit("vpt_multi_rebuild_bvh_quality", rebuild, rebuild.quality)

    def update_instances(self, edit: InstanceEdit) -> None:
        """vpt_multi_update_instances: DeviceScene.update_instances with the same edit on every device"""
        self._edit("vpt_multi_update_instances", edit)

    def update_shapes(self, edit: ShapeEdit) -> None:
        """vpt_multi_update_shapes: DeviceScene.update_shapes with the same edit on every device"""
        self._edit("vpt_multi_update_shapes", edit)

    def pathtrace_samples(self, state: PathtraceState, params: PathtraceParams, count: int = 1) -> None:
        """host state in, host state out (the contract of vpt_render); a device's part of the upload is skipped only while `state`'s
        arrays are the very ones the last call downloaded into and their checksum over every word is unchanged (include/vpt.h)"""
        abi = params.to_abi()
        samples = C.c_int(state.samples)
        _check(hip.vpt_multi_render(self.handle, C.byref(abi), count, state.width, state.height, state.image.ctypes.data,
                                    state.hits.ctypes.data, state.rngs.ctypes.data, C.byref(samples)), "vpt_multi_render")
        state.samples = samples.value

    # -- resident state: upload once, render in batches without transfers, download on demand ---------
    def set_state(self, state: PathtraceState) -> None:
        _check(hip.vpt_multi_set_state(self.handle, state.width, state.height, state.image.ctypes.data, state.hits.ctypes.data,
                                       state.rngs.ctypes.data, state.samples), "vpt_multi_set_state")
        self._resident = (state.width, state.height, state.samples)

    def render_resident(self, params: PathtraceParams, count: int = 1) -> int:
        """`count` passes on the state the devices hold; returns the sample count reached"""
        abi = params.to_abi()
        w, h, n = self._resident
        samples = C.c_int(n)
        _check(hip.vpt_multi_render(self.handle, C.byref(abi), count, w, h, None, None, None, C.byref(samples)), "vpt_multi_render")
        self._resident = (w, h, samples.value)
        return samples.value

    def get_state(self, state: PathtraceState) -> None:
        samples = C.c_int(0)
        _check(hip.vpt_multi_get_state(self.handle, state.image.ctypes.data, state.hits.ctypes.data, state.rngs.ctypes.data,
                                       C.byref(samples)), "vpt_multi_get_state")
        state.samples = samples.value

    def transport(self) -> str:
        return hip.vpt_multi_transport(self.handle).decode()

    def uploaded_parts(self) -> int:
        """devices whose part of the caller's arrays the last pathtrace_samples call uploaded (include/vpt.h: the residency rule)"""
        return hip.vpt_multi_uploaded_parts(self.handle)

    def get_render(self, width: int, height: int) -> np.ndarray:
        out = np.zeros((height, width, 4), np.float32)
        _check(hip.vpt_multi_get_render(self.handle, out.ctypes.data), "vpt_multi_get_render")
        return out

    def close(self) -> None:
        if getattr(self, "handle", None) and hip is not None:
            hip.vpt_multi_destroy(self.handle)
        self.handle = None

    def __del__(self):
        self.close()


def layout_slots(layout: VptLayout) -> int:
    n = hip.vpt_layout_slots(C.byref(layout))
    if n < 0:
        raise VptError(hip.vpt_last_error().decode())
    return n


def state_upload(layout: VptLayout, state: PathtraceState, d_image: int, d_hits: int, d_rng: int, stream: int = 0):
    _check(hip.vpt_state_upload(C.byref(layout), state.image.ctypes.data, state.hits.ctypes.data,
                                state.rngs.ctypes.data, d_image, d_hits, d_rng, stream), "vpt_state_upload")


def state_download(layout: VptLayout, d_image: int, d_hits: int, d_rng: int, state: PathtraceState, stream: int = 0):
    _check(hip.vpt_state_download(C.byref(layout), d_image, d_hits, d_rng, state.image.ctypes.data,
                                  state.hits.ctypes.data, state.rngs.ctypes.data, stream), "vpt_state_download")


def resolve_device(layout: VptLayout, d_tiles_all: int, samples: int, d_rows: int, stream: int = 0):
    _check(hip.vpt_resolve_device(C.byref(layout), d_tiles_all, samples, d_rows, stream), "vpt_resolve_device")


def resolve_hits_device(layout: VptLayout, d_tiles_all: int, d_hits_all: int, d_rows: int, stream: int = 0):
    """get_render with each pixel's own sample count on the device (vpt_resolve_hits_device): row-major float4"""
    _check(hip.vpt_resolve_hits_device(C.byref(layout), d_tiles_all, d_hits_all, d_rows, stream), "vpt_resolve_hits_device")


def resolve_srgb8_device(layout: VptLayout, d_tiles_all: int, samples: int, d_rgba8: int, stream: int = 0):
    """get_render + rgb_to_srgb + float_to_byte on the device (row-major RGBA8)"""
    _check(hip.vpt_resolve_srgb8_device(C.byref(layout), d_tiles_all, samples, d_rgba8, stream), "vpt_resolve_srgb8_device")


def resolve_ids_device(layout: VptLayout, d_ids_all: int, d_uvt_all: Optional[int], d_ids_rows: int, d_uvt_rows: Optional[int], stream: int = 0):
    """vpt_resolve_ids_device: the ids / uvt planes of all ranks, tile-major -> row-major (the uvt pair None together)"""
    _check(hip.vpt_resolve_ids_device(C.byref(layout), d_ids_all, d_uvt_all, d_ids_rows, d_uvt_rows, stream), "vpt_resolve_ids_device")


def get_render(state: PathtraceState) -> np.ndarray:
    """get_render, yocto_pathtrace.cpp:1105-1116: image * (1/samples) in float32"""
    return state.image * np.float32(np.float32(1.0) / np.float32(state.samples))


def get_render_hits(state: PathtraceState) -> np.ndarray:
    """get_render with each pixel's own sample count: image * float32(1 / hits), 0 where hits == 0 (after pathtrace_adaptive)"""
    hits = state.hits.astype(np.float32)
    with np.errstate(divide="ignore"):
        scale = np.where(state.hits > 0, np.float32(1.0) / hits, np.float32(0.0)).astype(np.float32)
    return np.where((state.hits > 0)[..., None], state.image * scale[..., None], np.float32(0.0)).astype(np.float32)


def _image4(a, shape=None) -> np.ndarray:
    a = np.ascontiguousarray(a, np.float32)
    if a.ndim != 3 or a.shape[2] != 4 or (shape is not None and a.shape != shape):
        raise VptError(f"expected a (height, width, 4) float32 image{'' if shape is None else ' of shape ' + str(shape)}, got {a.shape}")
    return a


def denoise_render(render: np.ndarray, albedo: Optional[np.ndarray] = None, normal: Optional[np.ndarray] = None,
                   variance: Optional[np.ndarray] = None, *, iterations: int = DENOISE_ITERATIONS,
                   sigma_luminance: float = DENOISE_SIGMA_LUMINANCE, sigma_normal: float = DENOISE_SIGMA_NORMAL,
                   sigma_albedo: float = DENOISE_SIGMA_ALBEDO, device: Optional[int] = None) -> np.ndarray:
    """denoise_render (include/vpt.h: the rule of vpt_denoise_params): the guided à-trous filter over an (h, w, 4) float32 resolved
    render.  albedo / normal: resolved renders of the `color` / `normal` (`implicit_normal`) shaders; variance: (h, w) float32 estimate
    of the variance of each pixel's mean luminance (None: the spatial seed).  device None: the host C++ mirror; else that GPU
    (vpt_denoise) - same bits.  The inputs are left unchanged; out[..., 3] == render[..., 3]."""
    render = _image4(render)
    h, w, _ = render.shape
    albedo = None if albedo is None else _image4(albedo, render.shape)
    normal = None if normal is None else _image4(normal, render.shape)
    if variance is not None:
        variance = np.ascontiguousarray(variance, np.float32)
        if variance.shape != (h, w):
            raise VptError(f"expected a variance of shape {(h, w)}, got {variance.shape}")
    out = np.zeros_like(render)
    err = C.create_string_buffer(512)
    ptr = lambda a: None if a is None else a.ctypes.data
    if host.vpth_denoise(w, h, render.ctypes.data, ptr(normal), ptr(albedo), ptr(variance), iterations, sigma_luminance, sigma_normal,
                         sigma_albedo, -1 if device is None else device, out.ctypes.data, err, len(err)) != 0:
        raise VptError(err.value.decode())
    return out


def half_variance(sum_a: np.ndarray, a: int, sum_n: np.ndarray, n: int, device: Optional[int] = None) -> np.ndarray:
    """the variance of each pixel's mean luminance from the radiance sums (PathtraceState.image) after the first `a` samples and
    after all `n` of one chain, 0 < a < n (include/vpt.h): (h, w) float32.  device None: host loops; else that GPU - same bits."""
    sum_a = _image4(sum_a)
    sum_n = _image4(sum_n, sum_a.shape)
    h, w, _ = sum_a.shape
    out = np.zeros((h, w), np.float32)
    err = C.create_string_buffer(512)
    if host.vpth_half_variance(w, h, sum_a.ctypes.data, a, sum_n.ctypes.data, n, -1 if device is None else device, out.ctypes.data,
                               err, len(err)) != 0:
        raise VptError(err.value.decode())
    return out


def pathtrace_guides(scene: HostScene, dev, params: PathtraceParams, samples: int = 16):
    """the two guide renders of denoise_render on `dev` (a DeviceScene or MultiDeviceScene of `scene`): (normal, albedo) as resolved
    (h, w, 4) float32 images - `samples` passes of the `normal` and the `color` shader over a fresh make_state; for the implicit
    shaders: `implicit_normal`, and albedo None"""
    implicit = params.shader in ("implicit", "implicit_normal")
    if not implicit and isinstance(dev, DeviceScene):  # both from one first-hit pass: the same rays traced once, the same bits
        p = PathtraceParams(params.camera, params.resolution, "normal", samples, params.bounces, params.noparallel, params.noimplicit_mis,
                            params.spheretrace_maxiter)
        st = scene.make_state(p)
        sums = dev.render_aovs(st, p, samples, ("normal", "albedo"))
        scale = np.float32(np.float32(1.0) / np.float32(st.samples))
        return sums["normal"] * scale, sums["albedo"] * scale

    def render(shader):
        p = PathtraceParams(params.camera, params.resolution, shader, samples, params.bounces, params.noparallel, params.noimplicit_mis,
                            params.spheretrace_maxiter)
        st = scene.make_state(p)
        dev.pathtrace_samples(st, p, samples)
        return get_render(st)

    return render("implicit_normal" if implicit else "normal"), None if implicit else render("color")


def denoise_scratch_bytes(width: int, height: int) -> int:
    n = hip.vpt_denoise_scratch_bytes(width, height)
    if n < 0:
        raise VptError(hip.vpt_last_error().decode())
    return n


def denoise_device(width: int, height: int, d_color: int, d_normal: Optional[int], d_albedo: Optional[int], d_variance: Optional[int],
                   d_out: int, d_scratch: int, *, iterations: int = DENOISE_ITERATIONS, sigma_luminance: float = DENOISE_SIGMA_LUMINANCE,
                   sigma_normal: float = DENOISE_SIGMA_NORMAL, sigma_albedo: float = DENOISE_SIGMA_ALBEDO, stream: int = 0) -> None:
    """vpt_denoise_device over raw device pointers (row-major float4 images, float variance; None: not given), asynchronous on
    `stream`; d_scratch holds denoise_scratch_bytes(width, height) bytes"""
    par = VptDenoise(iterations, sigma_luminance, sigma_normal, sigma_albedo)
    _check(hip.vpt_denoise_device(C.byref(par), width, height, d_color, d_normal, d_albedo, d_variance, d_out, d_scratch, stream),
           "vpt_denoise_device")


def half_variance_device(width: int, height: int, d_sum_a: int, a: int, d_sum_n: int, n: int, d_variance: int, stream: int = 0) -> None:
    """vpt_half_variance_device over raw device pointers (row-major float4 sums in, float variance out), asynchronous on `stream`"""
    _check(hip.vpt_half_variance_device(width, height, d_sum_a, a, d_sum_n, n, d_variance, stream), "vpt_half_variance_device")


def state_init_device(layout: VptLayout, d_image: int, d_hits: int, d_rng: int, stream: int = 0) -> None:
    """vpt_state_init_device: make_state into this rank's tile-major slots on the device (raw device pointers), asynchronous"""
    _check(hip.vpt_state_init_device(C.byref(layout), d_image, d_hits, d_rng, stream), "vpt_state_init_device")


def make_state_jump(width: int, height: int) -> np.ndarray:
    """make_state's rngs, (h, w, 2) uint64, every pixel by a jump of the master stream (csrc/vpt_rng_jump.h, host side)"""
    out = np.zeros((height, width, 2), np.uint64)
    if host.vpth_make_state_jump(width, height, out.ctypes.data) != 0:
        raise VptError("make_state_jump failed")
    return out


def tonemap_image(image: np.ndarray, exposure: float = 0.0, filmic: bool = False, srgb: bool = True, as_bytes: bool = False,
                  device: Optional[int] = None) -> np.ndarray:
    """tonemap_image of the reference (yocto_image.h:242-250; rule: include/vpt.h, vpt_tonemap_device) over an (h, w, 4) float32
    linear image: (h, w, 4) float32, or uint8 through float_to_byte with as_bytes.  device None: the host C++ mirror; else that GPU
    (vpt_tonemap) - the same bits without srgb, the device's powf with it."""
    image = _image4(image)
    h, w, _ = image.shape
    out = np.zeros((h, w, 4), np.uint8 if as_bytes else np.float32)
    f, b = (None, out.ctypes.data) if as_bytes else (out.ctypes.data, None)
    if device is None:
        if host.vpth_tonemap(h * w, image.ctypes.data, exposure, int(filmic), int(srgb), f, b) != 0:
            raise VptError("tonemap_image failed")
    else:
        par = VptDisplay(exposure, int(filmic), int(srgb))
        _check(hip.vpt_tonemap(C.byref(par), device, w, h, image.ctypes.data, f, b), "vpt_tonemap")
    return out


def tonemap_device(width: int, height: int, d_linear: int, d_display_f: Optional[int], d_rgba8: Optional[int], display: DisplayParams,
                   stream: int = 0) -> None:
    """vpt_tonemap_device over raw device pointers (row-major float4 in; float4 and / or RGBA8 out), asynchronous on `stream`"""
    par = display.to_abi()
    _check(hip.vpt_tonemap_device(C.byref(par), width, height, d_linear, d_display_f, d_rgba8, stream), "vpt_tonemap_device")


def upscale_preview(preview: np.ndarray, pratio: int, width: int, height: int) -> np.ndarray:
    """the preview replicated to full size (apps/ypathtrace/ypathtrace.cpp:164-169), host side: (height, width, 4) float32"""
    preview = _image4(preview)
    out = np.zeros((height, width, 4), np.float32)
    if host.vpth_upscale_preview(pratio, preview.shape[1], preview.shape[0], preview.ctypes.data, width, height, out.ctypes.data) != 0:
        raise VptError("upscale_preview: bad preview, size or ratio")
    return out


def upscale_device(pratio: int, pw: int, ph: int, d_preview: int, width: int, height: int, d_out: int, stream: int = 0) -> None:
    """vpt_upscale_device over raw device pointers (row-major float4), asynchronous on `stream`"""
    _check(hip.vpt_upscale_device(pratio, pw, ph, d_preview, width, height, d_out, stream), "vpt_upscale_device")


class RenderSession:
    """vpt_session (include/vpt.h): a progressive render of one camera whose state, linear image and display stay on the GPU of `dev`
    (a DeviceScene).  reset() is the reference's reset_display (preview included), advance(n) renders n more samples and refreshes the
    display; display() / image() / state() fetch.  While it lives, `dev` must not be used from another thread."""

    def __init__(self, dev: "DeviceScene", params: PathtraceParams, pratio: int = 8, display: Optional[DisplayParams] = None,
                 denoise: bool = False, guide_samples: int = 16, iterations: int = DENOISE_ITERATIONS,
                 sigma_luminance: float = DENOISE_SIGMA_LUMINANCE, sigma_normal: float = DENOISE_SIGMA_NORMAL,
                 sigma_albedo: float = DENOISE_SIGMA_ALBEDO, adaptive=None):
        self.dev, self.handle, self.adaptive = dev, None, None
        self._filter = VptDenoise(iterations, sigma_luminance, sigma_normal, sigma_albedo)
        abi = self._abi(params, pratio, display or DisplayParams(), denoise, guide_samples)
        out = _p()
        _check(hip.vpt_session_create(dev.handle, C.byref(abi), C.byref(out)), "vpt_session_create")
        self.handle = out
        if adaptive is not None:  # (threshold, min_samples, step)
            self.set_adaptive(*adaptive)

    def set_adaptive(self, threshold: Optional[float], min_samples: int = 16, step: int = 32) -> None:
        """vpt_session_set_adaptive: adaptive sampling with these settings from now on (params.samples is the per-pixel cap), and a
        reset; set_adaptive(None) switches it off.  A refused call leaves the session as it was."""
        if threshold is None:
            _check(hip.vpt_session_set_adaptive(self.handle, None), "vpt_session_set_adaptive")
            self.adaptive = None
            return
        ad = VptAdaptive(threshold, min_samples, step)
        _check(hip.vpt_session_set_adaptive(self.handle, C.byref(ad)), "vpt_session_set_adaptive")
        self.adaptive = (threshold, min_samples, step)

    def progress(self):
        """adaptive mode: (rounds run since the reset, samples taken, pixels still rendering)"""
        n, rendered, active = C.c_int(0), C.c_int64(0), C.c_int(0)
        _check(hip.vpt_session_progress(self.handle, C.byref(n), C.byref(rendered), C.byref(active)), "vpt_session_progress")
        return n.value, rendered.value, active.value

    def converged(self) -> bool:
        """adaptive mode: no pixel is still rendering"""
        return self.progress()[2] == 0

    def hits(self) -> np.ndarray:
        """adaptive mode: the samples every pixel has taken, (h, w) int32"""
        w, h = self.size
        out = np.zeros((h, w), np.int32)
        _check(hip.vpt_session_get_hits(self.handle, out.ctypes.data), "vpt_session_get_hits")
        return out

    def noise(self):
        """adaptive mode, after an advance: (se2, variance), (h, w) float32 each - the squared standard error of every pixel's mean
        luminance over its rounds, and its box3, which the filter is handed from the second round on"""
        w, h = self.size
        se2, var = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
        _check(hip.vpt_session_get_noise(self.handle, se2.ctypes.data, var.ctypes.data), "vpt_session_get_noise")
        return se2, var

    def adaptive_stats(self):
        """adaptive mode, after an advance: the Welford (mean, m2) of every pixel's rounds, (h, w) float32 each"""
        w, h = self.size
        mean, m2 = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
        _check(hip.vpt_session_get_adaptive_stats(self.handle, mean.ctypes.data, m2.ctypes.data), "vpt_session_get_adaptive_stats")
        return mean, m2

    def _abi(self, params, pratio, display, denoise, guide_samples) -> VptSessionParams:
        self.params, self.pratio, self.display_params, self.denoise, self.guide_samples = params, pratio, display, denoise, guide_samples
        return VptSessionParams(params.to_abi(), pratio, display.to_abi(), int(denoise), self._filter, guide_samples)

    def reset(self, params: Optional[PathtraceParams] = None, pratio: Optional[int] = None, display: Optional[DisplayParams] = None,
              denoise: Optional[bool] = None, guide_samples: Optional[int] = None) -> None:
        """reset_display; any argument given replaces the session's (a new size re-allocates)"""
        if params is None and pratio is None and display is None and denoise is None and guide_samples is None:
            _check(hip.vpt_session_reset(self.handle, None), "vpt_session_reset")
            return
        pick = lambda new, old: old if new is None else new
        old = (self.params, self.pratio, self.display_params, self.denoise, self.guide_samples)
        abi = self._abi(pick(params, old[0]), pick(pratio, old[1]), pick(display, old[2]), pick(denoise, old[3]), pick(guide_samples, old[4]))
        rc = hip.vpt_session_reset(self.handle, C.byref(abi))
        if rc != 0:
            self.params, self.pratio, self.display_params, self.denoise, self.guide_samples = old
        _check(rc, "vpt_session_reset")

    def advance(self, nsamples: int = 1) -> int:
        """min(nsamples, params.samples - samples) more samples, then image and display; returns the samples reached.  In adaptive
        mode: ceil(nsamples / step) whole rounds over the pixels still rendering; returns the largest hit count."""
        _check(hip.vpt_session_advance(self.handle, nsamples), "vpt_session_advance")
        return self.samples

    def set_display(self, display: DisplayParams) -> None:
        """tone-maps the image held again; nothing renders"""
        abi = display.to_abi()
        _check(hip.vpt_session_set_display(self.handle, C.byref(abi)), "vpt_session_set_display")
        self.display_params = display

    def edit(self, edit: SceneEdit) -> None:
        """vpt_scene_update on the session's scene with the SceneEdit of HostScene.update_bvh(), then a reset; a refused edit
        leaves the session as it was"""
        abi, keep = edit.to_abi()
        _check(hip.vpt_session_edit(self.handle, C.byref(abi)), "vpt_session_edit")
        del keep

    def edit_lights(self, edit: SceneEdit) -> None:
        """edit() through vpt_scene_update_lights, with the SceneEdit of HostScene.update_lights()"""
        abi, keep = edit.to_abi()
        _check(hip.vpt_session_edit_lights(self.handle, C.byref(abi)), "vpt_session_edit_lights")
        del keep

    def edit_textures(self, edit: TextureEdit) -> None:
        """edit() through vpt_scene_update_textures, with the TextureEdit of HostScene.update_textures()"""
        abi, keep = edit.to_abi()
        _check(hip.vpt_session_edit_textures(self.handle, C.byref(abi)), "vpt_session_edit_textures")
        del keep

    def edit_volumes(self, edit: VolumeEdit) -> None:
        """edit() through vpt_scene_update_volumes, with the VolumeEdit of HostScene.update_volumes()"""
        abi, keep = edit.to_abi()
        _check(hip.vpt_session_edit_volumes(self.handle, C.byref(abi)), "vpt_session_edit_volumes")
        del keep

    def rebuild_bvh(self, rebuild: "BvhRebuild") -> None:
        """vpt_scene_rebuild_bvh on the session's scene with the BvhRebuild of HostScene.rebuild_bvh(), then a reset"""
        abi, keep = rebuild.to_abi()
        _check(hip.vpt_session_rebuild_bvh_quality(self.handle, C.byref(abi), rebuild.quality), "vpt_session_rebuild_bvh_quality")
        del keep

    def edit_instances(self, edit: InstanceEdit) -> None:
        """vpt_scene_update_instances on the session's scene with the InstanceEdit of HostScene.update_instances(), then a reset; a
        refused edit leaves the session as it was"""
        abi, keep = edit.to_abi()
        _check(hip.vpt_session_edit_instances(self.handle, C.byref(abi)), "vpt_session_edit_instances")
        del keep

    def edit_shapes(self, edit: ShapeEdit) -> None:
        """vpt_scene_update_shapes on the session's scene with the ShapeEdit of HostScene.update_shapes(), then a reset; a refused edit
        leaves the session as it was"""
        abi, keep = edit.to_abi()
        _check(hip.vpt_session_edit_shapes(self.handle, C.byref(abi)), "vpt_session_edit_shapes")
        del keep

    @property
    def size(self):
        w, h = C.c_int(), C.c_int()
        _check(hip.vpt_session_size(self.handle, C.byref(w), C.byref(h)), "vpt_session_size")
        return w.value, h.value

    @property
    def samples(self) -> int:
        return hip.vpt_session_samples(self.handle)

    def display(self, as_bytes: bool = True) -> np.ndarray:
        """the display: (h, w, 4) uint8 (4 B per pixel fetched) or, with as_bytes False, float32 (16 B)"""
        w, h = self.size
        out = np.zeros((h, w, 4), np.uint8 if as_bytes else np.float32)
        _check(hip.vpt_session_get_display(self.handle, out.ctypes.data if as_bytes else None, None if as_bytes else out.ctypes.data),
               "vpt_session_get_display")
        return out

    def image(self, denoised: bool = False) -> np.ndarray:
        """the linear image (the preview after a reset, get_render after an advance), unfiltered; denoised: the filtered one"""
        w, h = self.size
        out = np.zeros((h, w, 4), np.float32)
        if denoised:
            _check(hip.vpt_session_get_denoised(self.handle, out.ctypes.data), "vpt_session_get_denoised")
        else:
            _check(hip.vpt_session_get_image(self.handle, out.ctypes.data), "vpt_session_get_image")
        return out

    def state(self) -> PathtraceState:
        w, h = self.size
        st = PathtraceState(w, h, 0, np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.int32), np.zeros((h, w, 2), np.uint64))
        n = C.c_int(0)
        _check(hip.vpt_session_get_state(self.handle, st.image.ctypes.data, st.hits.ctypes.data, st.rngs.ctypes.data, C.byref(n)),
               "vpt_session_get_state")
        st.samples = n.value
        return st

    def guides(self):
        """denoise = True: the guides the filter reads, (normal, albedo) as resolved (h, w, 4) float32 images; albedo None for the
        implicit shaders"""
        w, h = self.size
        has_albedo = self.params.shader not in ("implicit", "implicit_normal")
        normal, albedo = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32) if has_albedo else None
        _check(hip.vpt_session_get_guides(self.handle, normal.ctypes.data, albedo.ctypes.data if has_albedo else None), "vpt_session_get_guides")
        return normal, albedo

    def pick(self, x: int, y: int) -> Optional[dict]:
        """what is under pixel (x, y) of the frame on display (vpt_session_pick): None on a miss, else a dict of instance, element,
        shape, material, u, v, distance.  24 bytes cross PCIe; the first pick or ids() after a reset makes the id frame."""
        out = VptPick()
        _check(hip.vpt_session_pick(self.handle, x, y, C.byref(out)), "vpt_session_pick")
        if not out.hit:
            return None
        return {name: getattr(out, name) for name in ("instance", "element", "shape", "material", "u", "v", "distance")}

    def ids(self):
        """the id frame (vpt_session_get_ids): (ids, uvt) = (h, w, 2) int32 {instance, element} (-1 on a miss) and (h, w, 3) float32
        {u, v, distance} of the rays through the pixel centres, in vpt_intersect's format"""
        w, h = self.size
        ids, uvt = np.zeros((h, w, 2), np.int32), np.zeros((h, w, 3), np.float32)
        _check(hip.vpt_session_get_ids(self.handle, ids.ctypes.data, uvt.ctypes.data), "vpt_session_get_ids")
        return ids, uvt

    def stats(self):
        """(kernel launches, bytes to the device, bytes to the host) of the last call on the session"""
        n, up, down = C.c_int(0), C.c_int64(0), C.c_int64(0)
        _check(hip.vpt_session_stats(self.handle, C.byref(n), C.byref(up), C.byref(down)), "vpt_session_stats")
        return n.value, up.value, down.value

    def close(self) -> None:
        if getattr(self, "handle", None) and hip is not None:
            hip.vpt_session_destroy(self.handle)
        self.handle = None

    def __del__(self):
        self.close()


def selftest_reciprocal(device: int = 0):
    """(mismatches, fallbacks) of the kernels' exact-reciprocal shortcut over all 2^32 floats (include/vpt.h)"""
    bad, skipped = C.c_ulonglong(0), C.c_ulonglong(0)
    _check(hip.vpt_selftest_reciprocal(device, C.byref(bad), C.byref(skipped)), "vpt_selftest_reciprocal")
    return bad.value, skipped.value


def linear_to_srgb8(image_sum: np.ndarray, samples: int) -> np.ndarray:
    """save_image's quantisation: rgb_to_srgb then float_to_byte (yocto_color.h:207-231)"""
    h, w, _ = image_sum.shape
    out = np.zeros((h, w, 4), np.uint8)
    src = np.ascontiguousarray(image_sum, np.float32)
    host.vpth_linear_to_srgb8(w, h, src.ctypes.data, samples, out.ctypes.data)
    return out


def encode_jpeg_q75(rgba8: np.ndarray) -> bytes:
    """byte-exact stand-in for the reference's stbi_write_jpg(..., quality 75) (stb_image_write.h:1398-1611)"""
    h, w, _ = rgba8.shape
    src = np.ascontiguousarray(rgba8, np.uint8)
    n = host.vpth_encode_jpeg_q75(w, h, src.ctypes.data, None, 0)
    buf = (C.c_uint8 * n)()
    host.vpth_encode_jpeg_q75(w, h, src.ctypes.data, buf, n)
    return bytes(buf)


def layout_pixel_index(layout: VptLayout) -> np.ndarray:
    """Host mirror of the device's slot -> pixel map (slot_to_pixel, csrc/vpt_kernels.hip.h): for every
    state slot of `layout.rank`, the row-major pixel index j*width+i it holds, or -1 for padding."""
    tw, th, w, h = layout.tile_w, layout.tile_h, layout.width, layout.height
    if tw % 8 or th % 8 or tw < 8 or th < 8:
        raise VptError("tile size must be a multiple of 8x8")
    tiles_x, tiles_y = -(-w // tw), -(-h // th)
    per_tile = tw * th
    local_tiles = -(-(tiles_x * tiles_y) // layout.nranks)
    slot = np.arange(local_tiles * per_tile, dtype=np.int64)
    local_tile, p = slot // per_tile, slot % per_tile
    tile = local_tile * layout.nranks + layout.rank
    ty, tx = tile // tiles_x, tile % tiles_x
    bw = tw // 8
    blk, q = p // 64, p % 64
    by, bx = blk // bw, blk % bw
    px = tx * tw + bx * 8 + (q % 8)
    py = ty * th + by * 8 + (q // 8)
    ok = (tile < tiles_x * tiles_y) & (px < w) & (py < h)
    return np.where(ok, py * w + px, -1)
