"""The edits of a resident scene as Python holds them - what HostScene's setters fill and update_*() hands out, what DeviceScene,
MultiDeviceScene and RenderSession apply.  Every class has empty() and to_abi(): (the struct of include/vpt.h, the objects that keep
the arrays it points into alive across the call)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ._abi import (INSTANCE, MESH_ELEMENTS, MESH_FLOATS, SCULPT_RECORD_BYTES, VOXELS_REPLACE, VptBakeDesc, VptBvhRebuild, VptCamera, VptEnvironment,
                   VptError, VptInstanceEdit, VptMaterial, VptSceneEdit, VptSculptEdit, VptSculptEntry, VptSculptStamp, VptSdf, VptShapeData, VptShapeEdit,
                   VptSubdivEdit, VptSubdivLevel, VptSubdivPlan, VptTexture, VptTextureEdit, VptVolumeEdit, VptVolumeInstance, VptVolumeNew, VptVolumeSetEdit,
                   VptVolumeSource, VOLUME_FILL, VOLUME_FROM_BAKE, VOLUME_FROM_HOST, _address)


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


# ---- the two list edits: remove / set / add over the instances or over the shapes ------------------------------------------------------
class _ListEdit:
    """`set`, a dictionary current id -> item that replaces those entries; `remove`, current ids erased after that (ids close up); `add`,
    a list of items appended after the survivors.  A subclass says what an item is (_item), how items are packed into records
    (_records), which struct takes them (ABI) and what besides the records has to stay alive (_kept)."""
    ABI = None

    def __init__(self, remove=(), set=None, add=()):
        self.remove = tuple(int(i) for i in remove)
        self.set = {int(k): self._item(v) for k, v in dict(set or {}).items()}
        self.add = [self._item(v) for v in add]

    def empty(self) -> bool:
        return not (self.remove or self.set or self.add)

    def _kept(self) -> list:
        return []

    def to_abi(self):
        """(the struct, the arrays it points into: keep them alive across the call)"""
        remove, set_ids = np.array(self.remove, np.int32), np.array(list(self.set.keys()), np.int32)
        set_rec, add_rec = self._records(list(self.set.values())), self._records(self.add)
        ptr = lambda a, n: _address(a) if n else None   # (a record array of no items still has one unused element)
        abi = self.ABI(len(remove), ptr(remove, len(remove)), len(set_ids), ptr(set_ids, len(set_ids)), ptr(set_rec, len(set_ids)),
                       len(self.add), ptr(add_rec, len(self.add)))
        return abi, [remove, set_ids, set_rec, add_rec] + self._kept()


class InstanceEdit(_ListEdit):
    """What vpt_scene_update_instances takes (include/vpt.h: vpt_instance_edit): `set`, a dictionary current id -> (frame (12,) float32,
    shape, material) that replaces those instances; `remove`, current ids erased after that (ids close up); `add`, a list of (frame,
    shape, material) appended after the survivors.  HostScene.update_instances makes one; DeviceScene.update_instances /
    MultiDeviceScene.update_instances / RenderSession.edit_instances apply it."""
    ABI = VptInstanceEdit

    @staticmethod
    def _item(v):
        return np.ascontiguousarray(v[0], np.float32).reshape(12).copy(), int(v[1]), int(v[2])

    @staticmethod
    def _records(items) -> np.ndarray:
        out = np.zeros(len(items), INSTANCE)
        for i, (frame, shape, material) in enumerate(items):
            out[i] = (frame, shape, material)
        return out


class ShapeEdit(_ListEdit):
    """What vpt_scene_update_shapes takes (include/vpt.h: vpt_shape_edit): `set`, a dictionary current id -> mesh (the dictionary mesh()
    makes) that replaces those shapes whole; `remove`, current ids erased after that (ids close up, the instances' shape ids follow; no
    instance may name a removed shape); `add`, a list of meshes appended after the survivors.  HostScene.update_shapes makes one;
    DeviceScene.update_shapes / MultiDeviceScene.update_shapes / RenderSession.edit_shapes apply it.
    Importing an object into a running scene is a ShapeEdit followed by an InstanceEdit: add_shape(...) returns the id the shape has after
    update_shapes(); once that edit is handed out, add_instance(frame, id, material) and update_instances() put it in place."""
    ABI = VptShapeEdit

    @staticmethod
    def _item(v):
        return mesh(**v)

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

    def _kept(self) -> list:
        return [self.set, self.add]   # the meshes the records point into


# ---- subdivision surfaces: the plan that is attached once, and the edit of cages and displacements ---------------------------------------
LEVEL_TABLES = {"edges": 2, "faces": 4, "new_faces": 4, "valence": 0, "offsets": 0, "items": 0}   # int32 per entry (0: a plain array)


class SubdivPlan:
    """What vpt_scene_attach_subdiv takes (include/vpt.h: vpt_subdiv_plan): the settings of a subdiv, its cage's floats and the integer
    half of its tesselation - `levels`, a list of dictionaries of the int32 tables of LEVEL_TABLES (one vpt_subdiv_level each, dim 3),
    `quads` (n, 4) after the last level and `verts` (m, 3), split_facevarying's table.  HostScene.subdiv_plan makes one."""

    def __init__(self, shape, subdivisions, smooth, displacement, displacement_tex, cage_positions, cage_normals, levels, quads, verts):
        self.shape, self.subdivisions, self.smooth = int(shape), int(subdivisions), bool(smooth)
        self.displacement, self.displacement_tex = float(displacement), int(displacement_tex)
        self.cage_positions = np.ascontiguousarray(cage_positions, np.float32).reshape(-1, 3)
        self.cage_normals = np.ascontiguousarray(cage_normals, np.float32).reshape(-1, 3)
        self.levels = [{k: np.ascontiguousarray(L[k], np.int32).reshape((-1, w) if w else (-1,)) for k, w in LEVEL_TABLES.items()} for L in levels]
        self.quads = np.ascontiguousarray(quads, np.int32).reshape(-1, 4)
        self.verts = np.ascontiguousarray(verts, np.int32).reshape(-1, 3)

    def to_abi(self):
        """(VptSubdivPlan, the arrays it points into: keep them alive across the call)"""
        levels = (VptSubdivLevel * max(1, len(self.levels)))()
        nv = len(self.cage_positions)
        for rec, L in zip(levels, self.levels):
            rec.dim, rec.num_vertices, rec.num_edges, rec.num_faces, rec.num_new_faces = 3, nv, len(L["edges"]), len(L["faces"]), len(L["new_faces"])
            for k in LEVEL_TABLES:
                setattr(rec, k, L[k].ctypes.data)
            rec.num_items = len(L["items"])
            nv = nv + rec.num_edges + rec.num_faces
        ptr = lambda a: a.ctypes.data if len(a) else None
        abi = VptSubdivPlan(self.shape, self.subdivisions, int(self.smooth), self.displacement, self.displacement_tex,
                            len(self.cage_positions), ptr(self.cage_positions), len(self.cage_normals), ptr(self.cage_normals),
                            len(self.levels), C.addressof(levels) if self.levels else None, len(self.quads), ptr(self.quads), len(self.verts), ptr(self.verts))
        return abi, [levels, self]


class SubdivEdit:
    """What vpt_scene_update_subdivs takes (include/vpt.h: vpt_subdiv_edit), as a dictionary subdiv id -> (cage positions (n, 3) float32
    or None: keep, displacement or None: keep); an entry (None, None) tesselates again from what the device holds.  `shape_of`: subdiv
    id -> the shape it edits, `plan_of`: a function subdiv id -> SubdivPlan - how DeviceScene.update_subdivs, MultiDeviceScene.update_subdivs
    and RenderSession.edit_subdivs attach a named subdiv's plan on first use.  HostScene.set_subdiv fills one, update_subdivs() hands it out."""

    def __init__(self, subdivs=None, shape_of=None, plan_of=None):
        self.subdivs = {int(k): (None if p is None else np.ascontiguousarray(p, np.float32).reshape(-1, 3).copy(), None if d is None else float(d))
                        for k, (p, d) in dict(subdivs or {}).items()}
        self.shape_of, self.plan_of = dict(shape_of or {}), plan_of

    def empty(self) -> bool:
        return not self.subdivs

    def payload_bytes(self) -> int:
        """bytes of the edit itself as vpt_scene_update_stats counts them: 12 per cage vertex of an entry with a new cage"""
        return sum(p.nbytes for p, _ in self.subdivs.values() if p is not None)

    def to_abi(self, ids=None):
        """(VptSubdivEdit, objects that keep its arrays alive); ids: subdiv id -> the id its plan has on the device (None: the same)"""
        n = len(self.subdivs)
        names = np.array([k if ids is None else ids[k] for k in self.subdivs], np.int32)
        cages, amounts = (C.c_void_p * max(1, n))(), np.full(max(1, n), np.nan, np.float32)
        for i, (p, d) in enumerate(self.subdivs.values()):
            cages[i] = None if p is None else p.ctypes.data
            if d is not None:
                amounts[i] = d
        abi = VptSubdivEdit(n, names.ctypes.data if n else None, C.addressof(cages), amounts.ctypes.data)
        return abi, [names, cages, amounts, self.subdivs]


# ---- the three dictionary edits, id -> value, and the packing they share ---------------------------------------------------------------
def _structs(d: dict, T):
    """the values of a dictionary as a ctypes array of T (one unused element where the dictionary is empty)"""
    return (T * max(1, len(d)))(*d.values())


def _frames(d: dict) -> np.ndarray:
    return np.ascontiguousarray(np.array([np.asarray(f, np.float32).reshape(12) for f in d.values()], np.float32).reshape(-1, 12))


def _table(keep: list, d: dict, payload):
    """one id -> value table of an edit, its values packed in `payload`: (count, address of the ids, address of the payload); both
    arrays join `keep`"""
    ids = np.array(list(d.keys()), np.int32)
    keep += [ids, payload]
    return len(d), ids.ctypes.data, _address(payload)


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
        abi.num_cameras, abi.camera_ids, abi.cameras = _table(keep, self.cameras, _structs(self.cameras, VptCamera))
        abi.num_instances, abi.instance_ids, abi.instance_frames = _table(keep, self.instances, _frames(self.instances))
        abi.num_environments, abi.environment_ids, abi.environment_frames = _table(keep, self.environments, _frames(self.environments))
        abi.num_materials, abi.material_ids, abi.materials = _table(keep, self.materials, _structs(self.materials, VptMaterial))
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
        abi.num_shapes, abi.shape_ids, abi.shape_positions = _table(keep, self.shapes, pos)
        abi.shape_normals = _address(nrm)
        return abi, keep + [nrm]


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
        abi.num_environments, abi.environment_ids, abi.environments = _table(keep, self.environments, _structs(self.environments, VptEnvironment))
        abi.num_textures, abi.texture_ids, abi.textures = _table(keep, self.textures, entries)
        abi.num_texels_f, abi.texels_f = len(texels_f), texels_f.ctypes.data
        abi.num_texels_b, abi.texels_b = len(texels_b), texels_b.ctypes.data
        return abi, keep + [texels_f, texels_b]


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
        abi.num_vol_instances, abi.vol_instance_ids, abi.vol_instances = _table(keep, self.vol_instances, _structs(self.vol_instances, VptVolumeInstance))
        abi.num_sdfs, abi.sdf_ids, abi.sdfs = _table(keep, self.sdfs, _structs(self.sdfs, VptSdf))
        abi.num_volumes, abi.volume_ids, abi.volumes = _table(keep, self.volumes, entries)
        abi.num_voxels, abi.voxels = len(voxels), voxels.ctypes.data
        return abi, keep + [voxels]


# ---- the set of volumes, grid instances and SDFs: remove / add over the three lists -----------------------------------------------------
@dataclass
class VolumeNew:
    """One added volume of a VolumeSetEdit (include/vpt.h: vpt_volume_new): whd (w, h, d), res, and where the voxels come from - source
    VOLUME_FROM_HOST: voxels, float32 of shape (d, h, w); VOLUME_FROM_BAKE: bake = (positions (n, 3), triangles (m, 3), origin, step), the
    grid of bake_sdf_grid over whd; VOLUME_FILL: the bits of `fill` in every voxel; VOLUME_COPY: the voxels volume copy_of (a current id,
    of the same whd) holds before the edit."""
    whd: tuple
    res: float
    source: int = VOLUME_FROM_HOST
    voxels: Optional[np.ndarray] = None
    bake: Optional[tuple] = None
    fill: float = 0.0
    copy_of: int = -1


class VolumeSetEdit:
    """What vpt_scene_update_volume_set takes (include/vpt.h: vpt_volume_set_edit): current ids of grid instances, SDFs and volumes to
    erase (the ids close up, a surviving instance's volume id follows), then volumes (VolumeNew), grid instances (VptVolumeInstance, their
    `volume` in the NEW numbering) and SDFs (VptSdf) appended after the survivors.  HostScene's add_volume / remove_volumes /
    add_volume_instance / remove_volume_instances / add_sdf / remove_sdfs fill one, update_volume_set() hands it out;
    DeviceScene.update_volume_set / MultiDeviceScene.update_volume_set / RenderSession.edit_volume_set apply it."""

    def __init__(self, remove_vol_instances=(), remove_sdfs=(), remove_volumes=(), add_volumes=(), add_vol_instances=(), add_sdfs=()):
        self.remove_vol_instances = tuple(int(i) for i in remove_vol_instances)
        self.remove_sdfs = tuple(int(i) for i in remove_sdfs)
        self.remove_volumes = tuple(int(i) for i in remove_volumes)
        self.add_volumes, self.add_vol_instances, self.add_sdfs = list(add_volumes), list(add_vol_instances), list(add_sdfs)

    def empty(self) -> bool:
        return not (self.remove_vol_instances or self.remove_sdfs or self.remove_volumes or self.add_volumes or self.add_vol_instances or self.add_sdfs)

    def to_abi(self):
        """(VptVolumeSetEdit, objects that keep its arrays alive)"""
        keep, abi = [], VptVolumeSetEdit()
        entries = (VptVolumeNew * max(1, len(self.add_volumes)))()
        pool, count = [], 0
        for e, new in zip(entries, self.add_volumes):
            whd = tuple(int(v) for v in new.whd)
            e.whd[:], e.res, e.source, e.fill, e.copy_of = whd, float(new.res), int(new.source), float(new.fill), int(new.copy_of)
            if new.source == VOLUME_FILL:   # the bits as they are: a NaN keeps its payload
                C.memmove(C.addressof(e) + VptVolumeNew.fill.offset, np.array([new.fill], np.float32).ctypes.data, 4)
            if new.source == VOLUME_FROM_BAKE:
                positions, triangles, origin, step = new.bake
                positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
                triangles = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
                desc = VptBakeDesc(len(positions), positions.ctypes.data, len(triangles), triangles.ctypes.data)
                desc.whd[:] = whd
                desc.origin[:] = [float(v) for v in np.broadcast_to(np.asarray(origin, np.float32), (3,))]
                desc.step[:] = [float(v) for v in np.broadcast_to(np.asarray(step, np.float32), (3,))]
                keep += [positions, triangles, desc]
                e.bake = C.addressof(desc)
            elif new.source == VOLUME_FROM_HOST:
                voxels = np.ascontiguousarray(new.voxels, np.float32)
                if voxels.shape != whd[::-1]:
                    raise VptError(f"voxels of an added volume have the shape (d, h, w) = {whd[::-1]}, got {voxels.shape}")
                e.offset = count
                pool.append(voxels.reshape(-1))
                count += voxels.size
        voxels = np.ascontiguousarray(np.concatenate(pool)) if pool else np.zeros(0, np.float32)
        for name, ids in (("remove_vol_instance", self.remove_vol_instances), ("remove_sdf", self.remove_sdfs), ("remove_volume", self.remove_volumes)):
            arr = np.array(ids, np.int32)
            keep.append(arr)
            setattr(abi, f"num_{name}s", len(arr))
            setattr(abi, f"{name}_ids", arr.ctypes.data if len(arr) else None)
        instances, sdfs = (VptVolumeInstance * max(1, len(self.add_vol_instances)))(*self.add_vol_instances), (VptSdf * max(1, len(self.add_sdfs)))(*self.add_sdfs)
        abi.num_add_volumes, abi.add_volumes = len(self.add_volumes), C.addressof(entries) if self.add_volumes else None
        abi.num_add_vol_instances, abi.add_vol_instances = len(self.add_vol_instances), C.addressof(instances) if self.add_vol_instances else None
        abi.num_add_sdfs, abi.add_sdfs = len(self.add_sdfs), C.addressof(sdfs) if self.add_sdfs else None
        abi.num_voxels, abi.voxels = len(voxels), voxels.ctypes.data if len(voxels) else None
        return abi, keep + [entries, instances, sdfs, voxels]


# ---- sculpting: strokes of analytic brushes over boxes of voxels --------------------------------------------------------------------------
@dataclass
class Stamp:
    """One stamp of a stroke (include/vpt.h: vpt_sculpt_stamp): an analytic brush (a VptSdf; its material is ignored), the op -
    SCULPT_REPLACE / SCULPT_UNION / SCULPT_SUBTRACT / SCULPT_INTERSECT - and the blend width (0: the reference's selects; > 0: the
    polynomial smooth minimum over that width)."""
    brush: VptSdf
    op: int
    blend: float = 0.0

    def to_abi(self) -> VptSculptStamp:
        out = VptSculptStamp(op=int(self.op), blend=float(self.blend))
        C.memmove(C.byref(out.brush), C.byref(self.brush), C.sizeof(VptSdf))
        return out


@dataclass
class SculptEntry:
    """One entry of a SculptEdit (include/vpt.h: vpt_sculpt_entry): the volume, the box region_lo .. region_lo + region_whd of its voxels
    (each (x, y, z)), the grid they are sampled on - voxel (i, j, k) at origin + (i, j, k) * step - and the stroke: Stamps in order."""
    volume: int
    region_lo: tuple
    region_whd: tuple
    origin: tuple
    step: tuple
    stamps: list


class SculptEdit:
    """What vpt_scene_sculpt_volumes takes (include/vpt.h: vpt_sculpt_edit): a list of SculptEntry, applied in order; a volume may be
    named more than once.  HostScene.sculpt_volume fills one, update_sculpts() hands it out; DeviceScene.sculpt_volumes /
    MultiDeviceScene.sculpt_volumes / RenderSession.edit_sculpts apply it."""

    def __init__(self, entries=()):
        self.entries = list(entries)

    def empty(self) -> bool:
        return not self.entries

    def payload_bytes(self) -> int:
        """bytes of the edit itself as vpt_scene_update_stats counts them: SCULPT_RECORD_BYTES per stamp when anything is launched"""
        launched = any(len(e.stamps) and all(int(v) > 0 for v in e.region_whd) for e in self.entries)
        return SCULPT_RECORD_BYTES * sum(len(e.stamps) for e in self.entries) if launched else 0

    def to_abi(self):
        """(VptSculptEdit, the arrays it points into: keep them alive across the call)"""
        count = sum(len(e.stamps) for e in self.entries)
        entries, stamps = (VptSculptEntry * max(1, len(self.entries)))(), (VptSculptStamp * max(1, count))()
        first = 0
        for rec, e in zip(entries, self.entries):
            rec.volume, rec.first_stamp, rec.num_stamps = int(e.volume), first, len(e.stamps)
            rec.region_lo[:], rec.region_whd[:] = [int(v) for v in e.region_lo], [int(v) for v in e.region_whd]
            rec.origin[:] = [float(v) for v in np.broadcast_to(np.asarray(e.origin, np.float32), (3,))]
            rec.step[:] = [float(v) for v in np.broadcast_to(np.asarray(e.step, np.float32), (3,))]
            for s in e.stamps:
                stamps[first] = s.to_abi()
                first += 1
        abi = VptSculptEdit(len(self.entries), C.addressof(entries) if self.entries else None, count, C.addressof(stamps) if count else None)
        return abi, [entries, stamps]
