"""The host side of a scene: HostScene (load_scene + tesselate_surfaces + make_bvh + make_lights through libvpt_host.so, the getters and
setters of a loaded scene, and the ledger of its pending edits) and the free host functions it uses."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ._abi import (BVH_MIDDLE, BVH_NODE, BVH_SAH, LIGHT, MESH_ELEMENTS, MESH_FLOATS, SDF_TYPES, VOLUME_COPY, VOLUME_FILL, VOLUME_FROM_BAKE, VOLUME_FROM_HOST, VOXELS_REPLACE, VptBakeStats, VptCamera,
                   VptEnvironment, VptError, VptMaterial, VptSceneDescBvh, VptSceneDescLights, VptSculptEntry, VptSdf, VptVolumeInstance, _Handle,
                   _check, _filled, _host_call, _mesh_desc, _mesh_region, _meshed, hip, host)
from .device import PathtraceParams, PathtraceState
from .edits import (LEVEL_TABLES, BvhRebuild, InstanceEdit, SceneEdit, SculptEdit, SculptEntry, ShapeEdit, Stamp, SubdivEdit, SubdivPlan,
                    TextureEdit, VolumeEdit, VolumeNew, VolumeSetEdit, VolumeSource, mesh)


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
    _host_call(host.vpth_catmullclark, quads.ctypes.data, n, verts.ctypes.data, m, dim, int(lock_boundary), -1 if device is None else device,
               qo.ctypes.data, C.byref(nq), vo.ctypes.data, C.byref(nv))
    return qo[:nq.value].copy(), vo[:nv.value].copy()


def vertex_normals(positions: np.ndarray, faces: np.ndarray, device: Optional[int] = None) -> np.ndarray:
    """quads_normals ((n, 4) faces; z == w: a triangle) / triangles_normals ((n, 3)) of yocto_shape.cpp:1478-1512 over (m, 3) float32
    positions: area-weighted face normals added per vertex in face order, normalised.  device: GPU index (vpt_vertex_normals)."""
    positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32)
    out = np.zeros_like(positions)
    _host_call(host.vpth_vertex_normals, positions.ctypes.data, len(positions), faces.ctypes.data, len(faces), faces.shape[1],
               -1 if device is None else device, out.ctypes.data)
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
    _host_call(host.vpth_displace_vertices, texels.ctypes.data, texels.shape[1], texels.shape[0], int(texels.dtype == np.float32), int(linear),
               C.c_float(displacement), positions.ctypes.data, normals.ctypes.data, texcoords.ctypes.data, len(positions),
               -1 if device is None else device, out.ctypes.data)
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
    _host_call(host.vpth_bake_grid, positions.ctypes.data, len(positions), triangles.ctypes.data, len(triangles), whd.ctypes.data, origin.ctypes.data,
               step.ctypes.data, -1 if device is None else device, voxels.ctypes.data, C.byref(st))
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
    _host_call(host.vpth_fit_volume, bmin.ctypes.data, bmax.ctypes.data, whd.ctypes.data, padding, C.byref(res), origin.ctypes.data, step.ctypes.data,
               frame.ctypes.data)
    return res.value, origin, step, frame


def save_volume(path: str, voxels: np.ndarray, res: float) -> None:
    """the binary .sdf file the scene loader reads ("binary": true): int32 w h d, float res, 16 floats, the voxels; voxels of shape (d, h, w)"""
    voxels = np.ascontiguousarray(voxels, np.float32)
    if voxels.ndim != 3:
        raise VptError(f"expected (d, h, w) voxels, got {voxels.shape}")
    whd = np.array(voxels.shape[::-1], np.int32)
    _host_call(host.vpth_save_volume, os.fsencode(path), whd.ctypes.data, C.c_float(res), voxels.ctypes.data)


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
    _host_call(host.vpth_bake_volume, positions.ctypes.data, len(positions), triangles.ctypes.data, len(triangles), whd.ctypes.data, padding,
               -1 if device is None else device, voxels.ctypes.data, C.byref(res), frame.ctypes.data, C.byref(st))
    return BakedVolume(voxels.reshape(int(whd[2]), int(whd[1]), int(whd[0])), res.value, frame, 1.0, _bake_stats(st))


def mesh_sdf(voxels: np.ndarray, origin, step, iso: float = 0.0, device: Optional[int] = 0, *, region=None, stats: Optional[dict] = None) -> dict:
    """The iso surface of a signed-distance grid as a quad mesh by the rule of include/vpt.h (vpt_mesh_sdf: naive surface nets).  voxels:
    (d, h, w) float32, voxel (i, j, k) sampled at origin + (i, j, k) * step (three floats each, or one for every axis); inside is
    voxel < iso.  Returns the mesh(...) dictionary HostScene.add_shape takes: positions, normals (n, 3) float32 and quads (m, 4) int32 that
    face out of the inside (None where the surface does not cross the grid).  device: GPU index, or None for the host mirror - the same
    bits.  region = (lo, whd), each (x, y, z), host mirror only: that box meshed as a grid of its own, its vertices in place
    (vpt_scene_mesh_volume's region).  stats: a dict that receives num_vertices, num_quads, launches, device_ms."""
    voxels = np.ascontiguousarray(voxels, np.float32)
    if voxels.ndim != 3:
        raise VptError(f"expected (d, h, w) voxels, got {voxels.shape}")
    desc, box = _mesh_desc(voxels.shape[::-1], origin, step, iso), _mesh_region(region)
    if device is None:
        call = lambda *out: _host_call(host.vpth_mesh_sdf, C.byref(desc), voxels.ctypes.data, C.byref(box) if box else None, *out)
    elif box is not None:
        raise VptError("mesh_sdf: a region is meshed by the host mirror (device=None) or out of a resident scene (DeviceScene.mesh_volume)")
    else:
        call = lambda *out: _check(hip.vpt_mesh_sdf(device, C.byref(desc), voxels.ctypes.data, *out), "vpt_mesh_sdf")
    m = _meshed(call, stats)
    return mesh(m["positions"], quads=m["quads"], normals=m["normals"])


def density_from_sdf(voxels: np.ndarray, width: float) -> np.ndarray:
    """a signed-distance grid as a soft-edged cloud for the volgrid shader: clip(-sdf / width, 0, 1) in float32 - 1 from `width` inside
    the surface on, 0 outside it.  A baked or sculpted volume becomes a medium with set_volume(index, density_from_sdf(voxels, width))."""
    width = np.float32(width)
    if not (np.isfinite(width) and width > 0):
        raise VptError(f"density_from_sdf: width {width!r} must be finite and > 0")
    return np.clip(-np.asarray(voxels, np.float32) / width, np.float32(0), np.float32(1)).astype(np.float32)


def save_mesh_ply(path: str, positions, quads, normals=None) -> None:
    """positions, normals (unless None) and quads as a binary little-endian PLY file, which the scene loader reads back with the same bits"""
    positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    quads = np.ascontiguousarray(np.zeros((0, 4)) if quads is None else quads, np.int32).reshape(-1, 4)
    if normals is not None:
        normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if len(normals) != len(positions):
            raise VptError("save_mesh_ply: one normal per vertex")
    _host_call(host.vpth_save_mesh_ply, os.fsencode(path), positions.ctypes.data, None if normals is None else normals.ctypes.data, len(positions),
               quads.ctypes.data, len(quads))


# Which change of a HostScene may begin while which other is pending.  The ids of a pending edit name the lists as they were when it
# began, so a change that renumbers or relies on a list waits until the edit over that list is handed out.  Kind of call -> the pending
# state that refuses it, asked in this order:
#   "edit": a SceneEdit that holds anything; "geometry": one that holds instance frames or shape vertices (cameras, materials and
#   environment frames name lists nothing renumbers); "instances" / "shapes": an InstanceEdit / ShapeEdit that holds anything;
#   "subdivs": a SubdivEdit that holds anything (its shapes wait for update_bvh like moved vertices).
# Texture and volume edits name lists of their own and wait for nothing of the above; set_camera, set_material, set_environment_frame are
# never refused.  The implicit side has the same rule within itself: "volumes": a VolumeEdit or SculptEdit that holds anything - their ids
# name the volumes, grid instances and SDFs as they are - and "volume_set": a VolumeSetEdit that holds anything, which renumbers all three.
# A volume's voxels have two ledgers, the VolumeEdit and the SculptEdit: a volume pending in one is refused by the setters of the other
# (_note_volume, sculpt_volume), since each ledger is applied to the device as a whole and in its own call.
_REFUSED_WHILE = {"vertices": ("instances", "shapes"),                       # set_instance_frame, set_shape_positions, set_subdiv (cage, displacement)
                  "rebuild": ("edit", "subdivs", "instances", "shapes"),      # rebuild_bvh
                  "instances": ("geometry", "subdivs", "shapes"),             # add_instance, remove_instances, set_instance, update_instances
                  "shapes": ("geometry", "subdivs", "instances"),             # add_shape, set_shape, remove_shapes, update_shapes, set_subdiv (level, smooth)
                  "volume_entries": ("volume_set",),                          # set_volume_instance, set_sdf, set_volume, bake_volume, sculpt_volume
                  "volume_set": ("volumes",)}                                 # add_volume, remove_volumes, add_volume_instance, ..., update_volume_set
_HAND_OUT = {"edit": "edit out with update_bvh()", "geometry": "edit out with update_bvh()",
             "instances": "instance changes out with update_instances()", "shapes": "shape changes out with update_shapes()",
             "subdivs": "subdiv changes out with update_subdivs()", "volumes": "volume changes out with update_volumes() / update_sculpts()",
             "volume_set": "additions and removals of volumes, grid instances and SDFs out with update_volume_set()"}


class HostScene(_Handle):
    """load_scene + tesselate_surfaces + make_bvh + make_lights, flattened for the C-ABI."""
    _free = staticmethod(host.vpth_scene_free)

    def __init__(self, filename: str, bvh_device: Optional[int] = None, tess_device: Optional[int] = None, *, bvh_quality: int = 0):
        """bvh_device: build the BVHs on that GPU (make_bvh_device / vpt_build_bvh_quality) instead of on the host - same arrays;
        tess_device: the vertex arithmetic of tesselate_surfaces on that GPU (vpt_subdivide_vertices) - same mesh;
        bvh_quality: BVH_MIDDLE, or BVH_SAH for make_bvh(..., highquality = true) - every tree is built at that quality after loading"""
        if bvh_quality not in (BVH_MIDDLE, BVH_SAH):
            raise VptError(f"HostScene: unknown bvh_quality {bvh_quality!r}")
        # the pending edits: what the setters noted since the matching update_*() handed the last one out
        self._edit, self._inst_edit, self._shape_edit = SceneEdit(), InstanceEdit(), ShapeEdit()
        self._texture_edit, self._volume_edit, self._subdiv_edit = TextureEdit(), VolumeEdit(), SubdivEdit()
        self._sculpt_edit, self._volume_set_edit = SculptEdit(), VolumeSetEdit()
        self._lazy_bakes = []   # (volume, VolumeSource) of bake_volume whose host copy is not baked yet
        self.handle = _host_call(host.vpth_scene_load_ex, os.fsencode(filename), -1 if tess_device is None else tess_device, size=1024, handle=True)
        self.filename = filename
        if bvh_device is not None:
            _host_call(host.vpth_scene_rebuild_bvh_device_quality, self.handle, bvh_device, bvh_quality, size=1024)
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

    def _get(self, kind: int, index: int, out):
        """item `index` of a kind, into `out` (None: a float32 array of the item's size)"""
        return _filled(lambda ptr, n: host.vpth_scene_get_item(self.handle, kind, index, ptr, n),
                       lambda n: np.zeros(n // 4, np.float32) if out is None else out, f"item {index} out of range")

    def _set(self, kind: int, index: int, value) -> None:
        if isinstance(value, np.ndarray):
            ptr, n = value.ctypes.data, value.nbytes
        else:
            ptr, n = C.addressof(value), C.sizeof(value)
        _host_call(host.vpth_scene_set_item, self.handle, kind, index, ptr, n)

    def _may(self, what: str, kind: str, why: str = "") -> None:
        """VptError unless a call of `kind` (_REFUSED_WHILE) may go ahead: the message names the update_*() to call first"""
        pending = {"edit": not self._edit.empty(), "geometry": bool(self._edit.instances or self._edit.shapes),
                   "instances": not self._inst_edit.empty(), "shapes": not self._shape_edit.empty(), "subdivs": not self._subdiv_edit.empty(),
                   "volumes": not (self._volume_edit.empty() and self._sculpt_edit.empty()), "volume_set": not self._volume_set_edit.empty()}
        for blocker in _REFUSED_WHILE[kind]:
            if pending[blocker]:
                raise VptError(f"{what}: hand the pending {_HAND_OUT[blocker]} first" + (why if blocker == "geometry" else ""))

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
        voxels = _filled(lambda ptr, n: host.vpth_scene_get_volume(self.handle, index, whd.ctypes.data, C.byref(res), ptr, n),
                         lambda n: np.zeros(n, np.float32), f"volume {index} out of range")
        return voxels.reshape(int(whd[2]), int(whd[1]), int(whd[0])), res.value

    def set_camera(self, index: int, camera: VptCamera) -> None:
        self._set(self._CAMERA, index, camera)
        self._edit.cameras[index] = self.camera(index)

    def set_instance_frame(self, index: int, frame) -> None:
        self._may("set_instance_frame", "vertices")
        frame = np.ascontiguousarray(frame, np.float32).reshape(12)
        self._set(self._INSTANCE, index, frame)
        self._edit.instances[index] = frame.copy()

    def set_environment_frame(self, index: int, frame) -> None:
        frame = np.ascontiguousarray(frame, np.float32).reshape(12)
        self._set(self._ENVIRONMENT, index, frame)
        self._edit.environments[index] = frame.copy()

    def set_material(self, index: int, material: VptMaterial) -> None:
        self._set(self._MATERIAL, index, material)
        self._edit.materials[index] = self.material(index)

    def set_shape_positions(self, index: int, positions, normals=None) -> None:
        """the vertices of a shape (same count), and its normals when given"""
        self._may("set_shape_positions", "vertices")
        positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        self._set(self._POSITIONS, index, positions)
        if normals is not None:
            normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
            self._set(self._NORMALS, index, normals)
            normals = normals.copy()
        elif index in self._edit.shapes:
            normals = self._edit.shapes[index][1]
        self._edit.shapes[index] = (positions.copy(), normals)

    def update_bvh(self) -> SceneEdit:
        """update_bvh of the reference over what the setters changed since the last call (a refit: topology and primitive order stay);
        desc / stats() describe the edited scene afterwards.  Returns the SceneEdit for DeviceScene.update."""
        _host_call(host.vpth_scene_update_bvh, self.handle)
        edit, self._edit = self._edit, SceneEdit()
        return edit

    def update_lights(self) -> SceneEdit:
        """update_bvh(), then make_lights of the edited scene (an emission switched on or off, an emitter's vertices moved): desc /
        stats() carry the new light list and CDFs.  Returns the SceneEdit for DeviceScene.update_lights."""
        edit = self.update_bvh()
        _host_call(host.vpth_scene_update_lights, self.handle)
        return edit

    def rebuild_bvh(self, shapes=None, scene: bool = True, *, quality: int = 0) -> "BvhRebuild":
        """make_bvh of the reference again, on the scene as it is now, for the shapes named (ids; "all": every shape; None: none) and
        - `scene`, or whenever a shape is named - for the scene BVH: topology, node counts and primitive orders change; desc / stats()
        describe the rebuilt scene afterwards.  A pending edit is handed out with update_bvh() first.  Returns the BvhRebuild for
        DeviceScene.rebuild_bvh.  quality: BVH_MIDDLE or BVH_SAH for every tree this call builds; the others keep theirs."""
        if quality not in (BVH_MIDDLE, BVH_SAH):
            raise VptError(f"rebuild_bvh: unknown quality {quality!r}")
        self._may("rebuild_bvh", "rebuild")
        ids = list(range(self.count("shapes"))) if isinstance(shapes, str) and shapes == "all" else [int(i) for i in (shapes or ())]
        arr = np.ascontiguousarray(ids, np.int32)
        _host_call(host.vpth_scene_rebuild_bvh_quality, self.handle, arr.ctypes.data if len(arr) else None, len(arr), int(bool(scene)), quality)
        return BvhRebuild(ids, scene, quality=quality)

    # -- the set of instances (the host side of vpt_scene_update_instances): add_instance / remove_instances / set_instance note a
    #    change, ids naming the list as it is now; update_instances() applies them to the scene - set, then remove, then add - builds
    #    the scene BVH and the lights anew and hands the InstanceEdit out.  The ids of a pending SceneEdit name the old list, so the
    #    two kinds of change do not mix: each is handed out before the other begins ------------------------------------------------
    def _begin_instance_change(self, what: str) -> InstanceEdit:
        self._may(what, "instances", " (its ids name the instances as they are now)")
        return self._inst_edit

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
        self._may("update_instances", "instances")
        edit, self._inst_edit = self._inst_edit, InstanceEdit()
        if edit.empty():
            return edit
        abi, keep = edit.to_abi()
        _host_call(host.vpth_scene_edit_instances, self.handle, abi.remove_ids, abi.num_remove, abi.set_ids, abi.set, abi.num_set, abi.add,
                   abi.num_add)
        del keep
        return edit

    # -- the shape list (the host side of vpt_scene_update_shapes): add_shape / set_shape / remove_shapes note a change, ids naming the
    #    list as it is now; update_shapes() applies them to the scene - set, then remove, then add - builds the new shapes' BVHs (and the
    #    scene BVH when a shape was replaced) and the lights anew and hands the ShapeEdit out.  The ids of a pending SceneEdit or
    #    InstanceEdit name the old list, so the kinds of change do not mix: each is handed out before another begins ---------------------
    def _begin_shape_change(self, what: str) -> ShapeEdit:
        self._may(what, "shapes", " (its ids name the shapes as they are now)")
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
        self._may("update_shapes", "shapes")
        edit, self._shape_edit = self._shape_edit, ShapeEdit()
        if edit.empty():
            return edit
        abi, keep = edit.to_abi()
        _host_call(host.vpth_scene_edit_shapes, self.handle, abi.remove_ids, abi.num_remove, abi.set_ids, abi.set, abi.num_set, abi.add, abi.num_add)
        del keep
        return edit

    # -- subdivision surfaces (the host side of vpt_scene_attach_subdiv / vpt_scene_update_subdivs): the scene keeps the cages it was
    #    tesselated from.  set_subdiv edits a cage or a setting and runs the mirror's tesselate_surface; a change of cage positions or
    #    displacement is noted in the pending SubdivEdit, which update_subdivs() hands out after update_bvh and make_lights; a change of
    #    subdivisions or smooth - or any that gives the shape other counts or pools - is noted as a `set` of the pending ShapeEdit ------
    _SUBDIV_CAGE = {"positions": (0, np.float32, 3), "normals": (1, np.float32, 3), "texcoords": (2, np.float32, 2),
                    "quadspos": (3, np.int32, 4), "quadsnorm": (4, np.int32, 4), "quadstexcoord": (5, np.int32, 4)}

    def _subdiv_item(self, index: int, kind: int, dtype, width: int) -> np.ndarray:
        a = _filled(lambda ptr, n: host.vpth_scene_subdiv_plan_item(self.handle, index, kind, ptr, n), lambda n: np.zeros(n // 4, dtype),
                    f"subdiv {index}: out of range, or its shape was removed")
        return a.reshape((-1, width) if width else (-1,))

    def subdiv(self, index: int) -> dict:
        """subdiv `index` as the scene keeps it: id, shape, subdivisions, smooth, catmullclark, displacement, displacement_tex and the
        cage - positions, normals (n, 3), texcoords (n, 2) float32, quadspos, quadsnorm, quadstexcoord (m, 4) int32 (copies)"""
        settings, displacement = np.zeros(5, np.int32), C.c_float()
        if host.vpth_scene_get_subdiv(self.handle, index, settings.ctypes.data, C.byref(displacement)) != 0:
            raise VptError(f"subdiv {index} out of range")
        out = {"id": index, "shape": int(settings[0]), "subdivisions": int(settings[1]), "smooth": bool(settings[2]), "catmullclark": bool(settings[3]),
               "displacement": displacement.value, "displacement_tex": int(settings[4])}
        out.update({name: self._subdiv_item(index, kind, dtype, width) for name, (kind, dtype, width) in self._SUBDIV_CAGE.items()})
        return out

    def subdivs(self) -> list:
        """every subdiv of the scene, as subdiv() returns it"""
        return [self.subdiv(i) for i in range(host.vpth_scene_subdiv_count(self.handle))]

    def subdiv_plan(self, index: int) -> SubdivPlan:
        """the tesselation plan of subdiv `index` as it is now (include/vpt.h: vpt_subdiv_plan), recorded by the mirror's own
        tesselate_surface: what DeviceScene attaches before the subdiv's first edit"""
        s = self.subdiv(index)
        levels = [{name: self._subdiv_item(index, 16 + 8 * l + k, np.int32, width) for k, (name, width) in enumerate(LEVEL_TABLES.items(), 1)}
                  for l in range(s["subdivisions"])]
        normals = s["normals"] if len(s["quadsnorm"]) else s["normals"][:0]   # (normals no face names are not the shape's)
        return SubdivPlan(s["shape"], s["subdivisions"], s["smooth"], s["displacement"], s["displacement_tex"], s["positions"], normals, levels,
                          self._subdiv_item(index, 7, np.int32, 4), self._subdiv_item(index, 6, np.int32, 3))

    def set_subdiv(self, index: int, positions=None, displacement: Optional[float] = None, subdivisions: Optional[int] = None,
                   smooth: Optional[bool] = None) -> None:
        """the cage's positions ((n, 3), same count), the displacement amount, the level or the smooth flag of subdiv `index` (None: as it
        is): the mirror re-tesselates its shape at once.  positions / displacement are applied to a resident scene by update_subdivs()
        and DeviceScene.update_subdivs; subdivisions / smooth change the shape's counts or pools and leave through update_shapes() as a
        `set` of the shape - so does a displacement switched between zero and non-zero where that adds or drops the shape's normals."""
        s = self.subdiv(index)
        if s["shape"] < 0:
            raise VptError(f"set_subdiv: the shape of subdiv {index} was removed")
        amount = s["displacement"] if displacement is None else float(displacement)
        normals_now = lambda d: s["smooth"] if d != 0 and s["displacement_tex"] >= 0 else len(s["quadsnorm"]) > 0
        reshapes = subdivisions is not None or smooth is not None or (s["subdivisions"] == 0 and normals_now(amount) != normals_now(s["displacement"]))
        if reshapes:
            pend = self._begin_shape_change("set_subdiv")
            if s["shape"] in pend.remove:
                raise VptError(f"set_subdiv: shape {s['shape']} is also removed")
        else:
            self._may("set_subdiv", "vertices")
        if positions is not None:
            positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
            if positions.shape != s["positions"].shape:
                raise VptError(f"set_subdiv: the cage of subdiv {index} has {len(s['positions'])} positions, got {len(positions)}")
        resized = C.c_int(0)
        _host_call(host.vpth_scene_set_subdiv, self.handle, index, None if positions is None else positions.ctypes.data,
                   C.c_float(np.nan if displacement is None else displacement), -1 if subdivisions is None else int(subdivisions),
                   -1 if smooth is None else int(bool(smooth)), C.byref(resized))
        if resized.value or reshapes:
            arrays = self.shape_arrays(s["shape"])
            self._shape_edit.set[s["shape"]] = self._check_mesh("set_subdiv", mesh(**arrays))
            return
        was = self._subdiv_edit.subdivs.get(index, (None, None))
        self._subdiv_edit.subdivs[index] = (was[0] if positions is None else positions.copy(), was[1] if displacement is None else float(displacement))
        self._subdiv_edit.shape_of[index] = s["shape"]

    def update_subdivs(self) -> SubdivEdit:
        """update_bvh and make_lights of the host library over the shapes set_subdiv re-tesselated since the last call: desc / stats()
        describe the edited scene afterwards.  Returns the SubdivEdit for DeviceScene.update_subdivs."""
        edit, self._subdiv_edit = self._subdiv_edit, SubdivEdit()
        if edit.empty():
            return edit
        _host_call(host.vpth_scene_update_bvh, self.handle)
        _host_call(host.vpth_scene_update_lights, self.handle)
        edit.plan_of = self.subdiv_plan
        return edit

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
        _host_call(host.vpth_scene_set_environment, self.handle, index, C.byref(env))
        self._texture_edit.environments[index] = self.environment(index)

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
        _host_call(host.vpth_scene_set_texture, self.handle, index, texels.shape[1], texels.shape[0], int(bool(linear)),
                   int(texels.dtype == np.float32), texels.ctypes.data)
        self._texture_edit.textures[index] = (texels.copy(), bool(linear))

    def update_textures(self) -> TextureEdit:
        """make_lights of the scene as set_environment / set_texture left it: desc, lights() and stats() carry the edited textures,
        environments, light list and CDFs.  Returns the TextureEdit for DeviceScene.update_textures."""
        _host_call(host.vpth_scene_update_textures, self.handle)
        edit, self._texture_edit = self._texture_edit, TextureEdit()
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
        self._may("set_volume_instance", "volume_entries")
        vi = self.volume_instance(index)
        if frame is not None:
            C.memmove(C.byref(vi.frame), np.ascontiguousarray(frame, np.float32).reshape(12).ctypes.data, 48)
        if volume is not None:
            vi.volume = int(volume)
        if material is not None:
            vi.material = int(material)
        if scalef is not None:
            vi.scalef = float(scalef)
        _host_call(host.vpth_scene_set_vol_instance, self.handle, index, C.byref(vi))
        self._volume_edit.vol_instances[index] = self.volume_instance(index)

    def sdf(self, index: int) -> VptSdf:
        out = VptSdf()
        if host.vpth_scene_get_sdf(self.handle, index, C.byref(out)) != 0:
            raise VptError(f"sdf {index} out of range")
        return out

    def set_sdf(self, index: int, sdf: Optional[VptSdf] = None, frame=None, type=None, material=None, whd=None, p=None) -> None:
        """an analytic SDF: a whole VptSdf, or the named fields of the one the scene holds (type: an index into SDF_TYPES or its name)"""
        self._may("set_sdf", "volume_entries")
        f = self._sdf_of(self.sdf(index) if sdf is None else sdf, frame, type, material, whd, p)
        _host_call(host.vpth_scene_set_sdf, self.handle, index, C.byref(f))
        self._volume_edit.sdfs[index] = self.sdf(index)

    @staticmethod
    def _sdf_of(f: VptSdf, frame=None, type=None, material=None, whd=None, p=None) -> VptSdf:
        """f with the named fields replaced (type: an index into SDF_TYPES or its name)"""
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
        return f

    def _write_volume(self, index: int, src: VolumeSource, voxels: np.ndarray) -> None:
        whd, lo, size = (np.array([int(v) for v in a], np.int32) for a in (src.whd, src.region_lo, src.region_whd))
        voxels = np.ascontiguousarray(voxels, np.float32)
        _host_call(host.vpth_scene_set_volume, self.handle, index, whd.ctypes.data, C.c_float(src.res), lo.ctypes.data, size.ctypes.data,
                   int(src.mode), voxels.ctypes.data)

    def _note_volume(self, index: int, src: VolumeSource) -> None:
        self._may("set_volume / bake_volume", "volume_entries")
        if index in self._volume_edit.volumes:
            raise VptError(f"volume {index} is already in the pending edit: hand it out with update_volumes() first")
        if any(e.volume == index for e in self._sculpt_edit.entries):
            raise VptError(f"volume {index} has sculpts pending: hand them out with update_sculpts() first")
        self._volume_edit.volumes[index] = src

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
            del self._volume_edit.volumes[index]   # refused: nothing was written, nothing is pending
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
        self._lazy_bakes.append((index, src))

    def _run_bakes(self) -> None:
        """the host copy of the volumes bake_volume named: the host mirror of the bake, run when the copy is read"""
        todo, self._lazy_bakes = self._lazy_bakes, []
        for index, src in todo:
            positions, triangles, origin, step = src.bake
            grid, _ = bake_sdf_grid(positions, triangles, src.whd, origin, step, device=None)
            lo, size = src.region_lo, src.region_whd
            box = grid[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]]
            self._write_volume(index, src, box)
        if todo:
            _host_call(host.vpth_scene_update_volumes, self.handle)

    def update_volumes(self) -> VolumeEdit:
        """make_lights of the scene as set_volume_instance / set_sdf / set_volume / bake_volume left it: desc, lights() and stats() carry
        the edited volumes, instances, SDFs, light list and CDFs.  Returns the VolumeEdit for DeviceScene.update_volumes."""
        _host_call(host.vpth_scene_update_volumes, self.handle)
        edit, self._volume_edit = self._volume_edit, VolumeEdit()
        return edit

    # -- the set of volumes, grid instances and SDFs (the host side of vpt_scene_update_volume_set): the add_* / remove_* calls note a
    #    change, removals naming the lists as they are now; update_volume_set() applies them to the scene - remove, then add - runs
    #    make_lights and hands the VolumeSetEdit out.  The ids of a pending VolumeEdit or SculptEdit name the old lists, so the two kinds of
    #    change do not mix: each is handed out before the other begins --------------------------------------------------------------------
    def _begin_volume_set_change(self, what: str) -> VolumeSetEdit:
        self._may(what, "volume_set")
        return self._volume_set_edit

    def _note_removals(self, what: str, kind: str, pending: tuple, ids) -> tuple:
        ids = [int(i) for i in ids]
        for i in ids:
            if not 0 <= i < self.count_implicit(kind):
                raise VptError(f"{what}: id {i} out of range")
        if len(set(ids)) != len(ids) or set(ids) & set(pending):
            raise VptError(f"{what}: an id is repeated")
        return pending + tuple(ids)

    def add_volume(self, voxels=None, *, bake=None, fill=None, copy_of=None, whd=None, res=None) -> int:
        """notes a new volume, appended at update_volume_set(); returns the id it has afterwards (given the removals noted so far).
        Exactly one source: voxels, float32 of shape (d, h, w); bake = (positions, faces) or (positions, faces, origin, step), a mesh baked
        on the device by the rule of vpt_bake_sdf into a grid of `whd` (origin / step: bake_volume's defaults) - the host copy runs the
        host mirror of the bake only when it is read; fill, a float every voxel of `whd` gets; copy_of, a current volume id whose voxels
        the new volume starts with.  res: the volume's (copy_of: the source's unless given)."""
        pend = self._begin_volume_set_change("add_volume")
        if sum(x is not None for x in (voxels, bake, fill, copy_of)) != 1:
            raise VptError("add_volume: exactly one of voxels, bake, fill and copy_of says where the voxels come from")
        if copy_of is not None:
            whd, old_res = self._volume_shape(int(copy_of))
            new = VolumeNew(whd, old_res if res is None else float(res), VOLUME_COPY, copy_of=int(copy_of))
        else:
            if res is None or not np.isfinite(res):
                raise VptError("add_volume: a finite res is needed")
            if voxels is not None:
                voxels = np.ascontiguousarray(voxels, np.float32)
                if voxels.ndim != 3 or (whd is not None and tuple(int(v) for v in _whd3(whd)) != voxels.shape[::-1]):
                    raise VptError(f"add_volume: expected (d, h, w) voxels of whd, got {voxels.shape}")
                new = VolumeNew(voxels.shape[::-1], float(res), VOLUME_FROM_HOST, voxels=voxels.copy())
            else:
                if whd is None:
                    raise VptError("add_volume: a baked or filled volume needs whd")
                whd = tuple(int(v) for v in _whd3(whd))
                if min(whd) < 0 or whd[0] * whd[1] * whd[2] >= 2 ** 31:
                    raise VptError(f"add_volume: bad whd {whd}")
                if fill is not None:
                    new = VolumeNew(whd, float(res), VOLUME_FILL, fill=fill)
                else:
                    positions, faces = bake[0], bake[1]
                    origin = np.zeros(3, np.float32) if len(bake) < 3 or bake[2] is None else bake[2]
                    step = (np.array([np.float32(res) * np.float32(w) / np.float32(max(1, w - 1)) for w in whd], np.float32)
                            if len(bake) < 4 or bake[3] is None else bake[3])
                    positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3).copy()
                    new = VolumeNew(whd, float(res), VOLUME_FROM_BAKE, bake=(positions, bake_triangles(faces), np.asarray(origin, np.float32).copy(),
                                                                              np.asarray(step, np.float32).copy()))
        pend.add_volumes.append(new)
        return self.count_implicit("volumes") - len(pend.remove_volumes) + len(pend.add_volumes) - 1

    def _volume_shape(self, index: int):
        """((w, h, d), res) of volume `index` without a copy of its voxels; a pending bake of that volume runs first (it may change both)"""
        if any(k == index for k, _ in self._lazy_bakes):
            self._run_bakes()
        whd, res = np.zeros(3, np.int32), C.c_float()
        if host.vpth_scene_get_volume(self.handle, index, whd.ctypes.data, C.byref(res), None, 0) < 0:
            raise VptError(f"volume {index} out of range")
        return tuple(int(v) for v in whd), res.value

    def remove_volumes(self, ids) -> None:
        """notes volumes (current ids) to erase at update_volume_set(): the survivors keep their order, the ids close up and the grid
        instances' volume ids follow.  No grid instance that stays or is added may name a removed volume: update_volume_set() refuses it."""
        pend = self._begin_volume_set_change("remove_volumes")
        pend.remove_volumes = self._note_removals("remove_volumes", "volumes", pend.remove_volumes, ids)

    def add_volume_instance(self, frame, volume: int, material: int, scalef: float = 1) -> int:
        """notes a new grid instance, appended at update_volume_set(); `volume` is an id of the list as update_volume_set() leaves it (what
        add_volume returned, or a survivor's new id).  Returns the id the instance has afterwards."""
        pend = self._begin_volume_set_change("add_volume_instance")
        frame = np.ascontiguousarray(frame, np.float32).reshape(-1)
        if frame.size != 12 or not np.all(np.isfinite(frame)) or not np.isfinite(scalef):
            raise VptError("add_volume_instance: a frame is twelve finite floats (x, y, z, o), scalef a finite one")
        if not 0 <= int(volume) < self.count_implicit("volumes") - len(pend.remove_volumes) + len(pend.add_volumes):
            raise VptError(f"add_volume_instance: volume {volume} out of range of the list after the edit")
        if not 0 <= int(material) < self.count("materials"):
            raise VptError(f"add_volume_instance: material {material} out of range")
        vi = VptVolumeInstance(volume=int(volume), material=int(material), scalef=float(scalef))
        C.memmove(C.byref(vi.frame), frame.ctypes.data, 48)
        pend.add_vol_instances.append(vi)
        return self.count_implicit("vol_instances") - len(pend.remove_vol_instances) + len(pend.add_vol_instances) - 1

    def remove_volume_instances(self, ids) -> None:
        """notes grid instances (current ids) to erase at update_volume_set()"""
        pend = self._begin_volume_set_change("remove_volume_instances")
        pend.remove_vol_instances = self._note_removals("remove_volume_instances", "vol_instances", pend.remove_vol_instances, ids)

    def add_sdf(self, sdf: Optional[VptSdf] = None, frame=None, type=None, material=None, whd=None, p=None) -> int:
        """notes a new analytic SDF, appended at update_volume_set(): a whole VptSdf, or one made of the named fields as set_sdf takes them
        (frame: identity unless given).  Returns the id it has afterwards."""
        pend = self._begin_volume_set_change("add_sdf")
        f = VptSdf()
        if sdf is not None:
            C.memmove(C.byref(f), C.byref(sdf), C.sizeof(VptSdf))
        else:
            C.memmove(C.byref(f.frame), np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32).ctypes.data, 48)
        f = self._sdf_of(f, frame, type, material, whd, p)
        floats = np.frombuffer(bytes(f), np.float32)
        if not (np.all(np.isfinite(floats[:12])) and np.all(np.isfinite(floats[14:21]))):
            raise VptError("add_sdf: a value is not finite")
        if not 0 <= f.type < len(SDF_TYPES) or not 0 <= f.material < self.count("materials"):
            raise VptError(f"add_sdf: type {f.type} or material {f.material} out of range")
        pend.add_sdfs.append(f)
        return self.count_implicit("sdfs") - len(pend.remove_sdfs) + len(pend.add_sdfs) - 1

    def remove_sdfs(self, ids) -> None:
        """notes analytic SDFs (current ids) to erase at update_volume_set(); a light SDF behind them follows the new numbering"""
        pend = self._begin_volume_set_change("remove_sdfs")
        pend.remove_sdfs = self._note_removals("remove_sdfs", "sdfs", pend.remove_sdfs, ids)

    def update_volume_set(self) -> VolumeSetEdit:
        """the host side of vpt_scene_update_volume_set over what the add_* / remove_* calls noted since the last call: erase / push_back
        on the scene's volumes, grid instances and SDFs, the instances' volume ids renumbered, make_lights; desc, lights() and stats()
        describe the edited scene afterwards.  A baked addition holds zeros until the host copy is read (_run_bakes); a bake still
        pending from before follows its volume to the new id, is dropped with a volume that goes, and runs first only where the edit
        copies its volume.  Returns the VolumeSetEdit for DeviceScene.update_volume_set; an edit the host library refuses stays pending
        and changes nothing."""
        self._may("update_volume_set", "volume_set")
        edit = self._volume_set_edit
        if edit.empty():
            return edit
        if {k for k, _ in self._lazy_bakes} & {n.copy_of for n in edit.add_volumes if n.source == VOLUME_COPY}:
            self._run_bakes()
        count = self.count_implicit("volumes")
        abi, keep = edit.to_abi()
        _host_call(host.vpth_scene_edit_volume_set, self.handle, C.byref(abi))
        del keep
        self._volume_set_edit = VolumeSetEdit()
        kept = [k for k in range(count) if k not in edit.remove_volumes]   # new id -> old id of the survivors
        self._lazy_bakes = [(kept.index(k), src) for k, src in self._lazy_bakes if k in kept]
        first = self.count_implicit("volumes") - len(edit.add_volumes)
        for k, new in enumerate(edit.add_volumes):
            if new.source == VOLUME_FROM_BAKE:
                self._lazy_bakes.append((first + k, VolumeSource(tuple(new.whd), new.res, (0, 0, 0), tuple(new.whd), VOXELS_REPLACE, None, new.bake)))
        return edit

    # -- sculpting (the host side of vpt_scene_sculpt_volumes): sculpt_volume applies a stroke to the scene's copy through the host mirror
    #    at once and notes it in the pending SculptEdit, which update_sculpts() hands out ----------------------------------------------
    def sculpt_volume(self, index: int, stamps, region=None, origin=None, step=None) -> SculptEntry:
        """a stroke - Stamps in order - over the voxels of volume `index` by the rule of vpt_scene_sculpt_volumes: each voxel (i, j, k)
        of the region is sampled at origin + (i, j, k) * step and taken through every stamp.  region None: the whole grid, else (lo, whd),
        each (x, y, z); origin / step None: bake_volume's defaults (origin 0, step = res * W / (W - 1) per axis: the grid's local frame
        divided by scalef).  Returns the entry it noted.  A refused call changes nothing."""
        index = int(index)
        self._may("sculpt_volume", "volume_entries")
        if index in self._volume_edit.volumes:
            raise VptError(f"sculpt_volume: volume {index} is in the pending volume edit: hand it out with update_volumes() first")
        old, res = self.volume(index)
        whd = old.shape[::-1]
        if origin is None:
            origin = np.zeros(3, np.float32)
        if step is None:
            step = np.array([np.float32(res) * np.float32(w) / np.float32(max(1, w - 1)) for w in whd], np.float32)
        lo, size = ((0, 0, 0), whd) if region is None else region
        stamps = [s if isinstance(s, Stamp) else Stamp(*s) for s in stamps]
        entry = SculptEntry(index, tuple(int(v) for v in lo), tuple(int(v) for v in size),
                            tuple(float(v) for v in np.broadcast_to(np.asarray(origin, np.float32), (3,))),
                            tuple(float(v) for v in np.broadcast_to(np.asarray(step, np.float32), (3,))), stamps)
        abi, keep = SculptEdit([entry]).to_abi()
        _host_call(host.vpth_scene_sculpt_volume, self.handle, C.cast(abi.entries, C.POINTER(VptSculptEntry)), abi.stamps, abi.num_stamps)
        del keep
        self._sculpt_edit.entries.append(entry)
        return entry

    def update_sculpts(self) -> SculptEdit:
        """the flattened descriptor of the scene as sculpt_volume left it (no light, no record changes: whd and res stay).  Returns the
        SculptEdit for DeviceScene.sculpt_volumes."""
        _host_call(host.vpth_scene_update_volumes, self.handle)
        edit, self._sculpt_edit = self._sculpt_edit, SculptEdit()
        return edit

    def volgrid_majorants(self, index: int) -> np.ndarray:
        """the host mirror of DeviceScene.volgrid_majorants on the scene's copy of volume `index` (pending bakes run first): the volgrid
        shader's brick majorants, float32 of shape (nbz, nby, nbx)"""
        dims = (C.c_int32 * 3)()
        _host_call(host.vpth_volgrid_majorants, self.desc, index, None, 0, C.cast(dims, C.c_void_p))
        out = np.zeros((dims[2], dims[1], dims[0]), np.float32)
        _host_call(host.vpth_volgrid_majorants, self.desc, index, out.ctypes.data, out.size, None)
        return out

    def volgrid_density(self, points):
        """the host mirror of DeviceScene.volgrid_density: (sigma, instance) at world points ((n, 3) float32) of the scene as it stands"""
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        sigma, instance = np.zeros(len(points), np.float32), np.full(len(points), -1, np.int32)
        _host_call(host.vpth_volgrid_density, self.desc, len(points), points.ctypes.data, instance.ctypes.data, sigma.ctypes.data)
        return sigma, instance

    def mesh_volume(self, index: int, iso: float = 0.0, origin=None, step=None, region=None, stats: Optional[dict] = None) -> dict:
        """the host mirror of DeviceScene.mesh_volume on the scene's copy of volume `index` (pending bakes run first, as for volume()):
        mesh_sdf(device=None) with bake_volume's defaults - origin 0, step = res * W / (W - 1) per axis"""
        voxels, res = self.volume(index)
        if origin is None:
            origin = np.zeros(3, np.float32)
        if step is None:
            step = np.array([np.float32(res) * np.float32(w) / np.float32(max(1, w - 1)) for w in voxels.shape[::-1]], np.float32)
        return mesh_sdf(voxels, origin, step, iso, device=None, region=region, stats=stats)

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
