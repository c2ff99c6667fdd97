"""The device side: the render parameters and state, DeviceScene (one GPU), AdaptiveRun, MultiDeviceScene (several GPUs of this
process), and the helpers over device-resident state, layouts and resolves."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import TYPE_CHECKING, Optional

import numpy as np

from ._abi import (AOV_PLANES, BVH_NODE, INSTANCE, LIGHT, SDF_AOV_PLANES, SHADER_NAMES, VptAdaptive, VptAovPlanes, VptSdfAovPlanes, VptDisplay, VptError, VptLayout, VptParams,
                   VptSdf, VptVolume, VptVolumeInstance, _Handle, _check, shader_id, _counted, _edit_call, _mesh_desc, _mesh_region, _meshed, _p, hip, host)
from .edits import BvhRebuild, InstanceEdit, SceneEdit, SculptEdit, ShapeEdit, SubdivEdit, SubdivPlan, TextureEdit, VolumeEdit, VolumeSetEdit, mesh

if TYPE_CHECKING:
    from .host_scene import HostScene


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
        return VptParams(self.camera, self.resolution, shader_id(self.shader), self.samples,   # an unknown name: VptError("sampler unknown")
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


def device_count() -> int:
    return hip.vpt_device_count()


def _attach_subdiv(owner, attach, index: int, plan: SubdivPlan) -> int:
    """`plan` attached through vpt_scene_attach_subdiv / vpt_multi_attach_subdiv on owner.handle; owner._subdiv_ids[index] = its id there"""
    abi, keep = plan.to_abi()
    out = C.c_int(-1)
    _check(attach(owner.handle, C.byref(abi), C.byref(out)), "vpt_scene_attach_subdiv")
    del keep
    owner._subdiv_ids[int(index)] = out.value
    return out.value


def _subdiv_edit_call(owner, attach, shape_of_plan, handle, name: str, edit: SubdivEdit) -> None:
    """the edit entry point `name` on `handle` (a scene, multi-device scene or session) with a SubdivEdit: every named subdiv whose plan
    the scene behind `owner` (a DeviceScene or MultiDeviceScene) does not hold - never attached, or dropped since by update_shapes -
    is attached first, then the edit goes out under the plans' ids"""
    for index in edit.subdivs:
        have = owner._subdiv_ids.get(index)
        if have is None or shape_of_plan(owner.handle, have) != edit.shape_of.get(index, -2):
            if edit.plan_of is None:
                raise VptError(f"{name}: subdiv {index} has no plan on the device and the edit names no source of one (attach_subdiv first)")
            _attach_subdiv(owner, attach, index, edit.plan_of(index))
    abi, keep = edit.to_abi(owner._subdiv_ids)
    _check(getattr(hip, name)(handle, C.byref(abi)), name)
    del keep


class DeviceScene(_Handle):
    """vpt_scene: the scene resident in one GPU's HBM."""
    _free = staticmethod(hip.vpt_scene_destroy)

    def __init__(self, scene: HostScene, device: int = 0):
        self.host_scene = scene  # keep the flattened arrays alive until the upload finished
        out = _p()
        _check(hip.vpt_scene_create_curves(scene.desc, scene.curves, device, C.byref(out)), "vpt_scene_create")
        self.handle = out
        self.device = device
        self._subdiv_ids = {}   # subdiv of the host scene -> the id of its plan on the device (attach_subdiv)

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

    def render_sdf_aov_device(self, params: PathtraceParams, layout: VptLayout, nsamples: int, planes: dict, d_hits: int, d_rng: int,
                              stream: int = 0) -> None:
        """vpt_render_sdf_aov_device on this rank's tile-major slots: `planes` maps names of SDF_AOV_PLANES to raw device pointers"""
        unknown = set(planes) - set(SDF_AOV_PLANES)
        if unknown:
            raise VptError(f"unknown SDF AOV plane {sorted(unknown)[0]!r}: expected one of {SDF_AOV_PLANES}")
        abi, pl = params.to_abi(), VptSdfAovPlanes(**{k: v for k, v in planes.items() if v})
        _check(hip.vpt_render_sdf_aov_device(self.handle, C.byref(abi), C.byref(layout), nsamples, C.byref(pl), d_hits, d_rng, stream),
               "vpt_render_sdf_aov_device")

    def render_sdf_aovs(self, state: PathtraceState, params: PathtraceParams, nsamples: int = 1, planes=SDF_AOV_PLANES,
                        into: Optional[dict] = None) -> dict:
        """the sphere-traced first-hit pass (vpt_render_sdf_aov, include/vpt.h) over the hits / rngs of `state` (its image is left alone):
        `nsamples` more samples, at most params.samples in all, every camera ray marched once for every plane named in `planes`.  Returns
        {name: array}: the sums normal / albedo / depth as (h, w, 4) float32 - divide by state.samples, as get_render does - and ids
        (h, w, 2) int32 {vol_instance, sdf}, hit (h, w, 4) float32 {position, t} of the state's first sample.  `into`: the dict an earlier
        call returned, to go on from (batching is exact)."""
        out = {}
        for name in planes:
            if name not in SDF_AOV_PLANES:
                raise VptError(f"unknown SDF AOV plane {name!r}: expected one of {SDF_AOV_PLANES}")
            tail, dtype = ((2,), np.int32) if name == "ids" else ((4,), np.float32)
            shape = (state.height, state.width) + tail
            a = into.get(name) if into else None
            if a is None:
                a = np.zeros(shape, dtype)
            elif a.shape != shape or a.dtype != dtype or not a.flags["C_CONTIGUOUS"]:
                raise VptError(f"plane {name!r}: expected a contiguous {np.dtype(dtype).name} array of shape {shape}")
            out[name] = a
        for a in (state.hits, state.rngs):
            assert a.flags["C_CONTIGUOUS"]
        abi, pl, samples = params.to_abi(), VptSdfAovPlanes(**{k: a.ctypes.data for k, a in out.items()}), C.c_int(state.samples)
        _check(hip.vpt_render_sdf_aov(self.handle, C.byref(abi), nsamples, state.width, state.height, C.byref(pl), state.hits.ctypes.data,
                                      state.rngs.ctypes.data, C.byref(samples)), "vpt_render_sdf_aov")
        state.samples = samples.value
        return out

    def update(self, edit: SceneEdit) -> None:
        """vpt_scene_update (include/vpt.h): the edit applied to the resident scene, BVHs refitted on the device.  Afterwards the
        handle renders the bits of a DeviceScene made from the host scene after the same edit and update_bvh()."""
        _edit_call(self.handle, "vpt_scene_update", edit)

    def update_lights(self, edit: SceneEdit) -> None:
        """vpt_scene_update_lights (include/vpt.h): update() for an edit that may switch a material's emission between zero and non-zero
        or move the vertices of an emitter; the light tables are rebuilt on the device.  Afterwards the handle renders the bits of a
        DeviceScene made from the host scene after the same edit and update_lights()."""
        _edit_call(self.handle, "vpt_scene_update_lights", edit)

    def update_textures(self, edit: TextureEdit) -> None:
        """vpt_scene_update_textures (include/vpt.h): environments' emission and texture, and textures' texels; an environment's CDF
        is rebuilt on the device from the texels.  Afterwards the handle renders the bits of a DeviceScene made from the host scene
        after the same edit and update_textures()."""
        _edit_call(self.handle, "vpt_scene_update_textures", edit)

    def update_volumes(self, edit: VolumeEdit) -> None:
        """vpt_scene_update_volumes (include/vpt.h): grid instances, SDFs and volumes' voxels, from the host or baked on the device into
        the resident pool.  Afterwards the handle renders the bits of a DeviceScene made from the host scene after the same edit and
        update_volumes()."""
        _edit_call(self.handle, "vpt_scene_update_volumes", edit)

    def update_volume_set(self, edit: VolumeSetEdit) -> None:
        """vpt_scene_update_volume_set (include/vpt.h): volumes, grid instances and SDFs removed and added - the voxel pool laid out anew
        by one gather on the device, baked additions written into it by the bake kernel, the lights following the SDFs - with the
        VolumeSetEdit of HostScene.update_volume_set()."""
        _edit_call(self.handle, "vpt_scene_update_volume_set", edit)

    def sculpt_volumes(self, edit: SculptEdit) -> None:
        """vpt_scene_sculpt_volumes (include/vpt.h): strokes of analytic brushes evaluated on the device over boxes of the resident voxels -
        a few hundred bytes cross PCIe, not one voxel.  edit: what HostScene.update_sculpts() returns."""
        _edit_call(self.handle, "vpt_scene_sculpt_volumes", edit)

    def get_volumes(self):
        """(volumes, vol_instances, sdfs) as the device holds them, ctypes arrays of VptVolume, VptVolumeInstance, VptSdf
        (vpt_scene_get_volumes); a volume's offset is the resident pool's"""
        counts = (C.c_int32 * 3)()   # the handle's own: update_volume_set changes them
        _check(hip.vpt_scene_count_implicit(self.handle, C.cast(counts, _p)), "vpt_scene_count_implicit")
        nv, ni, ns = counts
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

    def volgrid_majorants(self, index: int) -> np.ndarray:
        """the brick majorants of volume `index` as the device holds them for the volgrid shader (vpt_scene_get_volgrid_majorants), built
        or rebuilt first when the scene was edited since: float32 of shape (nbz, nby, nbx) - the bits of HostScene.volgrid_majorants"""
        dims = (C.c_int32 * 3)()
        _check(hip.vpt_scene_get_volgrid_majorants(self.handle, index, None, 0, C.cast(dims, _p)), "vpt_scene_get_volgrid_majorants")
        out = np.zeros((dims[2], dims[1], dims[0]), np.float32)
        _check(hip.vpt_scene_get_volgrid_majorants(self.handle, index, out.ctypes.data, out.size, None), "vpt_scene_get_volgrid_majorants")
        return out

    def volgrid_density(self, points):
        """the volgrid shader's extinction at world points ((n, 3) float32), evaluated on the device (vpt_scene_volgrid_density): (sigma,
        instance) = (n,) float32 sums over the grid instances in index order, (n,) int32 first instance whose box holds the point or -1 -
        the bits of HostScene.volgrid_density"""
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        sigma, instance = np.zeros(len(points), np.float32), np.full(len(points), -1, np.int32)
        _check(hip.vpt_scene_volgrid_density(self.handle, len(points), points.ctypes.data, instance.ctypes.data, sigma.ctypes.data),
               "vpt_scene_volgrid_density")
        return sigma, instance

    def volgrid_track(self, rays, rngs):
        """the volgrid shader's free flight on given world rays ((n, 6) float32: origin, unit direction) with given PCG32 streams ((n, 2)
        uint64: state, inc), flown by the kernel's own tracking functions (vpt_scene_volgrid_track): (event, instance, t, steps, rngs_out)
        = (n,) int32 0 escape / 1 collision / 2 step bound, (n,) int32 the collision's grid instance or -1, (n,) float32 its world
        parameter or FLT_MAX, (n,) int32 tracking steps, (n, 2) uint64 the streams after the flight"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        rngs = np.ascontiguousarray(rngs, np.uint64).reshape(-1, 2)
        if len(rays) != len(rngs):
            raise VptError(f"volgrid_track: {len(rays)} rays but {len(rngs)} streams")
        n = len(rays)
        event, instance, steps = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
        t, rngs_out = np.zeros(n, np.float32), np.zeros((n, 2), np.uint64)
        _check(hip.vpt_scene_volgrid_track(self.handle, n, rays.ctypes.data, rngs.ctypes.data, event.ctypes.data, instance.ctypes.data, t.ctypes.data,
                                           steps.ctypes.data, rngs_out.ctypes.data), "vpt_scene_volgrid_track")
        return event, instance, t, steps, rngs_out

    def volgrid_stats(self) -> dict:
        """vpt_scene_volgrid_stats: tracking steps of this handle's volgrid launches so far, builds of its brick tables so far"""
        steps, builds = C.c_uint64(0), C.c_int32(0)
        _check(hip.vpt_scene_volgrid_stats(self.handle, C.byref(steps), C.byref(builds)), "vpt_scene_volgrid_stats")
        return {"steps": steps.value, "table_builds": builds.value}

    def mesh_volume(self, index: int, iso: float = 0.0, origin=None, step=None, region=None, stats: Optional[dict] = None) -> dict:
        """vpt_scene_mesh_volume (include/vpt.h): the iso surface of volume `index` as a quad mesh, made on the device from the voxels where
        they lie in the resident pool - no voxel crosses PCIe, nothing of the scene changes.  origin / step None: bake_volume's defaults
        (origin 0, step = res * W / (W - 1) per axis: the grid's local frame divided by scalef).  region = (lo, whd), each (x, y, z): that
        box meshed as a grid of its own, its vertices in place.  Returns the mesh(...) dictionary HostScene.add_shape takes - the bits of
        mesh_sdf(get_voxels(index), ...) and of HostScene.mesh_volume.  stats: a dict that receives num_vertices, num_quads, launches,
        device_ms."""
        desc = None
        if not (iso == 0.0 and origin is None and step is None):
            vols, _, _ = self.get_volumes()
            if not 0 <= index < len(vols):
                raise VptError(f"volume {index} out of range")
            whd, res = tuple(vols[index].whd), np.float32(vols[index].res)
            if step is None:
                step = np.array([res * np.float32(w) / np.float32(max(1, w - 1)) for w in whd], np.float32)
            desc = _mesh_desc(whd, np.zeros(3, np.float32) if origin is None else origin, step, iso)
        box = _mesh_region(region)
        call = lambda *out: _check(hip.vpt_scene_mesh_volume(self.handle, index, C.byref(desc) if desc else None, C.byref(box) if box else None, *out),
                                   "vpt_scene_mesh_volume")
        m = _meshed(call, stats)
        return mesh(m["positions"], quads=m["quads"], normals=m["normals"])

    def get_lights(self):
        """(light list as a LIGHT array, CDF pool as float32) as the device holds them (vpt_scene_get_lights)"""
        n, m = C.c_int(0), C.c_int64(0)   # (two counts at once: not _counted's shape)
        _check(hip.vpt_scene_get_lights(self.handle, None, 0, C.byref(n), None, 0, C.byref(m)), "vpt_scene_get_lights")
        lights, cdf = np.zeros(n.value, LIGHT), np.zeros(m.value, np.float32)
        _check(hip.vpt_scene_get_lights(self.handle, lights.ctypes.data, len(lights), None, cdf.ctypes.data, len(cdf), None), "vpt_scene_get_lights")
        return lights, cdf

    def get_media(self):
        """the medium records of the device, float32 [materials, 12] (vpt_scene_get_media): density, scattering, emission, scanisotropy, 0, 0"""
        return _counted(hip.vpt_scene_get_media, self.handle, np.dtype((np.float32, 12)), "vpt_scene_get_media", None)

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
        _edit_call(self.handle, "vpt_scene_rebuild_bvh_quality", rebuild, rebuild.quality)

    def update_instances(self, edit: InstanceEdit) -> None:
        """vpt_scene_update_instances (include/vpt.h): instances re-pointed, removed and added on the device; the scene BVH and the
        lights follow.  Afterwards the handle renders the bits of a DeviceScene made from the host scene after the same
        HostScene.update_instances()."""
        _edit_call(self.handle, "vpt_scene_update_instances", edit)

    def update_shapes(self, edit: ShapeEdit) -> None:
        """vpt_scene_update_shapes (include/vpt.h): shapes replaced, removed and added on the device; pools, BVHs, instances and lights
        follow.  Afterwards the handle renders the bits of a DeviceScene made from the host scene after the same
        HostScene.update_shapes()."""
        _edit_call(self.handle, "vpt_scene_update_shapes", edit)

    def attach_subdiv(self, index: int, plan: SubdivPlan) -> int:
        """vpt_scene_attach_subdiv (include/vpt.h): the tesselation plan of the host scene's subdiv `index` uploaded once; nothing
        renders, no table of the scene changes.  Returns the plan's id on the device (update_subdivs keeps the map)."""
        return _attach_subdiv(self, hip.vpt_scene_attach_subdiv, index, plan)

    def detach_subdiv(self, index: int) -> None:
        """vpt_scene_detach_subdiv: frees the plan of the host scene's subdiv `index`"""
        _check(hip.vpt_scene_detach_subdiv(self.handle, self._subdiv_ids.pop(index)), "vpt_scene_detach_subdiv")

    def subdiv_count(self) -> int:
        """the plans attached (vpt_scene_subdiv_count)"""
        return hip.vpt_scene_subdiv_count(self.handle)

    def update_subdivs(self, edit: SubdivEdit) -> None:
        """vpt_scene_update_subdivs (include/vpt.h): the named subdivs tesselated again on the device from the edit's cages and
        displacements, into the resident vertex pools; refit and lights follow.  A named subdiv without a plan on the device gets one
        first (edit.plan_of).  Afterwards the handle renders the bits of a DeviceScene made from the host scene after the same
        HostScene.set_subdiv() and update_subdivs()."""
        _subdiv_edit_call(self, hip.vpt_scene_attach_subdiv, hip.vpt_scene_subdiv_shape, self.handle, "vpt_scene_update_subdivs", edit)

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
        return _counted(hip.vpt_scene_get_instances, self.handle, INSTANCE, "vpt_scene_get_instances")

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
        return _counted(hip.vpt_last_wave_costs, self.handle, np.uint32, "vpt_last_wave_costs")


class AdaptiveRun(_Handle):
    """vpt_adaptive_run (include/vpt.h): the round loop of an adaptive render on device-resident tile-major state, resumable.  The
    pointers are raw device addresses and stay the caller's."""
    _free = staticmethod(hip.vpt_adaptive_run_destroy)

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


def box3_device(width: int, height: int, d_in: int, d_out: int, stream: int = 0) -> None:
    """vpt_box3_device: the denoiser's box3 of a row-major float plane"""
    _check(hip.vpt_box3_device(width, height, d_in, d_out, stream), "vpt_box3_device")


class MultiDeviceScene(_Handle):
    """vpt_multi: the scene on several GPUs of this process, tiles dealt round-robin (include/vpt.h)."""
    _free = staticmethod(hip.vpt_multi_destroy)

    def __init__(self, scene: HostScene, devices):
        self.host_scene = scene
        devs = (C.c_int * len(devices))(*devices)
        out = _p()
        _check(hip.vpt_multi_create_curves(scene.desc, scene.curves, devs, len(devices), C.byref(out)), "vpt_multi_create")
        self.handle = out
        self._subdiv_ids = {}   # subdiv of the host scene -> the id of its plan on every device

    def attach_subdiv(self, index: int, plan: SubdivPlan) -> int:
        """vpt_multi_attach_subdiv: DeviceScene.attach_subdiv on every device (the same id on each)"""
        return _attach_subdiv(self, hip.vpt_multi_attach_subdiv, index, plan)

    def update_subdivs(self, edit: SubdivEdit) -> None:
        """vpt_multi_update_subdivs: DeviceScene.update_subdivs with the same edit on every device"""
        _subdiv_edit_call(self, hip.vpt_multi_attach_subdiv, hip.vpt_multi_subdiv_shape, self.handle, "vpt_multi_update_subdivs", edit)

    def update(self, edit: SceneEdit) -> None:
        """vpt_multi_update: the same edit on every device; the resident tile state is left as it is"""
        _edit_call(self.handle, "vpt_multi_update", edit)

    def update_lights(self, edit: SceneEdit) -> None:
        """vpt_multi_update_lights: DeviceScene.update_lights with the same edit on every device"""
        _edit_call(self.handle, "vpt_multi_update_lights", edit)

    def update_textures(self, edit: TextureEdit) -> None:
        """vpt_multi_update_textures: DeviceScene.update_textures with the same edit on every device"""
        _edit_call(self.handle, "vpt_multi_update_textures", edit)

    def update_volumes(self, edit: VolumeEdit) -> None:
        """vpt_multi_update_volumes: DeviceScene.update_volumes with the same edit on every device"""
        _edit_call(self.handle, "vpt_multi_update_volumes", edit)

    def update_volume_set(self, edit: VolumeSetEdit) -> None:
        """vpt_multi_update_volume_set: DeviceScene.update_volume_set with the same edit on every device"""
        _edit_call(self.handle, "vpt_multi_update_volume_set", edit)

    def sculpt_volumes(self, edit: SculptEdit) -> None:
        """vpt_multi_sculpt_volumes: DeviceScene.sculpt_volumes with the same edit on every device"""
        _edit_call(self.handle, "vpt_multi_sculpt_volumes", edit)

    def rebuild_bvh(self, rebuild: "BvhRebuild") -> None:
        """vpt_multi_rebuild_bvh: DeviceScene.rebuild_bvh on every device (each builds its own trees: equal by construction)"""
        _edit_call(self.handle, "vpt_multi_rebuild_bvh_quality", rebuild, rebuild.quality)

    def update_instances(self, edit: InstanceEdit) -> None:
        """vpt_multi_update_instances: DeviceScene.update_instances with the same edit on every device"""
        _edit_call(self.handle, "vpt_multi_update_instances", edit)

    def update_shapes(self, edit: ShapeEdit) -> None:
        """vpt_multi_update_shapes: DeviceScene.update_shapes with the same edit on every device"""
        _edit_call(self.handle, "vpt_multi_update_shapes", edit)

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


def resolve_sdf_ids_device(layout: VptLayout, d_ids_all: int, d_hit_all: Optional[int], d_ids_rows: int, d_hit_rows: Optional[int], stream: int = 0):
    """vpt_resolve_sdf_ids_device: the ids / hit planes of all ranks, tile-major -> row-major (the hit pair None together)"""
    _check(hip.vpt_resolve_sdf_ids_device(C.byref(layout), d_ids_all, d_hit_all, d_ids_rows, d_hit_rows, stream), "vpt_resolve_sdf_ids_device")


def state_init_device(layout: VptLayout, d_image: int, d_hits: int, d_rng: int, stream: int = 0) -> None:
    """vpt_state_init_device: make_state into this rank's tile-major slots on the device (raw device pointers), asynchronous"""
    _check(hip.vpt_state_init_device(C.byref(layout), d_image, d_hits, d_rng, stream), "vpt_state_init_device")


def make_state_jump(width: int, height: int) -> np.ndarray:
    """make_state's rngs, (h, w, 2) uint64, every pixel by a jump of the master stream (csrc/vpt_rng_jump.h, host side)"""
    out = np.zeros((height, width, 2), np.uint64)
    if host.vpth_make_state_jump(width, height, out.ctypes.data) != 0:
        raise VptError("make_state_jump failed")
    return out


def selftest_reciprocal(device: int = 0):
    """(mismatches, fallbacks) of the kernels' exact-reciprocal shortcut over all 2^32 floats (include/vpt.h)"""
    bad, skipped = C.c_ulonglong(0), C.c_ulonglong(0)
    _check(hip.vpt_selftest_reciprocal(device, C.byref(bad), C.byref(skipped)), "vpt_selftest_reciprocal")
    return bad.value, skipped.value


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
