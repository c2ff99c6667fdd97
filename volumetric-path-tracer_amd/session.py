"""RenderSession: a progressive render whose state, image and display stay on the GPU."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from ._abi import (DENOISE_ITERATIONS, DENOISE_SIGMA_ALBEDO, DENOISE_SIGMA_LUMINANCE, DENOISE_SIGMA_NORMAL, VptAdaptive, VptDenoise, VptPick,
                   VptError, VptSdf, VptSdfPick, VptSessionParams, _Handle, _check, _edit_call, _p, hip)
from .device import DeviceScene, DisplayParams, PathtraceParams, PathtraceState, _subdiv_edit_call
from .edits import BvhRebuild, InstanceEdit, SceneEdit, SculptEdit, SculptEntry, ShapeEdit, Stamp, SubdivEdit, TextureEdit, VolumeEdit, VolumeSetEdit


class RenderSession(_Handle):
    """vpt_session (include/vpt.h): a progressive render of one camera whose state, linear image and display stay on the GPU of `dev`
    (a DeviceScene).  reset() is the reference's reset_display (preview included), advance(n) renders n more samples and refreshes the
    display; display() / image() / state() fetch.  While it lives, `dev` must not be used from another thread."""
    _free = staticmethod(hip.vpt_session_destroy)

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
        _edit_call(self.handle, "vpt_session_edit", edit)

    def edit_lights(self, edit: SceneEdit) -> None:
        """edit() through vpt_scene_update_lights, with the SceneEdit of HostScene.update_lights()"""
        _edit_call(self.handle, "vpt_session_edit_lights", edit)

    def edit_textures(self, edit: TextureEdit) -> None:
        """edit() through vpt_scene_update_textures, with the TextureEdit of HostScene.update_textures()"""
        _edit_call(self.handle, "vpt_session_edit_textures", edit)

    def edit_volumes(self, edit: VolumeEdit) -> None:
        """edit() through vpt_scene_update_volumes, with the VolumeEdit of HostScene.update_volumes()"""
        _edit_call(self.handle, "vpt_session_edit_volumes", edit)

    def edit_volume_set(self, edit: VolumeSetEdit) -> None:
        """edit() through vpt_scene_update_volume_set, with the VolumeSetEdit of HostScene.update_volume_set(); the reset drops both id
        frames, so pick_sdf names the lists as the edit leaves them"""
        _edit_call(self.handle, "vpt_session_edit_volume_set", edit)

    def edit_sculpts(self, edit: SculptEdit) -> None:
        """vpt_scene_sculpt_volumes on the session's scene with the SculptEdit of HostScene.update_sculpts(), then a reset; a refused edit
        leaves the session as it was"""
        _edit_call(self.handle, "vpt_session_sculpt_volumes", edit)

    def sculpt_at(self, host, x: int, y: int, brush: VptSdf, op: int, blend: float = 0.0, region_margin: int = 2) -> SculptEntry:
        """The editor's gesture: one stamp of `brush` where the ray through pixel (x, y) hits a voxel grid.  pick_sdf(x, y) names the grid
        instance and the hit (a miss or a hit on an analytic SDF raises VptError); the hit is taken into that instance's voxel space,
        transform_point(instance.frame, position) / scalef; the brush keeps its frame's axes and gets the origin that puts its local origin
        at the hit; the region is the box around the ball that holds the brush (a plane: the whole grid), widened by blend and by
        region_margin voxels and clipped to the grid.  Then host.sculpt_volume, host.update_sculpts() and edit_sculpts: `host` is the
        HostScene the session's scene was made from.  Returns the entry it made.  The arithmetic of this helper carries no bit contract:
        the entry it makes goes to the host mirror and to the device alike."""
        pick = self.pick_sdf(x, y)
        if pick is None:
            raise VptError(f"sculpt_at: the ray through pixel ({x}, {y}) hits nothing")
        if pick["vol_instance"] < 0:
            raise VptError(f"sculpt_at: pixel ({x}, {y}) shows analytic SDF {pick['sdf']}, not a voxel grid")
        inst = host.volume_instance(pick["vol_instance"])
        to_grid = np.array([inst.frame.x[:], inst.frame.y[:], inst.frame.z[:], inst.frame.o[:]], np.float64)
        centre = (pick["position"].astype(np.float64) @ to_grid[:3] + to_grid[3]) / float(inst.scalef)
        voxels, res = host.volume(pick["volume"])
        whd = np.array(voxels.shape[::-1])
        step = np.array([np.float32(res) * np.float32(w) / np.float32(max(1, w - 1)) for w in whd], np.float64)
        placed = VptSdf()
        C.memmove(C.byref(placed), C.byref(brush), C.sizeof(VptSdf))
        axes = np.array([brush.frame.x[:], brush.frame.y[:], brush.frame.z[:]], np.float64)
        placed.frame.o[:] = [float(v) for v in -(centre @ axes)]
        q, size = [float(v) for v in brush.p], [float(v) for v in brush.whd]
        reach = {0: float(np.linalg.norm(q[1:4])) + abs(q[0]), 1: float(np.linalg.norm(size)), 2: float(np.hypot(q[0], max(abs(q[1]), abs(q[2])))),
                 3: np.inf, 4: abs(q[0]), 5: abs(q[0]) + abs(q[1])}.get(int(brush.type), np.inf)
        stretch = np.linalg.svd(axes, compute_uv=False).min()   # a local ball of radius r lies inside a voxel-space ball of r / stretch
        reach = (reach + float(blend)) / stretch if stretch > 0 else np.inf
        if np.isfinite(reach):
            lo = np.clip(np.floor((centre - reach) / step).astype(np.int64) - region_margin, 0, whd)
            hi = np.clip(np.ceil((centre + reach) / step).astype(np.int64) + region_margin + 1, lo, whd)
        else:
            lo, hi = np.zeros(3, np.int64), whd
        entry = host.sculpt_volume(pick["volume"], [Stamp(placed, op, blend)], region=(tuple(lo), tuple(hi - lo)))
        self.edit_sculpts(host.update_sculpts())
        return entry

    def mesh_volume(self, index: int, iso: float = 0.0, origin=None, step=None, region=None, stats: Optional[dict] = None) -> dict:
        """DeviceScene.mesh_volume on the session's scene (vpt_scene_mesh_volume waits for the session's launches); the session goes on
        as it was: nothing of the scene changes"""
        return self.dev.mesh_volume(index, iso, origin, step, region, stats)

    def volume_to_shape(self, host, vol_instance: int, material: int):
        """The editor's gesture: the surface the sphere trace finds on grid instance `vol_instance` as a shape of quads, instanced where it
        is.  The instance's grid is meshed on the device with step * scalef (the instance's lookup space); the mesh becomes a new shape
        (host.add_shape, update_shapes, edit_shapes) and a new instance of it with `material` and the inverse of the grid instance's frame
        (host.add_instance, update_instances, edit_instances): `host` is the HostScene the session's scene was made from.  Returns (shape
        id, instance id).  The arithmetic of this helper carries no bit contract: the mesh it makes goes to the host mirror and to the
        device alike."""
        inst = host.volume_instance(vol_instance)
        voxels, res = host.volume(inst.volume)
        scale = np.float32(inst.scalef)
        step = np.array([np.float32(res) * np.float32(w) / np.float32(max(1, w - 1)) * scale for w in voxels.shape[::-1]], np.float32)
        m = self.mesh_volume(inst.volume, step=step)
        if m["positions"] is None or m["quads"] is None:
            raise VptError(f"volume_to_shape: the grid of volume instance {vol_instance} has no surface inside it")
        to_grid = np.array([inst.frame.x[:], inst.frame.y[:], inst.frame.z[:], inst.frame.o[:]], np.float64)
        axes = np.linalg.inv(to_grid[:3])   # world = (grid - o) @ inverse(axes)
        frame = np.concatenate([axes, -(to_grid[3] @ axes)[None]]).astype(np.float32).reshape(12)
        shape = host.add_shape(**m)
        self.edit_shapes(host.update_shapes())
        instance = host.add_instance(frame, shape, material)
        self.edit_instances(host.update_instances())
        return shape, instance

    def rebuild_bvh(self, rebuild: "BvhRebuild") -> None:
        """vpt_scene_rebuild_bvh on the session's scene with the BvhRebuild of HostScene.rebuild_bvh(), then a reset"""
        _edit_call(self.handle, "vpt_session_rebuild_bvh_quality", rebuild, rebuild.quality)

    def edit_instances(self, edit: InstanceEdit) -> None:
        """vpt_scene_update_instances on the session's scene with the InstanceEdit of HostScene.update_instances(), then a reset; a
        refused edit leaves the session as it was"""
        _edit_call(self.handle, "vpt_session_edit_instances", edit)

    def edit_shapes(self, edit: ShapeEdit) -> None:
        """vpt_scene_update_shapes on the session's scene with the ShapeEdit of HostScene.update_shapes(), then a reset; a refused edit
        leaves the session as it was"""
        _edit_call(self.handle, "vpt_session_edit_shapes", edit)

    def edit_subdivs(self, edit: SubdivEdit) -> None:
        """vpt_scene_update_subdivs on the session's scene with the SubdivEdit of HostScene.update_subdivs(), then a reset; plans are
        attached on the session's DeviceScene as DeviceScene.update_subdivs attaches them; a refused edit leaves the session as it was"""
        _subdiv_edit_call(self.dev, hip.vpt_scene_attach_subdiv, hip.vpt_scene_subdiv_shape, self.handle, "vpt_session_edit_subdivs", edit)

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
        if self.params.shader == "volgrid":
            raise VptError("guides: a volgrid session has none (vpt_session_get_guides: unsupported)")
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

    def pick_sdf(self, x: int, y: int) -> Optional[dict]:
        """what is under pixel (x, y) of an implicit session's frame (vpt_session_pick_sdf): None on a miss, else a dict of vol_instance,
        sdf (exactly one >= 0), volume (-1 for an analytic SDF), material, distance, position, normal.  48 bytes cross PCIe; the first
        pick_sdf or sdf_ids() after a reset makes the id frame."""
        out = VptSdfPick()
        _check(hip.vpt_session_pick_sdf(self.handle, x, y, C.byref(out)), "vpt_session_pick_sdf")
        if not out.hit:
            return None
        pick = {name: getattr(out, name) for name in ("vol_instance", "sdf", "volume", "material", "distance")}
        pick["position"], pick["normal"] = np.array(out.position[:], np.float32), np.array(out.normal[:], np.float32)
        return pick

    def sdf_ids(self):
        """the id frame of an implicit session (vpt_session_get_sdf_ids): (ids, hit) = (h, w, 2) int32 {vol_instance, sdf} (-1, -1 on a
        miss) and (h, w, 4) float32 {position, t} of the rays through the pixel centres (zeros on a miss)"""
        w, h = self.size
        ids, hit = np.zeros((h, w, 2), np.int32), np.zeros((h, w, 4), np.float32)
        _check(hip.vpt_session_get_sdf_ids(self.handle, ids.ctypes.data, hit.ctypes.data), "vpt_session_get_sdf_ids")
        return ids, hit

    def stats(self):
        """(kernel launches, bytes to the device, bytes to the host) of the last call on the session"""
        n, up, down = C.c_int(0), C.c_int64(0), C.c_int64(0)
        _check(hip.vpt_session_stats(self.handle, C.byref(n), C.byref(up), C.byref(down)), "vpt_session_stats")
        return n.value, up.value, down.value
