"""Images on the host and on the device: resolving a state, denoising and its guides, the tone map, the preview's upscale, and the
quantisation and JPEG encoding of a saved image."""
from __future__ import annotations

import ctypes as C
from typing import TYPE_CHECKING, Optional

import numpy as np

from ._abi import (DENOISE_ITERATIONS, DENOISE_SIGMA_ALBEDO, DENOISE_SIGMA_LUMINANCE, DENOISE_SIGMA_NORMAL, VptDenoise, VptDisplay, VptError,
                   _check, _filled, _host_call, hip, host)
from .device import DeviceScene, DisplayParams, PathtraceParams, PathtraceState

if TYPE_CHECKING:
    from .host_scene import HostScene


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
    ptr = lambda a: None if a is None else a.ctypes.data
    _host_call(host.vpth_denoise, w, h, render.ctypes.data, ptr(normal), ptr(albedo), ptr(variance), iterations, sigma_luminance, sigma_normal,
               sigma_albedo, -1 if device is None else device, out.ctypes.data)
    return out


def half_variance(sum_a: np.ndarray, a: int, sum_n: np.ndarray, n: int, device: Optional[int] = None) -> np.ndarray:
    """the variance of each pixel's mean luminance from the radiance sums (PathtraceState.image) after the first `a` samples and
    after all `n` of one chain, 0 < a < n (include/vpt.h): (h, w) float32.  device None: host loops; else that GPU - same bits."""
    sum_a = _image4(sum_a)
    sum_n = _image4(sum_n, sum_a.shape)
    h, w, _ = sum_a.shape
    out = np.zeros((h, w), np.float32)
    _host_call(host.vpth_half_variance, w, h, sum_a.ctypes.data, a, sum_n.ctypes.data, n, -1 if device is None else device, out.ctypes.data)
    return out


def pathtrace_guides(scene: HostScene, dev, params: PathtraceParams, samples: int = 16):
    """the two guide renders of denoise_render on `dev` (a DeviceScene or MultiDeviceScene of `scene`): (normal, albedo) as resolved
    (h, w, 4) float32 images - `samples` passes of the `normal` and the `color` shader over a fresh make_state; for the implicit
    shaders: `implicit_normal`, and albedo None"""
    if params.shader == "volgrid":   # a medium has no first hit on a surface: nothing to guide a filter by
        raise VptError("pathtrace_guides: the volgrid shader has no guides (no surface normal, no albedo)")
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
    return bytes(_filled(lambda ptr, n: host.vpth_encode_jpeg_q75(w, h, src.ctypes.data, ptr, n), lambda n: (C.c_uint8 * n)(),
                         "encode_jpeg_q75: bad image"))
