// vpt_srgb.hip.h — the 8-bit output stage on the device, shared by vpt_resolve_srgb8_device (vpt_kernels.hip) and
// vpt_tonemap_device (vpt_frame_stages.hip): rgb_to_srgb (yocto_color.h:228-231) and float_to_byte (:207-211, clamp(int(a * 256), 0, 255)).
// powf is ocml's here and glibc's in the reference: a byte can differ by one where the curve lands within an ulp of a multiple of
// 1/256 (the parity pipeline keeps using the host routine, vpth_linear_to_srgb8).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float srgb_curve(float rgb) { return (rgb <= 0.0031308f) ? 12.92f * rgb : (1 + 0.055f) * powf(rgb, 1 / 2.4f) - 0.055f; }
__device__ __forceinline__ unsigned char srgb_quant(float a) {
  int b = (int)(a * 256);
  return (unsigned char)(b < 0 ? 0 : (b > 255 ? 255 : b));
}
