// vpt_sdf_aov.h — what vpt_session.hip needs of vpt_sdf_aov.hip beyond the C-ABI of include/vpt.h.
#pragma once
#include "vpt.h"

// The 48 bytes of a vpt_sdf_pick for `pixel` (y * width + x) of a row-major id frame (ids: int32 x2, hit: float4 per pixel, as
// vpt_resolve_sdf_ids_device leaves them) into d_out48: one launch on `stream`, asynchronous.  volume / material come from the scene's
// resident tables, the normal from the SDF's normal function at the stored (position, t).
int vpt_sdf_pick_device(const vpt_scene* scene, const void* d_ids_rowmajor, const void* d_hit_rowmajor, long long pixel, void* d_out48, void* stream);
