// vpt_frame_stages.h — what vpt_session.hip needs of vpt_frame_stages.hip beyond the C-ABI of include/vpt.h.
#pragma once
#include "vpt.h"

// vpt_session_set_display's conditions on a vpt_display_params (those of vpt_tonemap_device)
int check_display(const vpt_display_params* display);

// vpt_state_init_device; d_image may be null here (hits and rng alone: the state a first-hit pass runs over)
int state_init(const vpt_layout* layout, void* d_image, void* d_hits, void* d_rng, void* stream);

// The 24 bytes of a pick - {hit, instance, element} as int32, {u, v, distance} as float - for `pixel` (y * width + x) of a row-major id
// frame (ids: int32 x2, uvt: float x3 per pixel, as vpt_resolve_ids_device leaves them) into d_out24: one launch on `stream`,
// asynchronous.  The sibling of vpt_sdf_pick_device (csrc/vpt_sdf_aov.h), argument for argument: `scene` is not read - shape and
// material come from the instance table the session read with the id frame.
int vpt_pick_device(const vpt_scene* scene, const void* d_ids_rowmajor, const void* d_uvt_rowmajor, long long pixel, void* d_out24, void* stream);
