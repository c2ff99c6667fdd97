// vpt_bake_prep.h — the host half of vpt_bake_sdf (include/vpt.h) that needs no device: validation of a descriptor
// and the feature normals (vpt_bake_feature_normals of include/vpt.h, under the name of the entry that asks for them).
#pragma once
#include "vpt.h"

// VPT_OK, or VPT_ERR_INVALID_ARG with a message that starts with `entry` and names what is wrong with the descriptor
int vpt_bake_validate(const vpt_bake_desc* desc, const char* entry);
// vpt_bake_feature_normals for `entry`: validates the descriptor, then fills normals (21 floats per triangle) and kept (nullable)
int vpt_bake_normals(const vpt_bake_desc* desc, float* normals, int32_t* kept, const char* entry);
