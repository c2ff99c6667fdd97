// vpt_subdiv.h — the launchers of the tesselation kernels (vpt_subdiv.hip) for a caller that keeps its meshes on the device: the host-array
// entry points of include/vpt.h (vpt_subdivide_vertices, vpt_vertex_normals, vpt_displace_vertices) are wrappers of them, and so is the
// re-tesselation of a resident scene's subdivs (vpt_subdiv_update.hip).  Every pointer is a device pointer; nothing is allocated, copied
// or waited for; the launches go to `stream` on the current device; each call returns the number of launches it made.  Every index the
// tables hold was checked on the host by whoever uploaded them.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "vpt_device.h"

// one Catmull-Clark level on the device: vpt_subdiv_level of include/vpt.h, its tables uploaded
struct subdiv_level_dev {
  int         nv, ne, nf;   // of the level's cage; it refines to nv + ne + nf vertices
  const int2* edges;
  const int4* faces;
  const int4* tquads;
  const int*  valence;
  const int*  offsets;
  const int*  items;
};
inline int refined_vertices(const subdiv_level_dev& L) { return L.nv + L.ne + L.nf; }

// the index checks of vpt_subdivide_vertices on a level whose sizes are sane (non-negative, at most 2^30 refined vertices) and whose
// tables are not null: VPT_ERR_INVALID_ARG, the message names the entry
int subdiv_check_level_indices(const vpt_subdiv_level& level);

// `vert` (L.nv entries of dim floats) -> `out` (refined_vertices(L) entries) through `tverts` (as many): the points pass, then the
// averaging pass - two launches
int subdiv_launch_level(int dim, const subdiv_level_dev& L, const float* vert, float* tverts, float* out, hipStream_t stream);

// Consecutive levels of float3 positions in ONE launch of ONE workgroup, for levels that refine to at most SUBDIV_FUSE_WIDTH vertices:
// a thread per refined vertex, __syncthreads() between the points pass and the averaging pass and between one level and the next; the
// barrier's workgroup-scope fence is what makes a level's vertices (global memory) visible to the next pass.  Same device functions as
// the two kernels of subdiv_launch_level: same bits.  Level k reads level k - 1's output and writes buf[k & 1]; the first reads `vert`.
enum { SUBDIV_FUSE_WIDTH = 256, SUBDIV_FUSE_LEVELS = 6 };
struct subdiv_fused_levels {
  subdiv_level_dev L[SUBDIV_FUSE_LEVELS];
  int              count;
};
int subdiv_launch_levels_fused(const subdiv_fused_levels& levels, const float* vert, float* tverts, float* buf0, float* buf1, hipStream_t stream);

// quads_normals / triangles_normals: faces[stride * f + 0 .. corners) are face f's vertices (corners 4: a quad, z == w a triangle; 3: a
// triangle - with stride 4 the int4 elements of a resident scene); offsets / items: per vertex the faces that add to it, in face order
int subdiv_launch_normals(int num_vertices, int corners, int stride, const float* positions, const int* faces, const int* offsets, const int* items,
    float* normals, hipStream_t stream);
// the per-vertex face lists of subdiv_launch_normals (host, integers): VPT_ERR_INVALID_ARG for a face that names a vertex out of range
int subdiv_face_lists(int num_vertices, int num_faces, int corners, int stride, const int32_t* faces, std::vector<int>& offsets, std::vector<int>& items);

// out = positions + normals * displacement * (mean(xyz(eval_texture(sc, texture, uv, as_linear))) [- 0.5 when byte_texture]); float3
// positions / normals / out, float2 uv; sc: any scene whose texture tables hold `texture`
int subdiv_launch_displace(const DScene& sc, int texture, int byte_texture, float displacement, int num_vertices, const float* positions, const float* normals,
    const float* uv, float* out, hipStream_t stream);
