// vpt_aov.hip — the first-hit pass of vpt_render_aov_device (vpt_aov_kernel.hip.h) for scenes of faces, and the layout kernels of
// its planes: the gather of ids / uvt to row-major (vpt_resolve_ids_device) and the two-way permutation behind vpt_render_aov.
#include "vpt_aov_kernel.hip.h"
VPT_AOV_DEFINE(true, false)
VPT_AOV_DEFINE(false, false)

// the counterpart of vpt_resolve_kernel for the two id planes: [nranks][nslots] -> row-major, values as they are
__global__ void vpt_resolve_ids_kernel(DParams pr, const int2* ids_all, const float* uvt_all, int2* rows_ids, float* rows_uvt) {
  int g = blockIdx.x * blockDim.x + threadIdx.x;   // global slot over all ranks
  if (g >= pr.nslots * pr.nranks) return;
  DParams q = pr;
  q.rank    = g / pr.nslots;
  int px, py;
  if (!slot_to_pixel(q, g - q.rank * pr.nslots, px, py)) return;
  const long long idx = (long long)py * pr.width + px;
  rows_ids[idx] = ids_all[g];
  if (uvt_all)
    for (int c = 0; c < 3; c++) rows_uvt[3 * idx + c] = uvt_all[3 * (long long)g + c];
}

__global__ void vpt_aov_permute_kernel(DParams pr, int to_tiles, aov_planes tiles, int* tiles_hits, ulonglong2* tiles_rng, aov_planes rows,
    int* rows_hits, ulonglong2* rows_rng) {
  int slot = blockIdx.x * blockDim.x + threadIdx.x;
  int px, py;
  if (slot >= pr.nslots || !slot_to_pixel(pr, slot, px, py)) return;
  const long long idx = (long long)py * pr.width + px;
  float4* const   t4[4] = {tiles.normal, tiles.albedo, tiles.texcoord, tiles.depth};
  float4* const   r4[4] = {rows.normal, rows.albedo, rows.texcoord, rows.depth};
  for (int k = 0; k < 4; k++) {
    if (!t4[k]) continue;
    if (to_tiles) t4[k][slot] = r4[k][idx];
    else r4[k][idx] = t4[k][slot];
  }
  if (tiles.ids) {
    if (to_tiles) tiles.ids[slot] = rows.ids[idx];
    else rows.ids[idx] = tiles.ids[slot];
  }
  if (tiles.uvt)
    for (int c = 0; c < 3; c++) {
      if (to_tiles) tiles.uvt[3 * (long long)slot + c] = rows.uvt[3 * idx + c];
      else rows.uvt[3 * idx + c] = tiles.uvt[3 * (long long)slot + c];
    }
  if (to_tiles) tiles_hits[slot] = rows_hits[idx], tiles_rng[slot] = rows_rng[idx];
  else rows_hits[idx] = tiles_hits[slot], rows_rng[idx] = tiles_rng[slot];
}
