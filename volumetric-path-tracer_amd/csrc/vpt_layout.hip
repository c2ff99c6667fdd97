// vpt_layout.hip — everything that knows how a plane of per-pixel entries maps to the tile-major slots of include/vpt.h (vpt_layout):
// see vpt_layout.h.  Holds no render kernel; the kernels that compute while they move (the resolves, vpt_state_init_kernel) stay
// with their units.
#include "vpt_layout.h"
#include "vpt_kernels.hip.h"   // slot_to_pixel

int make_dparams(const vpt_params* p, const vpt_layout* l, int nsamples, DParams& out) {
  REQUIRE(p && l, "null params/layout");
  REQUIRE(l->width > 0 && l->height > 0 && l->nranks > 0 && l->rank >= 0 && l->rank < l->nranks, "bad layout");
  REQUIRE(l->width < 32768 && l->height < 32768, "frame side must be below 32768 pixels (the kernels keep a pixel's coordinates in one word; the reference's --resolution ends at 4096)");
  REQUIRE(l->tile_w >= 8 && l->tile_h >= 8 && l->tile_w % 8 == 0 && l->tile_h % 8 == 0, "tile size must be a multiple of 8x8");
  out = {};
  out.camera = p->camera, out.shader = p->shader, out.bounces = p->bounces, out.noimplicit_mis = p->noimplicit_mis;
  out.spheretrace_maxiter = p->spheretrace_maxiter, out.preview = p->samples == 1, out.nsamples = nsamples;
  out.width = l->width, out.height = l->height, out.tile_w = l->tile_w, out.tile_h = l->tile_h;
  out.tiles_x = (l->width + l->tile_w - 1) / l->tile_w, out.tiles_y = (l->height + l->tile_h - 1) / l->tile_h;
  out.rank = l->rank, out.nranks = l->nranks;
  long long tiles = (long long)out.tiles_x * out.tiles_y;
  long long local = (tiles + l->nranks - 1) / l->nranks;   // every rank allocates the same count
  long long slots = local * l->tile_w * l->tile_h;
  REQUIRE(slots < (1LL << 31), "image too large");
  out.nslots = (int)slots;
  return VPT_OK;
}

int vpt_layout_dparams(const vpt_layout* l, DParams& out) {
  vpt_params none = {};
  return make_dparams(&none, l, 0, out);
}

namespace {

struct plane_list {   // a kernel argument: the loop over it is wave-uniform and its entries are read as scalars
  layout_plane e[k_layout_planes];
  int          n;
};

// One lane per slot: of this rank, or (LAYOUT_ALL_TILES_TO_ROWS) of the [nranks][nslots] buffers of all ranks.  An entry moves in
// one access of its width; 12 bytes as three dwords, because those planes are aligned to 4 bytes only.
__global__ void __launch_bounds__(256) vpt_layout_copy_kernel(DParams pr, int mode, plane_list list) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= pr.nslots * (mode == LAYOUT_ALL_TILES_TO_ROWS ? pr.nranks : 1)) return;
  if (mode == LAYOUT_ALL_TILES_TO_ROWS) pr.rank = g / pr.nslots;
  int px, py;
  if (!slot_to_pixel(pr, mode == LAYOUT_ALL_TILES_TO_ROWS ? g - pr.rank * pr.nslots : g, px, py)) return;   // padding, or another rank's
  const long long idx = (long long)py * pr.width + px;
  for (int k = 0; k < list.n; k++) {
    const layout_plane p = list.e[k];
    char* const        t = (char*)p.tiles + (long long)g * p.bytes;
    char* const        r = (char*)p.rows + idx * p.bytes;
    const char* const  src = mode == LAYOUT_ROWS_TO_TILES ? r : t;
    char* const        dst = mode == LAYOUT_ROWS_TO_TILES ? t : r;
    if (p.bytes == 16) *(uint4*)dst = *(const uint4*)src;
    else if (p.bytes == 8) *(uint2*)dst = *(const uint2*)src;
    else
      for (int c = 0; c < p.bytes; c += 4) *(unsigned*)(dst + c) = *(const unsigned*)(src + c);
  }
}

int reserve(device_buffer& b, size_t& have, size_t want) {
  if (have == want) return VPT_OK;
  have = 0;
  if (int rc = b.allocate(want)) return rc;
  have = want;
  return VPT_OK;
}

}  // namespace

int layout_copy(const vpt_layout* layout, layout_copy_mode mode, const layout_plane* planes, int n, hipStream_t st) {
  REQUIRE(planes && n >= 1 && n <= k_layout_planes, "layout copy of %d planes (1 .. %d)", n, k_layout_planes);
  plane_list list = {};
  for (int k = 0; k < n; k++) {
    const layout_plane& p = list.e[k] = planes[k];
    REQUIRE(p.tiles && p.rows, "layout copy: plane %d is null", k);
    REQUIRE(p.bytes == 4 || p.bytes == 8 || p.bytes == 12 || p.bytes == 16, "layout copy: plane %d has %d bytes per entry", k, p.bytes);
  }
  list.n = n;
  DParams pr;
  if (int rc = vpt_layout_dparams(layout, pr)) return rc;
  const long long total = (long long)pr.nslots * (mode == LAYOUT_ALL_TILES_TO_ROWS ? pr.nranks : 1);
  REQUIRE(total < (1LL << 31), "image too large");
  hipLaunchKernelGGL(vpt_layout_copy_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, pr, (int)mode, list);
  HIP_TRY(hipGetLastError());
  return VPT_OK;
}

int layout_prepare(const vpt_layout* layout, long long slots, const host_plane* planes, int n, layout_staging& sg) {
  REQUIRE(n >= 0 && n <= k_layout_planes, "layout transfer of %d planes (0 .. %d)", n, k_layout_planes);
  sg.n = 0, sg.pixels = (size_t)layout->width * layout->height;
  for (int k = 0; k < n; k++) {
    const host_plane& p = planes[k];
    sg.tiles[k] = nullptr;
    if (!p.host) continue;
    if (int rc = reserve(sg.row_buf[k], sg.row_bytes[k], sg.pixels * p.bytes)) return rc;
    if (!p.tiles)
      if (int rc = reserve(sg.tile_buf[k], sg.tile_bytes[k], (size_t)slots * p.bytes)) return rc;
    sg.tiles[k] = p.tiles ? p.tiles : sg.tile_buf[k].get();
    sg.host[sg.n] = p.host, sg.dev[sg.n++] = {sg.tiles[k], sg.row_buf[k].get(), p.bytes};
  }
  return VPT_OK;
}

static int fill_rows(const layout_staging& sg, hipStream_t st) {
  for (int k = 0; k < sg.n; k++) HIP_TRY(hipMemcpyAsync(sg.dev[k].rows, sg.host[k], sg.pixels * sg.dev[k].bytes, hipMemcpyHostToDevice, st));
  return VPT_OK;
}

int layout_upload(const vpt_layout* layout, const layout_staging& sg, hipStream_t st) {
  if (int rc = fill_rows(sg, st)) return rc;
  return layout_copy(layout, LAYOUT_ROWS_TO_TILES, sg.dev, sg.n, st);
}

int layout_download(const vpt_layout* layout, const layout_staging& sg, bool from_host, hipStream_t st) {
  if (from_host)
    if (int rc = fill_rows(sg, st)) return rc;
  if (int rc = layout_copy(layout, LAYOUT_TILES_TO_ROWS, sg.dev, sg.n, st)) return rc;
  for (int k = 0; k < sg.n; k++) HIP_TRY(hipMemcpyAsync(sg.host[k], sg.dev[k].rows, sg.pixels * sg.dev[k].bytes, hipMemcpyDeviceToHost, st));
  return VPT_OK;
}

int check_plane_set(const char* const* name, const void* const* given, int n, int ids, int dep) {
  bool any = false;
  for (int a = 0; a < n; a++) any = any || given[a];
  REQUIRE(any, "planes: every plane is null, nothing to render");
  REQUIRE(given[ids] || !given[dep], "planes: %s is given without ids", name[dep]);
  for (int a = 0; a < n; a++)
    for (int b = a + 1; b < n; b++) REQUIRE(!given[a] || given[a] != given[b], "planes: %s and %s share a buffer", name[a], name[b]);
  return VPT_OK;
}

// vpt_state_upload / vpt_state_download: one half each, through row-major copies that live for the call
static int move_state(const vpt_layout* layout, bool to_tiles, void* image_rgba, void* hits, void* rng, void* d_image, void* d_hits, void* d_rng,
    hipStream_t st) {
  if (!layout || !image_rgba || !hits || !rng || !d_image || !d_hits || !d_rng) return vpt_set_error(VPT_ERR_INVALID_ARG, "null argument");
  if (layout->width <= 0 || layout->height <= 0) return vpt_set_error(VPT_ERR_INVALID_ARG, "bad layout");
  const host_plane state[3] = {{image_rgba, 16, d_image}, {hits, 4, d_hits}, {rng, 16, d_rng}};
  layout_staging   rows;
  if (layout_prepare(layout, 0, state, 3, rows)) return VPT_ERR_HIP;
  if (int rc = to_tiles ? layout_upload(layout, rows, st) : layout_download(layout, rows, true, st)) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  return VPT_OK;
}

extern "C" {

int64_t vpt_layout_slots(const vpt_layout* layout) {
  DParams pr;
  if (vpt_layout_dparams(layout, pr) != VPT_OK) return -1;
  return pr.nslots;
}

int vpt_state_upload(const vpt_layout* layout, const float* image_rgba, const int32_t* hits, const uint64_t* rng, void* d_image, void* d_hits,
    void* d_rng, void* stream) {
  return move_state(layout, true, (void*)image_rgba, (void*)hits, (void*)rng, d_image, d_hits, d_rng, (hipStream_t)stream);
}

int vpt_state_download(const vpt_layout* layout, const void* d_image, const void* d_hits, const void* d_rng, float* image_rgba, int32_t* hits,
    uint64_t* rng, void* stream) {
  return move_state(layout, false, image_rgba, hits, rng, (void*)d_image, (void*)d_hits, (void*)d_rng, (hipStream_t)stream);
}

}  // extern "C"
