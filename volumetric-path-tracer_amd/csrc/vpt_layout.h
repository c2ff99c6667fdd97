// vpt_layout.h — the tile-major slot layout of include/vpt.h (vpt_layout) as the host sees it (csrc/vpt_layout.hip): the kernels'
// view of a layout, the one kernel that copies planes of per-pixel entries between row-major pixels and tile-major slots, and the
// host arrays -> rows -> tiles -> render -> rows -> host arrays round trip of the entry points that take host arrays.
// A new plane is one more entry in a list: it needs no kernel of its own.
#pragma once
#include "vpt_device.h"
#include "vpt_device_buffer.h"
#include "vpt_error.h"

// the kernels' view of a layout, validated; vpt_layout_dparams: for code that moves a state and renders nothing
int make_dparams(const vpt_params* p, const vpt_layout* l, int nsamples, DParams& out);
int vpt_layout_dparams(const vpt_layout* l, DParams& out);

// one plane on the device: `bytes` (4, 8, 12 or 16) per entry, tile-major and row-major
struct layout_plane {
  void* tiles;
  void* rows;
  int   bytes;
};
constexpr int k_layout_planes = 8;   // the most planes of one copy: the six of a first-hit pass, hits and rng
enum layout_copy_mode {
  LAYOUT_ROWS_TO_TILES,       // the pixels this rank owns -> its slots
  LAYOUT_TILES_TO_ROWS,       // this rank's slots -> the pixels it owns; pixels of other ranks are left alone
  LAYOUT_ALL_TILES_TO_ROWS,   // tiles = [nranks][nslots]: every pixel is written once
};
// One launch on `st` that copies every listed plane, values as they are; a slot that owns no pixel is neither read nor written.
int layout_copy(const vpt_layout* layout, layout_copy_mode mode, const layout_plane* planes, int n, hipStream_t st);

// one plane of a caller's host arrays (null: not given, skipped) and, for a caller that holds the state on the device, its tiles
struct host_plane {
  void* host;
  int   bytes;
  void* tiles = nullptr;
};
// The device copies of a transfer and, once prepared, what moves: the given planes, listed, and the tile-major pointer of every
// plane of the caller's list (null: not given).  An owner that keeps one between calls (vpt_render: the scene handle) allocates
// once per frame size.
struct layout_staging {
  device_buffer tile_buf[k_layout_planes], row_buf[k_layout_planes];
  size_t        tile_bytes[k_layout_planes] = {}, row_bytes[k_layout_planes] = {};
  layout_plane  dev[k_layout_planes];
  void*         host[k_layout_planes];
  void*         tiles[k_layout_planes];
  int           n = 0;
  size_t        pixels = 0;
};
// row-major copies for the given planes, tile-major ones too (of `slots` entries) where the caller brings none
int layout_prepare(const vpt_layout* layout, long long slots, const host_plane* planes, int n, layout_staging& sg);
// the two halves, asynchronous on `st`: host arrays -> rows -> tiles, and tiles -> rows -> host arrays.  from_host: the rows start
// from the host arrays, so that pixels of other ranks keep their values (a download into rows that do not hold the frame yet)
int layout_upload(const vpt_layout* layout, const layout_staging& sg, hipStream_t st);
int layout_download(const vpt_layout* layout, const layout_staging& sg, bool from_host, hipStream_t st);

// Host arrays through render(layout, tiles) and back, on one rank's layout and the null stream: tiles[k] is the tile-major copy of
// planes[k].  `staged`: kept by the caller between calls, else the copies live for this call.
template <typename Render>
int layout_round_trip(const vpt_layout& lay, const host_plane* planes, int n, layout_staging* staged, Render&& render) {
  const long long slots = vpt_layout_slots(&lay);
  if (slots < 0) return VPT_ERR_INVALID_ARG;
  layout_staging  own;
  layout_staging& sg = staged ? *staged : own;
  if (int rc = layout_prepare(&lay, slots, planes, n, sg)) return rc;
  if (int rc = layout_upload(&lay, sg, nullptr)) return rc;
  if (int rc = render(&lay, sg.tiles)) return rc;
  if (int rc = layout_download(&lay, sg, false, nullptr)) return rc;   // one rank owns every pixel, and the rows hold the frame
  HIP_TRY(hipStreamSynchronize(nullptr));
  return VPT_OK;
}

// A set of named planes, any of them null (device or host pointers alike): refuses a set that is all null, plane `dep` given without
// plane `ids`, and two planes in one buffer (the kernels update each plane on its own: updates would be lost).
int check_plane_set(const char* const* name, const void* const* given, int n, int ids, int dep);
