// vpt_update_helpers.h — what the units that edit a resident scene share (vpt_scene_update.hip, vpt_light_update.hip,
// vpt_texture_update.hip, vpt_volume_update.hip, vpt_bvh_rebuild.hip, vpt_instance_update.hip, vpt_shape_update.hip): the checks of an
// edit's lists and floats, the start and the end of an edit, the counted launch, the edit's payload as one host block, and the handling
// of the handle's tables - counted sends and read-backs, moves on the device, pools that grow.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "vpt_device_buffer.h"
#include "vpt_error.h"
#include "vpt_resident.h"

template <typename T>
inline T* mut(const T* p) { return const_cast<T*>(p); }   // the scene owns its tables: DScene names them const for the render kernels

inline bool finite_all(const float* p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(p[i])) return false;
  return true;
}
// ids of one list and the payload beside them: non-null, in range, no repeats
inline int check_ids(const char* what, int n, const int32_t* ids, const void* payload, int limit) {
  REQUIRE(n >= 0 && (n == 0 || (ids && payload)), "edit: %s list is null or has a negative count", what);
  std::vector<char> seen((size_t)limit, 0);
  for (int i = 0; i < n; i++) {
    REQUIRE(ids[i] >= 0 && ids[i] < limit, "edit: %s entry %d: id %d out of range (%d)", what, i, ids[i], limit);
    REQUIRE(!seen[(size_t)ids[i]], "edit: %s entry %d: id %d repeated", what, i, ids[i]);
    seen[(size_t)ids[i]] = 1;
  }
  return VPT_OK;
}
inline int check_ids(const char* what, int n, const int32_t* ids, int limit) { return check_ids(what, n, ids, ids, limit); }   // a list without a payload
// make_lights, yocto_pathtrace.cpp:990 and :1017
inline bool emissive(const vpt_material& m) { return !(m.emission[0] == 0 && m.emission[1] == 0 && m.emission[2] == 0); }
inline bool emissive(const vpt_environment& e) { return !(e.emission[0] == 0 && e.emission[1] == 0 && e.emission[2] == 0); }

// An edit has passed validation and is about to write: the counters of vpt_scene_update_stats start at zero, the events exist.
inline int begin_update(resident& r) {
  r.last_launches = 0, r.last_bytes = 0, r.last_ms = 0;
  if (!r.upd_ev0) {
    HIP_TRY(hipEventCreate(&r.upd_ev0));
    HIP_TRY(hipEventCreate(&r.upd_ev1));
  }
  return VPT_OK;
}
// The end of what vpt_scene_update_stats times: the mark on stream 0, where the unit has launched its last kernel ...
inline int mark_end(resident& r) {
  HIP_TRY(hipEventRecord(r.upd_ev1, 0));
  return VPT_OK;
}
// ... and, once the device has finished, the time between the two marks
inline int finish_update(resident& r) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipEventElapsedTime(&r.last_ms, r.upd_ev0, r.upd_ev1));
  return VPT_OK;
}

// One lane per item on stream 0, counted; nothing for n = 0.  (A launch of another shape counts itself with LAUNCHED.)
constexpr int BLOCK = 256;
inline unsigned blocks_for(long long n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }
#define LAUNCHED(r)             \
  do {                          \
    HIP_TRY(hipGetLastError()); \
    (r).last_launches++;        \
  } while (0)
#define LAUNCH(r, kernel, n, ...)                                                        \
  do {                                                                                   \
    if ((n) > 0) {                                                                       \
      hipLaunchKernelGGL(kernel, dim3(blocks_for(n)), dim3(BLOCK), 0, 0, __VA_ARGS__);   \
      LAUNCHED(r);                                                                       \
    }                                                                                    \
  } while (0)

// An edit's bulk payload goes to the device in ONE copy: every array at a 16-byte aligned offset of a host block, which the kernels
// that follow on stream 0 read at those offsets.
struct staged_block {
  std::vector<char> host;
  size_t add(const void* src, size_t bytes) {
    const size_t at = (host.size() + 15) & ~(size_t)15;
    host.resize(at + bytes);
    if (bytes) memcpy(host.data() + at, src, bytes);
    return at;
  }
};

// `count` entries from the host into their place in a table of the scene, counted
template <typename T>
inline int send(resident& r, const T* to, const T* host, size_t count) {
  if (count) HIP_TRY(hipMemcpy(mut(to), host, count * sizeof(T), hipMemcpyHostToDevice));
  r.last_bytes += (long long)(count * sizeof(T));
  return VPT_OK;
}
// a buffer allocated for `host` and filled with it, counted
template <typename T>
inline int send(resident& r, device_buffer& to, const std::vector<T>& host) {
  if (int rc = to.allocate(host.size() * sizeof(T))) return rc;
  return send(r, to.get<const T>(), host.data(), host.size());
}

// `count` entries from the device to the host, counted
template <typename T>
inline int fetch(resident& r, std::vector<T>& out, const void* dev, size_t count) {
  out.resize(count);
  if (count) HIP_TRY(hipMemcpy(out.data(), dev, count * sizeof(T), hipMemcpyDeviceToHost));
  r.last_bytes += (long long)(count * sizeof(T));
  return VPT_OK;
}
inline int copy_on_device(void* to, const void* from, size_t bytes) {
  if (bytes) HIP_TRY(hipMemcpy(to, from, bytes, hipMemcpyDeviceToDevice));
  return VPT_OK;
}

// `fresh` takes the place of the table at `old` among the scene's allocations
inline void adopt(std::vector<device_buffer>& tables, const void* old, device_buffer&& fresh) {
  for (device_buffer& t : tables)
    if (t.get() == old) {
      t = std::move(fresh);
      return;
    }
  tables.push_back(std::move(fresh));
}
// a pool of `have` entries (texels, voxels) grown by `more`: allocated anew, the old entries moved device to device
template <typename T>
inline int grow_pool(resident& r, const T*& pool, long long& have, long long more) {
  device_buffer fresh;
  if (int rc = fresh.allocate((size_t)(have + more) * sizeof(T))) return rc;
  if (int rc = copy_on_device(fresh.get(), pool, (size_t)have * sizeof(T))) return rc;
  const void* old = pool;
  pool = fresh.get<const T>();
  adopt(r.tables, old, std::move(fresh));
  have += more;
  return VPT_OK;
}
