// vpt_update_helpers.h — what the three update paths of a resident scene share (vpt_scene_update.hip, vpt_light_update.hip,
// vpt_texture_update.hip): the checks of an edit's lists and floats, and the handling of the handle's tables.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "vpt_device_buffer.h"
#include "vpt_error.h"

template <typename T>
inline T* mut(const T* p) { return const_cast<T*>(p); }   // the scene owns its tables: DScene names them const for the render kernels

inline bool finite_all(const float* p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(p[i])) return false;
  return true;
}
// ids of one list: non-null, in range, no repeats
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
// `fresh` takes the place of the table at `old` among the scene's allocations
inline void adopt(std::vector<device_buffer>& tables, const void* old, device_buffer&& fresh) {
  for (device_buffer& t : tables)
    if (t.get() == old) {
      t = std::move(fresh);
      return;
    }
  tables.push_back(std::move(fresh));
}
