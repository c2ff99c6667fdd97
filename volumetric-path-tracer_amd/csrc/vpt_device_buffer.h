// vpt_device_buffer.h — owner of one device allocation: freed when its owner goes, on every path.
// Frees on the current device: a holder of buffers on another device sets that device before it lets them go.
#pragma once
#include <cstddef>
#include <utility>

#include "vpt_error.h"

class device_buffer {   // move-only (its move operations delete the copies)
 public:
  device_buffer() = default;
  device_buffer(device_buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  device_buffer& operator=(device_buffer&& o) noexcept {
    if (this != &o) release(), p_ = std::exchange(o.p_, nullptr);
    return *this;
  }
  ~device_buffer() { release(); }

  // drops what it holds and allocates `bytes` (16 for 0: no kernel is handed a null table); fails with VPT_ERR_HIP only
  int allocate(size_t bytes) {
    release();
    HIP_TRY(hipMalloc(&p_, bytes ? bytes : 16));
    return VPT_OK;
  }
  template <typename T = void>
  T* get() const { return static_cast<T*>(p_); }

 private:
  void release() {
    if (p_) (void)hipFree(p_), p_ = nullptr;
  }
  void* p_ = nullptr;
};
