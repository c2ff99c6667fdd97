// vpt_error.h — error reporting shared by the library's translation units.
// vpt_set_error (vpt_capi.hip) records the message vpt_last_error() returns on the calling thread and returns `code`;
// HIP_TRY returns VPT_ERR_HIP from the enclosing function, with the failing call's text, when a HIP call fails;
// REQUIRE returns VPT_ERR_INVALID_ARG with the given message when a condition on the caller's input does not hold.
#pragma once

#include <hip/hip_runtime.h>

#include "vpt.h"

int vpt_set_error(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                                  \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return vpt_set_error(VPT_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));   \
  } while (0)

#define REQUIRE(cond, ...)                                                 \
  do {                                                                     \
    if (!(cond)) return vpt_set_error(VPT_ERR_INVALID_ARG, __VA_ARGS__);   \
  } while (0)
