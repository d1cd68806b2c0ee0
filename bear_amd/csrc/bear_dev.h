// bear_dev.h -- internal: how the host code of libbear_hip holds device memory and reports HIP errors.  One owner of a hipMalloc
// allocation, one mapping of a hipError_t to a status, one try-macro; every unit takes them from here (bear_common.h includes
// this file; bear_count.hip, which needs nothing else of the host side, includes it directly).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/bear_hip.h"

// the HIP error behind the last BEAR_ERR_HIP / BEAR_ERR_NOMEM of this thread, for the whole library: bear_last_hip_error()
__attribute__((visibility("hidden"))) inline thread_local int g_last_hip_error = 0;

// The status of a HIP call: out of device memory is BEAR_ERR_NOMEM from every entry (a caller may give memory back and try
// again), anything else BEAR_ERR_HIP.
static inline int hip_status(hipError_t e) {
  if (e != hipSuccess) g_last_hip_error = (int)e;
  return e != hipSuccess ? (e == hipErrorOutOfMemory ? BEAR_ERR_NOMEM : BEAR_ERR_HIP) : BEAR_OK;
}

// Returns the status of a failed call from the enclosing function.  Returning early is safe because whatever the function
// allocated so far sits in a dev_buf, or in a struct that a guard over its free function holds.
#define HIP_TRY(expr)                    \
  do {                                   \
    const int _st = hip_status(expr);    \
    if (_st != BEAR_OK) return _st;      \
  } while (0)

// Owner of one hipMalloc allocation of T[n]: freed with the owner, or earlier by reset() -- hipFree waits for the device, so
// where a temporary goes is part of a function's timing and of its peak memory, and is written out.  release() hands the
// pointer to a long-lived struct, whose free function then owns it.
template <typename T>
class dev_buf {
 public:
  dev_buf() = default;
  dev_buf(dev_buf &&o) noexcept : p_(o.release()) {}
  dev_buf(const dev_buf &) = delete;
  dev_buf &operator=(const dev_buf &) = delete;
  ~dev_buf() { reset(); }

  T *get() const { return p_; }
  hipError_t alloc(size_t n) {
    reset();
    return hipMalloc(&p_, n * sizeof(T));      // (leaves p_ NULL when it fails)
  }
  hipError_t alloc_zeroed(size_t n) {
    const hipError_t e = alloc(n);
    return e != hipSuccess ? e : hipMemset(p_, 0, n * sizeof(T));
  }
  void reset() {
    if (p_) (void)hipFree(release());
  }
  T *release() {
    T *p = p_;
    p_ = nullptr;
    return p;
  }

 private:
  T *p_ = nullptr;
};
