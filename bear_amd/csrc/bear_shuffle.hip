// bear_shuffle.hip -- the row shuffle (include/bear_hip.h, "On-device shuffle of resident rows"): whole columns permuted on the
// device, a range of the permuted rows gathered from device memory, and the same range gathered by host threads out of a table that
// stays on the host.  The only unit that includes -- and so emits -- kernels_shuffle.h; like the
// counting and the scoring unit it needs bear_dev.h alone of the host side (no workspace, no plan), so
// scripts/dev/shuffle_gather_check.hip links it by itself under the host sanitizers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#include "bear_dev.h"
#include "kernels_shuffle.h"

extern "C" {

// the range's argument checks, shared by the device and the host gather: BEAR_OK with *empty set when there is nothing to move
static int shuffle_range_check(const void *src, void *dst, uint64_t n_rows, uint64_t first, uint64_t n_out, uint32_t row_bytes,
                               bool *empty) {
  *empty = true;
  if (first > n_rows || n_out > n_rows - first) return BEAR_ERR_INVALID_ARG;
  if (n_out == 0 || row_bytes == 0) return BEAR_OK;
  if (!src || !dst || src == dst) return BEAR_ERR_INVALID_ARG;
  if (n_rows > (1ull << 62) / row_bytes) return BEAR_ERR_INVALID_ARG;
  *empty = false;
  return BEAR_OK;
}

int bear_shuffle_rows_range(const void *src, void *dst, uint64_t n_rows, uint64_t first, uint64_t n_out, uint32_t row_bytes,
                            uint64_t seed, void *stream) {
  bool empty;
  const int st = shuffle_range_check(src, dst, n_rows, first, n_out, row_bytes, &empty);
  if (st != BEAR_OK || empty) return st;
  const uint32_t hb = shf_half_bits(n_rows);
  const bool words = (row_bytes % 4 == 0) && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 4 == 0);
  const uint64_t total = words ? n_out * (row_bytes / 4) : n_out * (uint64_t)row_bytes;
  uint64_t blocks = (total + 255) / 256;
  if (blocks > SHF_MAX_BLOCKS) blocks = SHF_MAX_BLOCKS;       // the kernels stride over the rest
  if (words)
    hipLaunchKernelGGL(shuffle_words_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint32_t *>(src), static_cast<uint32_t *>(dst), n_rows, first, n_out, row_bytes / 4, hb,
                       seed);
  else
    hipLaunchKernelGGL(shuffle_bytes_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t *>(src), static_cast<uint8_t *>(dst), n_rows, first, n_out, row_bytes, hb, seed);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_shuffle_rows(const void *src, void *dst, uint64_t n_rows, uint32_t row_bytes, uint64_t seed, void *stream) {
  return bear_shuffle_rows_range(src, dst, n_rows, 0, n_rows, row_bytes, seed, stream);
}

int bear_shuffle_gather_host(const void *src, void *dst, uint64_t n_rows, uint64_t first, uint64_t n_out, uint32_t row_bytes,
                             uint64_t seed, int n_threads) {
  bool empty;
  const int st = shuffle_range_check(src, dst, n_rows, first, n_out, row_bytes, &empty);
  if (st != BEAR_OK || empty) return st;
  const uint32_t hb = shf_half_bits(n_rows);
  const uint8_t *s = static_cast<const uint8_t *>(src);
  uint8_t *d = static_cast<uint8_t *>(dst);
  // rows [j0, j1) of the range: every thread writes its own piece of dst and only reads src
  const auto piece = [=](uint64_t j0, uint64_t j1) {
    for (uint64_t j = j0; j < j1; ++j)
      memcpy(d + j * row_bytes, s + shf_perm(first + j, n_rows, hb, seed) * row_bytes, row_bytes);
  };
  uint64_t t = (uint64_t)(n_threads < 1 ? 1 : n_threads > 64 ? 64 : n_threads);
  if (t > n_out) t = n_out;
  const uint64_t step = (n_out + t - 1) / t;
  std::vector<std::thread> pool;
  try {
    for (uint64_t j0 = step; j0 < n_out; j0 += step) pool.emplace_back(piece, j0, j0 + step < n_out ? j0 + step : n_out);
  } catch (...) {
    // a thread that could not be started: the pieces without one are gathered here, after the first
    const uint64_t done = (uint64_t)(pool.size() + 1) * step;
    if (done < n_out) piece(done, n_out);
  }
  piece(0, step < n_out ? step : n_out);
  for (auto &th : pool) th.join();
  return BEAR_OK;
}

uint64_t bear_shuffle_source_row(uint64_t i, uint64_t n_rows, uint64_t seed) {
  return (n_rows == 0 || i >= n_rows) ? i : shf_perm(i, n_rows, shf_half_bits(n_rows), seed);
}

}  // extern "C"
