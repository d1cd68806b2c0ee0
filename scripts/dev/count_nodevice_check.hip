// Developer check, for a machine WITHOUT a GPU: every allocating entry of the counting unit (bear_count.hip) with valid arguments,
// and the argument checks of the entries that count in passes over key ranges.
// The first device call of each fails there, so this walks the error paths: a non-OK status, the out-handle NULL or emptied, the
// HIP error recorded, and -- built with the host sanitizers -- nothing leaked or touched after its release on the way out.
//
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -g \
//       scripts/dev/count_nodevice_check.hip bear_amd/csrc/bear_count.hip -o /tmp/count_nodevice_check && /tmp/count_nodevice_check
//
// bear_count_last_hip_error() is read because bear_count.hip defines it; it returns the library's one slot, the one behind
// bear_last_hip_error() (bear_dev.h).  On a machine with a GPU the calls succeed and the program says so and fails.
#include <stdio.h>
#include <stdlib.h>

#include "../../bear_amd/csrc/bear_dev.h"
#include "../../bear_amd/csrc/bear_levels.h"

static int failures = 0;

static void expect(bool ok, const char *entry, const char *what) {
  if (!ok) {
    ++failures;
    printf("FAIL %s: %s\n", entry, what);
  }
}

// a call that must have failed: its status, and the error slot (cleared before every call)
static void failed(const char *entry, int st) {
  expect(st != BEAR_OK, entry, "returned BEAR_OK without a device");
  expect(bear_count_last_hip_error() != 0, entry, "left no HIP error");
  expect(bear_count_last_hip_error() == g_last_hip_error, entry, "bear_count_last_hip_error() is not the library's slot");
  printf("%-28s status %d, HIP error %d\n", entry, st, bear_count_last_hip_error());
  g_last_hip_error = 0;
}

int main() {
  enum { N = 1000 };
  static uint8_t text[N], group[N];               // (never read: the first allocation fails)
  static unsigned long long codes[N];
  for (int i = 0; i < N; ++i) text[i] = (uint8_t)(i % 4), codes[i] = (unsigned long long)(i / 3);
  text[0] = 5;

  bear_kmer_sort *h = reinterpret_cast<bear_kmer_sort *>(1);
  uint64_t n_rows = 7;
  failed("bear_kmer_sort_create", bear_kmer_sort_create(text, group, N, 3, &h, &n_rows, nullptr));
  expect(h == nullptr && n_rows == 0, "bear_kmer_sort_create", "handle or row count left set");
  for (int width : {5, 21}) {
    h = reinterpret_cast<bear_kmer_sort *>(1);
    failed("bear_kmer_sort_create_wide", bear_kmer_sort_create_wide(text, group, N, 3, width, &h, &n_rows, nullptr));
    expect(h == nullptr && n_rows == 0, "bear_kmer_sort_create_wide", "handle or row count left set");
  }

  // the passes over key ranges: first the argument checks, which come before any device call and leave no HIP error ...
  uint64_t bytes = 7, hist[64];
  auto refused = [&](const char *entry, int st) {
    expect(st == BEAR_ERR_INVALID_ARG, entry, "a bad argument was not BEAR_ERR_INVALID_ARG");
    expect(bear_count_last_hip_error() == 0, entry, "an argument check reached the device");
  };
  refused("bear_kmer_sort_bytes", bear_kmer_sort_bytes(N, 3, 7, &bytes));
  refused("bear_kmer_sort_bytes", bear_kmer_sort_bytes(N, 13, 21, &bytes));
  refused("bear_kmer_sort_bytes", bear_kmer_sort_bytes(N, 0, 5, &bytes));
  refused("bear_kmer_sort_bytes", bear_kmer_sort_bytes(0xffffffffull, 3, 5, &bytes));
  refused("bear_kmer_sort_bytes", bear_kmer_sort_bytes(N, 3, 5, nullptr));
  expect(bear_kmer_sort_bytes(0, 3, 5, &bytes) == BEAR_OK && bytes == 0, "bear_kmer_sort_bytes", "no pairs need no bytes");
  refused("bear_kmer_bin_hist", bear_kmer_bin_hist(text, N, 2, 5, hist, 63, nullptr));          // 2 letters of 3 bits: 64 bins
  refused("bear_kmer_bin_hist", bear_kmer_bin_hist(text, N, 2, 7, hist, 64, nullptr));
  refused("bear_kmer_bin_hist", bear_kmer_bin_hist(text, N, 22, 5, hist, 1 << 18, nullptr));
  refused("bear_kmer_bin_hist", bear_kmer_bin_hist(text, N, 2, 5, nullptr, 64, nullptr));
  refused("bear_kmer_bin_hist", bear_kmer_bin_hist(nullptr, N, 2, 5, hist, 64, nullptr));
  struct { int lag, width; uint64_t lo, hi, cap; } bad[] = {{2, 5, 0, 65, 10}, {2, 5, 8, 8, 10},  {2, 5, 9, 8, 10}, {2, 7, 0, 64, 10},
                                                           {13, 21, 0, 1, 10}, {0, 5, 0, 1, 10},  {2, 5, 0, 64, 0xffffffffull}};
  for (const auto &b : bad) {
    h = reinterpret_cast<bear_kmer_sort *>(1);
    n_rows = 7;
    refused("bear_kmer_sort_create_range", bear_kmer_sort_create_range(text, group, N, b.lag, b.width, b.lo, b.hi, b.cap, &h, &n_rows, nullptr));
    expect(h == nullptr && n_rows == 0, "bear_kmer_sort_create_range", "handle or row count left set");
  }
  refused("bear_kmer_sort_create_range", bear_kmer_sort_create_range(text, group, N, 2, 5, 0, 64, 10, nullptr, &n_rows, nullptr));
  refused("bear_kmer_sort_create_range", bear_kmer_sort_create_range(nullptr, group, N, 2, 5, 0, 64, 10, &h, &n_rows, nullptr));
  // ... then valid arguments, which fail at the first device call
  failed("bear_kmer_bin_hist", bear_kmer_bin_hist(text, N, 2, 5, hist, 64, nullptr));
  for (int width : {5, 21}) {
    h = reinterpret_cast<bear_kmer_sort *>(1);
    n_rows = 7;
    failed("bear_kmer_sort_create_range", bear_kmer_sort_create_range(text, group, N, 3, width, 0, 8, 100, &h, &n_rows, nullptr));
    expect(h == nullptr && n_rows == 0, "bear_kmer_sort_create_range", "handle or row count left set");
  }

  bear_level_dev lv;
  failed("bear_level_build", bear_level_build(codes, N, 4, &lv, nullptr));
  expect(!lv.n && !lv.codes && !lv.parent_of_below && !lv.child_start && !lv.rows, "bear_level_build", "level not emptied");
  bear_window_dev wt;
  failed("bear_window_build", bear_window_build(codes, N, 1, 3, &wt, nullptr));
  expect(!wt.n && !wt.codes && !wt.row_of_context && !wt.perm && !wt.child_start && !wt.rows, "bear_window_build", "table not emptied");

  for (int width : {4, 8, 16}) failed("bear_canonical_order", bear_canonical_order(codes, N * 8 / width, width, nullptr));

  uint64_t need = 0;
  uint32_t perm[N];
  expect(bear_kmer_order_u64(reinterpret_cast<const uint64_t *>(codes), N, 5, perm, nullptr, &need, nullptr) == BEAR_OK && need > 0,
         "bear_kmer_order_u64", "size query");
  void *scratch = aligned_alloc(256, (need + 255) & ~255ull);     // (host memory: the launch that would write it fails)
  failed("bear_kmer_order_u64", bear_kmer_order_u64(reinterpret_cast<const uint64_t *>(codes), N, 5, perm, scratch, &need, nullptr));
  free(scratch);

  if (failures) printf("%d check(s) failed\n", failures);
  else printf("all error paths clean\n");
  return failures ? 1 : 0;
}
