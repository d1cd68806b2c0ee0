// Developer check, for a machine WITHOUT a GPU: the threaded host gather of the row shuffle (bear_shuffle_gather_host, bear_shuffle.hip)
// against bear_shuffle_source_row (the host evaluation of the permutation), over row sizes, ranges and thread counts, with guard rows around the destination; the argument
// checks of the range entries.  Built with
// the host sanitizers it also says that no thread reads or writes outside its piece:
//
//   hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -g \
//       scripts/dev/shuffle_gather_check.hip bear_amd/csrc/bear_shuffle.hip -o /tmp/shuffle_gather_check && /tmp/shuffle_gather_check
//   (and once more with -Xarch_host -fsanitize=thread)
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../bear_amd/csrc/bear_dev.h"

static int failures = 0;

static void expect(bool ok, const char *what, uint64_t a = 0, uint64_t b = 0, uint64_t c = 0) {
  if (!ok) {
    ++failures;
    printf("FAIL %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
  }
}

int main() {
  const uint64_t sizes[] = {1, 2, 5, 1365, 4099};
  const uint32_t row_sizes[] = {1, 13, 20, 84};
  const uint64_t seeds[] = {3, 20211012ull << 20};
  const int threads[] = {-1, 0, 1, 3, 16, 64, 1000};
  uint64_t calls = 0;
  for (uint64_t n : sizes)
    for (uint32_t rb : row_sizes) {
      std::vector<uint8_t> src(n * rb);
      for (size_t i = 0; i < src.size(); ++i) src[i] = (uint8_t)(i * 131 + (i >> 8) * 7 + n);
      const uint64_t ranges[][2] = {{0, 0}, {n, 0}, {0, n}, {n - n / 3, n / 3}, {n / 4, n / 2}, {n > 1 ? 1u : 0u, n > 1 ? n - 1 : 0}};
      for (uint64_t seed : seeds)
        for (const auto &r : ranges)
          for (int t : threads) {
            const uint64_t first = r[0], n_out = r[1];
            std::vector<uint8_t> dst((n_out + 2) * rb, 0xA5);           // one guard row on either side
            const int st = bear_shuffle_gather_host(src.data(), dst.data() + rb, n, first, n_out, rb, seed, t);
            ++calls;
            expect(st == BEAR_OK, "status", n, first, n_out);
            bool same = true, guards = true;
            for (uint64_t j = 0; j < n_out && same; ++j)
              same = memcmp(dst.data() + (j + 1) * rb, src.data() + bear_shuffle_source_row(first + j, n, seed) * rb, rb) == 0;
            for (uint32_t b = 0; b < rb; ++b) guards = guards && dst[b] == 0xA5 && dst[(n_out + 1) * rb + b] == 0xA5;
            expect(same, "rows", n, first, n_out);
            expect(guards, "guard rows", n, first, n_out);
          }
    }
  uint8_t a[200], b[240];
  memset(b, 7, sizeof b);
  const uint64_t bad[][2] = {{0, 11}, {5, 6}, {10, 1}, {11, 0}, {~0ull, 2}, {1, ~0ull}};
  for (const auto &r : bad) {
    expect(bear_shuffle_gather_host(a, b, 10, r[0], r[1], 20, 3, 4) == BEAR_ERR_INVALID_ARG, "host gather takes a range beyond the table", r[0], r[1]);
    expect(bear_shuffle_rows_range(a, b, 10, r[0], r[1], 20, 3, nullptr) == BEAR_ERR_INVALID_ARG, "range entry takes a range beyond the table", r[0], r[1]);
  }
  for (size_t i = 0; i < sizeof b; ++i) expect(b[i] == 7, "a refused call wrote", i);
  expect(bear_shuffle_gather_host(a, a, 10, 0, 10, 20, 3, 4) == BEAR_ERR_INVALID_ARG, "dst == src");
  expect(bear_shuffle_gather_host(nullptr, b, 10, 0, 10, 20, 3, 4) == BEAR_ERR_INVALID_ARG, "null src");
  expect(bear_shuffle_rows_range(a, b, 10, 10, 0, 20, 3, nullptr) == BEAR_OK, "an empty range is no launch");
  printf("%llu gathers checked, %d failure(s)\n", (unsigned long long)calls, failures);
  return failures ? 1 : 0;
}
