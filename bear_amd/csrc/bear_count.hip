// bear_count.hip -- k-mer transition counting on the device: the count table of summarize.py built straight from the
// sequences.
//
// The reference gets there in three stages (bear_model/summarize.py): (1) write prefix / suffix / full FASTQ files per
// input, (2) run the external KMC counter on each, (3) heap-merge the sorted KMC dumps into rows
// `kmer \t [[A,C,G,T,$ per group]...]` (Register / Consolidate, summarize.py:380-622).  What the three stages compute is
// stated by the reference's own test (bear_model/tests/test_summarize.py:88-115): for every sequence and lag L,
//     full = '[' * L + seq + ']' ;  for j in [L, len(full)):  counts[full[j-L:j]][group][full[j]] += 1 .
// On an MI355X that is one pass per lag over the resident text: every transition becomes a (context code, group * 5 +
// next letter) pair, the pairs are radix-sorted by context (rocPRIM radix_sort_pairs: a library sort is the right tool for
// the sort itself), and a run-length pass turns runs of equal contexts into rows and scatters the pair values into the
// planar uint32 [group][row][5] slabs the training kernels consume -- no KMC, no intermediate files, and the table can
// go to training without ever being text.
//
// Text layout [dev]: per sequence  5 (start marker), letters 0..3 (6 = any other character), 4 (stop).  A transition sits
// at every position holding 0..4; its context is the L codes before it, read back until the start marker, the rest
// filled with the start symbol.  Transitions whose context or next letter contains a 6 are dropped (KMC drops k-mers
// with non-ACGT letters likewise).  The protein alphabet takes the same pass with 5 bits per letter and rows of 21
// (bear_kmer_sort_create_wide: residues 0..19, stop 20, start marker 21, 22 = any other character; value group * 21 + next).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>

#include <new>

#include "bear_dev.h"
#include "bear_levels.h"

namespace {
// rocPRIM's two calls: `call(NULL, bytes)` asks for the size of the temporary storage, `call(temp, bytes)` enqueues the work.
// The caller owns `temp`: it is in use until the stream has been synchronised, and goes where the caller says.
template <typename Call>
hipError_t rocprim_run(dev_buf<unsigned char> &temp, Call call) {
  size_t bytes = 0;
  hipError_t e = call(nullptr, bytes);
  if (e != hipSuccess) return e;
  e = temp.alloc(bytes ? bytes : 8);
  if (e != hipSuccess) return e;
  return call(temp.get(), bytes);
}

// The same pass serves two alphabets (template over bits per letter and row width W; the start marker is W, the stop and
// the '[' of a context are both W - 1, any other character is W + 1):
//   W = 5,  3 bits: A,C,G,T = 0..3, stop 4, start marker 5, other 6            (bear_kmer_sort_create, lags 1..21)
//   W = 21, 5 bits: ARNDCEQGHILKMFPSTWYV = 0..19, stop 20, start marker 21, other 22   (bear_kmer_sort_create_wide, lags 1..12)
template <int BITS, int W>
struct cnt_alphabet;
template <>
struct cnt_alphabet<3, 5> {
  static constexpr int MAX_LAG = 21;
  __device__ static uint8_t ascii(uint32_t c) { return (uint8_t)("ACGT["[c]); }
};
template <>
struct cnt_alphabet<5, 21> {
  static constexpr int MAX_LAG = 12;
  __device__ static uint8_t ascii(uint32_t c) { return (uint8_t)("ARNDCEQGHILKMFPSTWYV["[c < 21u ? c : 20u]); }
};

// dropped transitions carry a key with only bit BITS*lag set: it sorts behind every context, and the radix sort needs to
// look at BITS*lag + 1 bits only (5 passes instead of 8 at lag 13 of the 3-bit alphabet)
template <int BITS>
__host__ __device__ inline uint64_t cnt_invalid(int lag) { return 1ull << (BITS * lag); }

// key: the context as the packed k-mer code (letter l of the k-mer in bits [BITS l, BITS l + BITS); W - 1 = '['): at 3 bits
// the code of bear_pack_kmers_u64.  `nx` is text[t], `next` the letter of the pair's value (0 where nx is none); a dropped
// transition gets cnt_invalid.  One routine for every kernel
// that forms keys: the passes over key ranges below must cut the very order the single pass sorts into.
template <int BITS, int W>
__device__ __forceinline__ uint64_t cnt_key(const uint8_t *__restrict__ text, uint64_t t, uint32_t nx, int lag, uint32_t &next) {
  constexpr uint32_t STOP = W - 1, START = W;
  const uint64_t CNT_INVALID = cnt_invalid<BITS>(lag);
  uint64_t key = CNT_INVALID;
  next = 0u;
  if (nx <= STOP) {
    next = nx;
    key = 0;
    bool started = false, bad = false;
    for (int i = 1; i <= lag; ++i) {                 // letter lag - i of the k-mer
      uint32_t c = STOP;
      if (!started) {
        c = (t >= (uint64_t)i) ? text[t - i] : START;
        if (c == START) {
          started = true;
          c = STOP;
        }
      }
      bad |= c > STOP;
      key |= (uint64_t)c << (BITS * (lag - i));
    }
    if (bad) key = CNT_INVALID;
  }
  return key;
}

template <int BITS, int W>
__global__ __launch_bounds__(256) void cnt_emit_kernel(const uint8_t *__restrict__ text, const uint8_t *__restrict__ grp,
                                                       uint64_t n_pos, int lag, uint64_t *__restrict__ keys,
                                                       uint32_t *__restrict__ vals) {
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < n_pos; t += (uint64_t)gridDim.x * 256) {
    uint32_t next;
    keys[t] = cnt_key<BITS, W>(text, t, text[t], lag, next);
    vals[t] = (uint32_t)grp[t] * (uint32_t)W + next;
  }
}

// ---- counting in passes over key ranges.  The sort order is the key order, so the table of the keys whose leading bits fall
// into [bin_lo, bin_hi) is a contiguous slice of the whole table, and the slices of disjoint ascending ranges, concatenated, are
// the table: nothing is merged and nothing approximated.  The bin of a valid key is its top BITS * HL bits below the invalid
// bit, HL = min(lag, BIN_LETTERS): the LAST letters of the context, the most significant ones of the sort.
template <int BITS>
struct cnt_bins;
template <>
struct cnt_bins<3> { static constexpr int LETTERS = BEAR_COUNT_BIN_LETTERS; };
template <>
struct cnt_bins<5> { static constexpr int LETTERS = BEAR_COUNT_BIN_LETTERS_WIDE; };
template <int BITS>
__host__ __device__ inline int cnt_bin_letters(int lag) { return lag < cnt_bins<BITS>::LETTERS ? lag : cnt_bins<BITS>::LETTERS; }
template <int BITS>
__host__ __device__ inline int cnt_bin_shift(int lag) { return BITS * (lag - cnt_bin_letters<BITS>(lag)); }
constexpr uint64_t CNT_NO_BIN = ~0ull;      // the bin of a dropped transition: in no range, counted nowhere

// Both kernels below run a loop that is uniform over the block (whole blocks of 256 positions, lanes past the end idle inside
// it), so that every lane of a wave reaches the ballots.  Waves have 64 lanes on gfx950.
//
// hist[bin] += valid transitions of that bin.  The histogram (up to 2^18 bins of 8 bytes) does not fit LDS, so the adds go to
// global memory; what is cheap to fold first is a run of neighbouring lanes with one bin (a homopolymer, the '[' contexts of
// short reads): the first lane of a run adds the run's length.
template <int BITS, int W>
__global__ __launch_bounds__(256) void cnt_bin_hist_kernel(const uint8_t *__restrict__ text, uint64_t n_pos, int lag,
                                                           unsigned long long *__restrict__ hist) {
  const uint64_t CNT_INVALID = cnt_invalid<BITS>(lag);
  const int shift = cnt_bin_shift<BITS>(lag);
  const unsigned lane = threadIdx.x & 63u;
  for (uint64_t base = (uint64_t)blockIdx.x * 256; base < n_pos; base += (uint64_t)gridDim.x * 256) {
    const uint64_t t = base + threadIdx.x;
    uint64_t bin = CNT_NO_BIN;
    if (t < n_pos) {
      uint32_t next;
      const uint64_t key = cnt_key<BITS, W>(text, t, text[t], lag, next);
      if (key != CNT_INVALID) bin = key >> shift;
    }
    const uint64_t before = __shfl_up(bin, 1);
    const bool head = lane == 0 || before != bin;
    const unsigned long long heads = __ballot(head);
    if (head && bin != CNT_NO_BIN) {
      const unsigned long long later = heads & ~((2ull << lane) - 1ull);       // run starts above this lane
      const unsigned next = later ? (unsigned)__ffsll((long long)later) - 1u : 64u;
      atomicAdd(&hist[bin], (unsigned long long)(next - lane));
    }
  }
}

// The pairs of one bin range, compacted.  A wave takes CNT_RANGE_CHUNKS chunks of 64 positions per step: a ballot of the lanes
// that write in each chunk, then ONE add on the 64-bit cursor, by lane 0, for all of them (every wave of the grid adds to that
// one address and waits for the answer: one add per 64 positions alone took 20 ms per 1e8 positions, more than the sort), the
// base broadcast, and each lane's slot from the chunks before its own and the writing lanes below it.  A slot at or beyond
// `capacity` is not written, whatever the text holds; the host compares the final cursor with the capacity.  Dropped transitions
// are not emitted, so the sort of a range reads BITS * lag bits.  The order of the pairs in front of the sort depends on which
// wave reaches the cursor first; the table does not: the sort orders by key, pairs of equal keys differ only in their values,
// and cnt_scatter_kernel adds each value's integer count to its cell -- a sum of ones, the same in any order.
constexpr int CNT_RANGE_CHUNKS = 8;
template <int BITS, int W>
__global__ __launch_bounds__(256) void cnt_emit_range_kernel(const uint8_t *__restrict__ text, const uint8_t *__restrict__ grp,
                                                             uint64_t n_pos, int lag, uint64_t bin_lo, uint64_t bin_hi,
                                                             uint64_t capacity, unsigned long long *__restrict__ cursor,
                                                             uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
  constexpr uint64_t STEP = 256ull * CNT_RANGE_CHUNKS;      // positions of a block per step: chunk c of a wave lies c * 256 further on
  const uint64_t CNT_INVALID = cnt_invalid<BITS>(lag);
  const int shift = cnt_bin_shift<BITS>(lag);
  const unsigned lane = threadIdx.x & 63u;
  for (uint64_t base = (uint64_t)blockIdx.x * STEP; base < n_pos; base += (uint64_t)gridDim.x * STEP) {
    uint64_t key[CNT_RANGE_CHUNKS];
    uint32_t next[CNT_RANGE_CHUNKS];
    unsigned long long mask[CNT_RANGE_CHUNKS];
    unsigned n_write = 0;
#pragma unroll
    for (int c = 0; c < CNT_RANGE_CHUNKS; ++c) {
      const uint64_t t = base + (uint64_t)c * 256 + threadIdx.x;
      key[c] = CNT_INVALID;
      next[c] = 0;
      if (t < n_pos) key[c] = cnt_key<BITS, W>(text, t, text[t], lag, next[c]);
      if (key[c] != CNT_INVALID && ((key[c] >> shift) < bin_lo || (key[c] >> shift) >= bin_hi)) key[c] = CNT_INVALID;   // not this pass's
      mask[c] = __ballot(key[c] != CNT_INVALID);
      n_write += (unsigned)__popcll(mask[c]);
    }
    if (n_write == 0u) continue;                        // (uniform over the wave)
    unsigned long long first = 0ull;
    if (lane == 0) first = atomicAdd(cursor, (unsigned long long)n_write);
    first = __shfl(first, 0);
#pragma unroll
    for (int c = 0; c < CNT_RANGE_CHUNKS; ++c) {
      const uint64_t slot = first + (uint64_t)__popcll(mask[c] & ((1ull << lane) - 1ull));
      if (key[c] != CNT_INVALID && slot < capacity) {
        keys[slot] = key[c];
        vals[slot] = (uint32_t)grp[base + (uint64_t)c * 256 + threadIdx.x] * (uint32_t)W + next[c];
      }
      first += (uint64_t)__popcll(mask[c]);
    }
  }
}

template <int BITS>
__global__ __launch_bounds__(256) void cnt_flag_kernel(const uint64_t *__restrict__ keys, uint64_t n, int lag,
                                                       uint32_t *__restrict__ flags) {
  const uint64_t CNT_INVALID = cnt_invalid<BITS>(lag);
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (uint64_t)gridDim.x * 256) {
    const uint64_t k = keys[t];
    flags[t] = (k != CNT_INVALID && (t == 0 || keys[t - 1] != k)) ? 1u : 0u;
  }
}

// rows: inclusive scan of the run-start flags (row index + 1).  One thread per sorted pair.
template <int BITS, int W>
__global__ __launch_bounds__(256) void cnt_scatter_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                          const uint32_t *__restrict__ rows, uint64_t n, uint64_t n_rows, int lag,
                                                          uint32_t n_groups, uint8_t *__restrict__ kmers, uint64_t *__restrict__ codes,
                                                          uint32_t *__restrict__ counts) {
  const uint64_t CNT_INVALID = cnt_invalid<BITS>(lag);
  constexpr uint32_t UW = W;
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (uint64_t)gridDim.x * 256) {
    const uint64_t k = keys[t];
    if (k == CNT_INVALID) continue;
    const uint64_t row = (uint64_t)rows[t] - 1u;
    const uint32_t v = vals[t];
    if (v / UW < n_groups) atomicAdd(&counts[((uint64_t)(v / UW) * n_rows + row) * UW + (v % UW)], 1u);   // group ids beyond n_groups are ignored
    if (t == 0 || keys[t - 1] != k) {                // run start: name the row
      if (BITS == 3 && codes) {                      // (the packed code belongs to the 4-letter fused heads: the host passes none at 5 bits)
        uint64_t packed = k;
        for (int l = lag; l < 21; ++l) packed |= 5ull << (3 * l);     // positions >= lag hold 5 (bear_pack_kmers_u64)
        codes[row] = packed;
      }
      if (kmers)
        for (int l = 0; l < lag; ++l)
          kmers[row * (uint64_t)lag + l] = cnt_alphabet<BITS, W>::ascii((uint32_t)(k >> (BITS * l)) & ((1u << BITS) - 1u));
    }
  }
}

unsigned grid_for(uint64_t n) {
  uint64_t b = (n + 255) / 256;
  return (unsigned)(b > (1u << 20) ? (1u << 20) : (b ? b : 1));
}
}  // namespace

struct bear_kmer_sort {
  uint64_t n_pos, n_rows;
  int lag, width;   // width: counts per row, 5 (3-bit keys) or 21 (5-bit keys)
  uint64_t *keys;   // sorted
  uint32_t *vals;   // sorted with the keys
  uint32_t *rows;   // inclusive scan of run starts
};

namespace {
// sort + run starts of `n` emitted pairs (n > 0), the common tail of a pass over the whole text and of a pass over one bin
// range: keys / vals / rows are what the handle keeps, *last = the number of rows
template <int BITS>
int sort_and_rows(dev_buf<uint64_t> &keys_in, dev_buf<uint32_t> &vals_in, dev_buf<uint64_t> &keys, dev_buf<uint32_t> &vals,
                  dev_buf<uint32_t> &rows, uint64_t n, unsigned key_bits, int lag, uint32_t *last, hipStream_t s) {
  dev_buf<unsigned char> temp;
  HIP_TRY(rocprim_run(temp, [&](void *t, size_t &tb) {
    return rocprim::radix_sort_pairs(t, tb, keys_in.get(), keys.get(), vals_in.get(), vals.get(), n, 0u, key_bits, s);
  }));
  HIP_TRY(hipStreamSynchronize(s));
  temp.reset();            // the sort's storage and its input keys go before `rows` comes: the peak of the pass
  keys_in.reset();
  dev_buf<uint32_t> &flags = vals_in;   // reuse
  HIP_TRY(rows.alloc(n));
  hipLaunchKernelGGL((cnt_flag_kernel<BITS>), dim3(grid_for(n)), dim3(256), 0, s, keys.get(), n, lag, flags.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(rocprim_run(temp, [&](void *t, size_t &tb) {
    return rocprim::inclusive_scan(t, tb, flags.get(), rows.get(), n, rocprim::plus<uint32_t>(), s);
  }));
  HIP_TRY(hipMemcpyAsync(last, rows.get() + (n - 1), 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return BEAR_OK;
}

int new_handle(bear_kmer_sort **out, uint64_t *n_rows_out, uint64_t n, uint32_t n_rows, int lag, int width, dev_buf<uint64_t> &keys,
               dev_buf<uint32_t> &vals, dev_buf<uint32_t> &rows) {
  *out = new (std::nothrow) bear_kmer_sort{n, n_rows, lag, width, keys.get(), vals.get(), rows.get()};
  if (!*out) return BEAR_ERR_NOMEM;
  (void)keys.release(), (void)vals.release(), (void)rows.release();
  *n_rows_out = n_rows;
  return BEAR_OK;
}

// emit + sort + run starts of one lag (every argument checked by the caller, before any device call)
template <int BITS, int W>
int kmer_sort_create(const uint8_t *text, const uint8_t *group, uint64_t n_pos, int lag, bear_kmer_sort **out, uint64_t *n_rows_out,
                     hipStream_t s) {
  dev_buf<uint64_t> keys_in, keys;
  dev_buf<uint32_t> vals_in, vals, rows;
  uint32_t last = 0;
  if (n_pos) {
    HIP_TRY(keys_in.alloc(n_pos));
    HIP_TRY(vals_in.alloc(n_pos));
    HIP_TRY(keys.alloc(n_pos));
    HIP_TRY(vals.alloc(n_pos));
    hipLaunchKernelGGL((cnt_emit_kernel<BITS, W>), dim3(grid_for(n_pos)), dim3(256), 0, s, text, group, n_pos, lag, keys_in.get(), vals_in.get());
    HIP_TRY(hipGetLastError());
    const int st = sort_and_rows<BITS>(keys_in, vals_in, keys, vals, rows, n_pos, (unsigned)(BITS * lag + 1), lag, &last, s);
    if (st != BEAR_OK) return st;
  }
  return new_handle(out, n_rows_out, n_pos, last, lag, W, keys, vals, rows);
}

// the same over the transitions whose bin lies in [bin_lo, bin_hi): buffers for `capacity` pairs, not for n_pos positions, and
// no invalid keys among them (BITS * lag key bits).  A pass that meets another number of pairs than `capacity` wrote at most
// `capacity` of them and leaves no handle: the text and the histogram the capacity came from do not belong together.
template <int BITS, int W>
int kmer_sort_create_range(const uint8_t *text, const uint8_t *group, uint64_t n_pos, int lag, uint64_t bin_lo, uint64_t bin_hi,
                           uint64_t capacity, bear_kmer_sort **out, uint64_t *n_rows_out, hipStream_t s) {
  dev_buf<uint64_t> keys_in, keys;
  dev_buf<uint32_t> vals_in, vals, rows;
  dev_buf<unsigned long long> cursor;
  unsigned long long n_pairs = 0;
  uint32_t last = 0;
  if (capacity) {
    HIP_TRY(keys_in.alloc(capacity));
    HIP_TRY(vals_in.alloc(capacity));
    HIP_TRY(keys.alloc(capacity));
    HIP_TRY(vals.alloc(capacity));
  }
  if (n_pos) {
    HIP_TRY(cursor.alloc(1));
    HIP_TRY(hipMemsetAsync(cursor.get(), 0, sizeof(unsigned long long), s));
    const unsigned blocks = grid_for((n_pos + CNT_RANGE_CHUNKS - 1) / CNT_RANGE_CHUNKS);      // (a block takes 256 * CNT_RANGE_CHUNKS positions per step)
    hipLaunchKernelGGL((cnt_emit_range_kernel<BITS, W>), dim3(blocks), dim3(256), 0, s, text, group, n_pos, lag, bin_lo, bin_hi, capacity,
                       cursor.get(), keys_in.get(), vals_in.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&n_pairs, cursor.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  if (n_pairs != capacity) return BEAR_ERR_INVALID_ARG;
  if (capacity) {
    const int st = sort_and_rows<BITS>(keys_in, vals_in, keys, vals, rows, capacity, (unsigned)(BITS * lag), lag, &last, s);
    if (st != BEAR_OK) return st;
  }
  return new_handle(out, n_rows_out, capacity, last, lag, W, keys, vals, rows);
}

// peak device bytes of a pass over n pairs: the four key / value buffers with the sort's storage, or, after the sort, what is
// left of them with `rows` and the scan's storage -- the allocations of sort_and_rows, in its order
template <int BITS>
int kmer_sort_bytes(uint64_t n, int lag, uint64_t *bytes_out) {
  size_t sort_b = 0, scan_b = 0;
  HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_b, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, n, 0u,
                                    (unsigned)(BITS * lag + 1), (hipStream_t) nullptr));
  HIP_TRY(rocprim::inclusive_scan(nullptr, scan_b, (uint32_t *)nullptr, (uint32_t *)nullptr, n, rocprim::plus<uint32_t>(), (hipStream_t) nullptr));
  const uint64_t at_sort = 24 * n + sort_b, at_scan = 20 * n + scan_b;
  *bytes_out = at_sort > at_scan ? at_sort : at_scan;
  return BEAR_OK;
}

bool sort_args_ok(const uint8_t *text, const uint8_t *group, uint64_t n_pos, int lag, int max_lag, bear_kmer_sort **out,
                  uint64_t *n_rows_out) {
  if (!out || !n_rows_out || lag < 1 || lag > max_lag) return false;
  *out = nullptr;
  *n_rows_out = 0;
  if (n_pos && (!text || !group)) return false;
  return n_pos < 0xffffffffull;   // row indices are 32-bit: shard the text above 4e9 positions
}

// the passes over bin ranges: width 5 or 21 with the lag limits of bear_kmer_sort_create_wide; the number of bins of a lag
bool range_width_lag_ok(int lag, int width) {
  if (width != 5 && width != 21) return false;
  return lag >= 1 && lag <= (width == 5 ? cnt_alphabet<3, 5>::MAX_LAG : cnt_alphabet<5, 21>::MAX_LAG);
}
uint64_t range_n_bins(int lag, int width) {
  return 1ull << (width == 5 ? 3 * cnt_bin_letters<3>(lag) : 5 * cnt_bin_letters<5>(lag));
}
}  // namespace

extern "C" {

int bear_count_last_hip_error(void) { return g_last_hip_error; }   // the library's one slot: bear_last_hip_error()

int bear_kmer_sort_create(const uint8_t *text, const uint8_t *group, uint64_t n_pos, int lag, bear_kmer_sort **out,
                          uint64_t *n_rows_out, void *stream) {
  if (!sort_args_ok(text, group, n_pos, lag, cnt_alphabet<3, 5>::MAX_LAG, out, n_rows_out)) return BEAR_ERR_INVALID_ARG;
  return kmer_sort_create<3, 5>(text, group, n_pos, lag, out, n_rows_out, static_cast<hipStream_t>(stream));
}

int bear_kmer_sort_create_wide(const uint8_t *text, const uint8_t *group, uint64_t n_pos, int lag, int width, bear_kmer_sort **out,
                               uint64_t *n_rows_out, void *stream) {
  if (width != 5 && width != 21) return BEAR_ERR_INVALID_ARG;
  const int max_lag = width == 5 ? cnt_alphabet<3, 5>::MAX_LAG : cnt_alphabet<5, 21>::MAX_LAG;   // 5 * 12 + 1 key bits fill one uint64
  if (!sort_args_ok(text, group, n_pos, lag, max_lag, out, n_rows_out)) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return width == 5 ? kmer_sort_create<3, 5>(text, group, n_pos, lag, out, n_rows_out, s)
                    : kmer_sort_create<5, 21>(text, group, n_pos, lag, out, n_rows_out, s);
}

int bear_kmer_sort_bytes(uint64_t n_pairs, int lag, int width, uint64_t *bytes_out) {
  if (!bytes_out || !range_width_lag_ok(lag, width) || n_pairs >= 0xffffffffull) return BEAR_ERR_INVALID_ARG;
  *bytes_out = 0;
  if (n_pairs == 0) return BEAR_OK;
  return width == 5 ? kmer_sort_bytes<3>(n_pairs, lag, bytes_out) : kmer_sort_bytes<5>(n_pairs, lag, bytes_out);
}

int bear_kmer_bin_hist(const uint8_t *text, uint64_t n_pos, int lag, int width, uint64_t *hist, uint64_t n_bins, void *stream) {
  if (!range_width_lag_ok(lag, width) || !hist || (n_pos && !text) || n_bins != range_n_bins(lag, width)) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipMemsetAsync(hist, 0, n_bins * sizeof(uint64_t), s));
  if (n_pos == 0) return BEAR_OK;
  unsigned long long *h = reinterpret_cast<unsigned long long *>(hist);
  if (width == 5)
    hipLaunchKernelGGL((cnt_bin_hist_kernel<3, 5>), dim3(grid_for(n_pos)), dim3(256), 0, s, text, n_pos, lag, h);
  else
    hipLaunchKernelGGL((cnt_bin_hist_kernel<5, 21>), dim3(grid_for(n_pos)), dim3(256), 0, s, text, n_pos, lag, h);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_kmer_sort_create_range(const uint8_t *text, const uint8_t *group, uint64_t n_pos, int lag, int width, uint64_t bin_lo,
                                uint64_t bin_hi, uint64_t capacity, bear_kmer_sort **out, uint64_t *n_rows_out, void *stream) {
  if (!out || !n_rows_out) return BEAR_ERR_INVALID_ARG;
  *out = nullptr;
  *n_rows_out = 0;
  if (!range_width_lag_ok(lag, width) || (n_pos && (!text || !group))) return BEAR_ERR_INVALID_ARG;
  if (bin_lo >= bin_hi || bin_hi > range_n_bins(lag, width) || capacity >= 0xffffffffull) return BEAR_ERR_INVALID_ARG;   // (32-bit row indices)
  hipStream_t s = static_cast<hipStream_t>(stream);
  return width == 5 ? kmer_sort_create_range<3, 5>(text, group, n_pos, lag, bin_lo, bin_hi, capacity, out, n_rows_out, s)
                    : kmer_sort_create_range<5, 21>(text, group, n_pos, lag, bin_lo, bin_hi, capacity, out, n_rows_out, s);
}

int bear_kmer_sort_reduce(const bear_kmer_sort *h, int n_groups, uint8_t *kmers, uint64_t *kmer_code, uint32_t *counts,
                          void *stream) {
  if (!h || n_groups < 1 || n_groups > 255) return BEAR_ERR_INVALID_ARG;
  if (h->width != 5 && kmer_code) return BEAR_ERR_INVALID_ARG;   // the packed 3-bit code is the 4-letter fused heads' only
  if (h->n_rows == 0) return BEAR_OK;
  if (!counts) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n_groups * h->n_rows * (size_t)h->width * 4, s));
  if (h->width == 5)
    hipLaunchKernelGGL((cnt_scatter_kernel<3, 5>), dim3(grid_for(h->n_pos)), dim3(256), 0, s, h->keys, h->vals, h->rows, h->n_pos,
                       h->n_rows, h->lag, (uint32_t)n_groups, kmers, kmer_code, counts);
  else
    hipLaunchKernelGGL((cnt_scatter_kernel<5, 21>), dim3(grid_for(h->n_pos)), dim3(256), 0, s, h->keys, h->vals, h->rows, h->n_pos,
                       h->n_rows, h->lag, (uint32_t)n_groups, kmers, kmer_code, counts);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_kmer_sort_destroy(bear_kmer_sort *h) {
  if (!h) return BEAR_OK;
  if (h->keys) (void)hipFree(h->keys);
  if (h->vals) (void)hipFree(h->vals);
  if (h->rows) (void)hipFree(h->rows);
  delete h;
  return BEAR_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ k-mer order of a batch (fused AR-function kernels)
// The sums of a training step do not depend on the order of a batch's rows, and the fused linear / convolutional kernels run
// about twice as fast when consecutive contexts share their leading letters (kernels_linear.h phase C, kernels_cnn.h shared
// windows).  bear_kmer_order_u64 returns the permutation that sorts packed contexts lexicographically, FIRST letter most
// significant (a radix sort over 3 lag bits of the letter-reversed code); bear_gather_rows applies a permutation to any
// row-major slab (count rows, packed contexts, k-mer bytes) -- once per batch, before its plan is built.
namespace {
__global__ __launch_bounds__(256) void order_keys_kernel(const unsigned long long *__restrict__ code, uint64_t n, int lag,
                                                         unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const unsigned long long w = code[i];
    unsigned long long k = 0ull;
    for (int l = 0; l < lag; ++l) k = (k << 3) | ((w >> (3 * l)) & 7ull);      // letter 0 ends up in the top field
    keys[i] = k;
    vals[i] = (uint32_t)i;
  }
}
__global__ __launch_bounds__(256) void gather_rows_kernel(const unsigned char *__restrict__ src, const uint32_t *__restrict__ perm,
                                                          unsigned char *__restrict__ dst, uint64_t n_rows, uint32_t row_bytes) {
  if ((row_bytes & 3u) == 0u) {      // word rows: one thread per 4-byte word, consecutive threads on consecutive words of a row
    const uint32_t wpr = row_bytes >> 2;
    const uint64_t total = n_rows * wpr;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256) {
      const uint64_t r = t / wpr;
      const uint32_t k = (uint32_t)(t - r * wpr);
      reinterpret_cast<uint32_t *>(dst)[t] = reinterpret_cast<const uint32_t *>(src)[(uint64_t)perm[r] * wpr + k];
    }
  } else {
    const uint64_t total = n_rows * row_bytes;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256) {
      const uint64_t r = t / row_bytes;
      dst[t] = src[(uint64_t)perm[r] * row_bytes + (t - r * row_bytes)];
    }
  }
}
}  // namespace

extern "C" int bear_kmer_order_u64(const uint64_t *kmer_code, uint64_t n_rows, int lag, uint32_t *perm, void *scratch,
                                   uint64_t *scratch_bytes, void *stream) {
  if (!scratch_bytes || lag < 1 || lag > 21 || n_rows > 0xffffffffull) return BEAR_ERR_INVALID_ARG;
  // caller-owned scratch: two key arrays, the identity values, rocPRIM's temporary storage (each piece 256-byte aligned)
  const uint64_t keys_b = (n_rows * 8 + 255) & ~255ull, vals_b = (n_rows * 4 + 255) & ~255ull;
  size_t tb = 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_rows)
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr,
                                      (uint32_t *)nullptr, n_rows, 0u, (unsigned)(3 * lag), s));
  const uint64_t need = n_rows ? 2 * keys_b + vals_b + (tb ? tb : 8) : 0;
  if (!scratch) {            // size query
    *scratch_bytes = need;
    return BEAR_OK;
  }
  if (n_rows == 0) return BEAR_OK;
  if (!kmer_code || !perm || *scratch_bytes < need || (reinterpret_cast<uintptr_t>(scratch) & 255)) return BEAR_ERR_INVALID_ARG;
  unsigned char *base = static_cast<unsigned char *>(scratch);
  unsigned long long *keys_in = reinterpret_cast<unsigned long long *>(base);
  unsigned long long *keys_out = reinterpret_cast<unsigned long long *>(base + keys_b);
  uint32_t *vals_in = reinterpret_cast<uint32_t *>(base + 2 * keys_b);
  void *temp = base + 2 * keys_b + vals_b;
  hipLaunchKernelGGL(order_keys_kernel, dim3(grid_for(n_rows)), dim3(256), 0, s, reinterpret_cast<const unsigned long long *>(kmer_code),
                     n_rows, lag, keys_in, vals_in);
  HIP_TRY(hipGetLastError());
  // stream-ordered from here on: the scratch is the caller's, nothing is freed and nothing waits on the host
  HIP_TRY(rocprim::radix_sort_pairs(temp, tb, keys_in, keys_out, vals_in, perm, n_rows, 0u, (unsigned)(3 * lag), s));
  return BEAR_OK;
}

extern "C" int bear_gather_rows(const void *src, const uint32_t *perm, void *dst, uint64_t n_rows, uint32_t row_bytes, void *stream) {
  if ((n_rows && (!src || !perm || !dst)) || row_bytes == 0 || src == dst) return BEAR_ERR_INVALID_ARG;
  if (n_rows == 0) return BEAR_OK;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for(n_rows * ((row_bytes & 3u) ? row_bytes : row_bytes >> 2))), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const unsigned char *>(src), perm, static_cast<unsigned char *>(dst),
                     n_rows, row_bytes);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

// ------------------------------------------------------------------ prefix levels of a sorted batch (bear_levels.h, kernels_cnn.h)
namespace {
__global__ __launch_bounds__(256) void level_flag_kernel(const unsigned long long *__restrict__ codes, uint64_t n, unsigned long long mask,
                                                         uint32_t *__restrict__ flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
    flag[i] = (i == 0 || ((codes[i] ^ codes[i - 1]) & mask) != 0ull) ? 1u : 0u;
}
// scan[i] = number of runs that start at or before row i: row i belongs to run scan[i] - 1; a run's first row writes the run's record
__global__ __launch_bounds__(256) void level_compact_kernel(const unsigned long long *__restrict__ codes, uint64_t n, unsigned long long mask,
                                                            unsigned long long fill, const uint32_t *__restrict__ flag,
                                                            uint32_t *__restrict__ scan_to_parent, unsigned long long *__restrict__ out_codes,
                                                            uint32_t *__restrict__ child_start, uint64_t n_runs) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint32_t run = scan_to_parent[i] - 1u;
    if (flag[i]) {
      out_codes[run] = (codes[i] & mask) | fill;
      child_start[run] = (uint32_t)i;
    }
    scan_to_parent[i] = run;
    if (i == 0) child_start[n_runs] = (uint32_t)n;
  }
}
}  // namespace

namespace {
struct rec16 { unsigned long long a, b; };
struct rec16_less {
  __device__ __host__ bool operator()(const rec16 &x, const rec16 &y) const { return x.a < y.a || (x.a == y.a && x.b < y.b); }
};
template <typename T, typename Less>
int canonical_sort(T *d, uint64_t n, Less less, hipStream_t s) {
  dev_buf<T> out;
  dev_buf<unsigned char> temp;
  HIP_TRY(out.alloc(n));
  HIP_TRY(rocprim_run(temp, [&](void *t, size_t &tb) { return rocprim::merge_sort(t, tb, d, out.get(), n, less, s); }));
  HIP_TRY(hipMemcpyAsync(d, out.get(), n * sizeof(T), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  return BEAR_OK;
}
}  // namespace

int bear_canonical_order(void *records, uint64_t n, int width, hipStream_t s) {
  if (n < 2) return BEAR_OK;
  if (!records) return BEAR_ERR_INVALID_ARG;
  if (width == 16) return canonical_sort(static_cast<rec16 *>(records), n, rec16_less(), s);
  if (width == 8) return canonical_sort(static_cast<unsigned long long *>(records), n, rocprim::less<unsigned long long>(), s);
  if (width == 4) return canonical_sort(static_cast<uint32_t *>(records), n, rocprim::less<uint32_t>(), s);
  return BEAR_ERR_INVALID_ARG;
}

// ------------------------------------------------------------------ window tables (bear_levels.h, kernels_cnn.h)
namespace {
__global__ __launch_bounds__(256) void window_keys_kernel(const unsigned long long *__restrict__ codes, uint64_t n, int shift, unsigned long long mask,
                                                          unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    keys[i] = (codes[i] >> shift) & mask;
    vals[i] = (uint32_t)i;
  }
}
// sorted position j belongs to run scan[j] - 1; a run's first position writes the window's record; every position its context's row
__global__ __launch_bounds__(256) void window_compact_kernel(const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ perm, uint64_t n,
                                                             int shift, unsigned long long fill, const uint32_t *__restrict__ flag,
                                                             const uint32_t *__restrict__ scan, unsigned long long *__restrict__ out_codes,
                                                             uint32_t *__restrict__ child_start, uint32_t *__restrict__ row_of_context,
                                                             uint64_t n_runs) {
  for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (uint64_t)gridDim.x * 256) {
    const uint32_t run = scan[j] - 1u;
    if (flag[j]) {
      out_codes[run] = (keys[j] << shift) | fill;
      child_start[run] = (uint32_t)j;
    }
    row_of_context[perm[j]] = run;
    if (j == 0) child_start[n_runs] = (uint32_t)n;
  }
}
}  // namespace

void bear_window_free(bear_window_dev *wt) {
  if (!wt) return;
  (void)hipFree(wt->codes);
  (void)hipFree(wt->row_of_context);
  (void)hipFree(wt->perm);
  (void)hipFree(wt->child_start);
  (void)hipFree(wt->rows);
  wt->codes = nullptr;
  wt->row_of_context = wt->perm = wt->child_start = nullptr;
  wt->rows = nullptr;
  wt->n = 0;
  wt->bytes = 0;
}

int bear_window_build(const unsigned long long *codes, uint64_t n_rows, int pos, int fw, bear_window_dev *out, hipStream_t s) {
  if (!codes || !out || n_rows == 0 || n_rows > 0xfffffffeull || pos < 0 || fw < 1 || pos + fw > 21) return BEAR_ERR_INVALID_ARG;
  const int shift = 3 * pos;
  const unsigned long long mask = (1ull << (3 * fw)) - 1ull;      // (fw <= 21: at most 63 bits)
  unsigned long long fill = 0ull;
  for (int l = 0; l < 21; ++l)
    if (l < pos || l >= pos + fw) fill |= 5ull << (3 * l);
  *out = bear_window_dev{};      // (what a failed build leaves)
  out->pos = pos;
  dev_buf<unsigned long long> keys_in, keys, win_codes;
  dev_buf<uint32_t> vals_in, scan, perm, row_of_context, child_start;
  dev_buf<double> rows;
  dev_buf<unsigned char> temp;
  uint32_t n_runs = 0;
  HIP_TRY(keys_in.alloc(n_rows));
  HIP_TRY(keys.alloc(n_rows));
  HIP_TRY(vals_in.alloc(n_rows));
  HIP_TRY(perm.alloc(n_rows));
  HIP_TRY(row_of_context.alloc(n_rows));
  hipLaunchKernelGGL(window_keys_kernel, dim3(grid_for(n_rows)), dim3(256), 0, s, codes, n_rows, shift, mask, keys_in.get(), vals_in.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(rocprim_run(temp, [&](void *t, size_t &tb) {      // stable: ties keep row order
    return rocprim::radix_sort_pairs(t, tb, keys_in.get(), keys.get(), vals_in.get(), perm.get(), n_rows, 0u, (unsigned)(3 * fw), s);
  }));
  HIP_TRY(hipStreamSynchronize(s));
  temp.reset();            // the sort's storage and its input keys go before `scan` comes: the peak of the build
  keys_in.reset();
  // runs of equal windows (the flag / scan of the prefix levels, on the sorted keys)
  dev_buf<uint32_t> &flag = vals_in;          // (the unsorted row numbers are no longer needed)
  HIP_TRY(scan.alloc(n_rows));
  hipLaunchKernelGGL(level_flag_kernel, dim3(grid_for(n_rows)), dim3(256), 0, s, keys.get(), n_rows, ~0ull, flag.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(rocprim_run(temp, [&](void *t, size_t &tb) {
    return rocprim::inclusive_scan(t, tb, flag.get(), scan.get(), n_rows, rocprim::plus<uint32_t>(), s);
  }));
  HIP_TRY(hipMemcpyAsync(&n_runs, scan.get() + (n_rows - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(win_codes.alloc(n_runs));
  HIP_TRY(child_start.alloc((size_t)n_runs + 1));
  HIP_TRY(rows.alloc((size_t)n_runs * 16));
  hipLaunchKernelGGL(window_compact_kernel, dim3(grid_for(n_rows)), dim3(256), 0, s, keys.get(), perm.get(), n_rows, shift, fill, flag.get(),
                     scan.get(), win_codes.get(), child_start.get(), row_of_context.get(), (uint64_t)n_runs);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  out->n = n_runs;
  out->codes = win_codes.release();
  out->row_of_context = row_of_context.release();
  out->perm = perm.release();
  out->child_start = child_start.release();
  out->rows = rows.release();
  out->bytes = (uint64_t)n_runs * (8 + 4 + 128) + n_rows * 8;
  return BEAR_OK;
}

void bear_level_free(bear_level_dev *lv) {
  if (!lv) return;
  (void)hipFree(lv->codes);
  (void)hipFree(lv->parent_of_below);
  (void)hipFree(lv->child_start);
  (void)hipFree(lv->rows);
  lv->codes = nullptr;
  lv->parent_of_below = nullptr;
  lv->child_start = nullptr;
  lv->rows = nullptr;
  lv->n = 0;
  lv->bytes = 0;
}

int bear_level_build(const unsigned long long *codes_below, uint64_t n_below, int letters, bear_level_dev *out, hipStream_t s) {
  if (!codes_below || !out || n_below == 0 || n_below > 0xfffffffeull || letters < 1 || letters > 21) return BEAR_ERR_INVALID_ARG;
  const unsigned long long mask = (1ull << (3 * letters)) - 1ull;
  unsigned long long fill = 0ull;
  for (int l = letters; l < 22 && 3 * l < 64; ++l) fill |= 5ull << (3 * l);     // (bear_pack_kmers_u64 fills positions >= lag the same way)
  *out = bear_level_dev{};       // (what a failed build leaves)
  out->letters = letters;
  dev_buf<uint32_t> flag, scan, child_start;
  dev_buf<unsigned long long> run_codes;
  dev_buf<double> rows;
  dev_buf<unsigned char> temp;
  uint32_t n_runs = 0;
  HIP_TRY(flag.alloc(n_below));
  HIP_TRY(scan.alloc(n_below));
  hipLaunchKernelGGL(level_flag_kernel, dim3(grid_for(n_below)), dim3(256), 0, s, codes_below, n_below, mask, flag.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(rocprim_run(temp, [&](void *t, size_t &tb) {
    return rocprim::inclusive_scan(t, tb, flag.get(), scan.get(), n_below, rocprim::plus<uint32_t>(), s);
  }));
  HIP_TRY(hipMemcpyAsync(&n_runs, scan.get() + (n_below - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(run_codes.alloc(n_runs));
  HIP_TRY(child_start.alloc((size_t)n_runs + 1));
  HIP_TRY(rows.alloc((size_t)n_runs * 16));
  hipLaunchKernelGGL(level_compact_kernel, dim3(grid_for(n_below)), dim3(256), 0, s, codes_below, n_below, mask, fill, flag.get(), scan.get(),
                     run_codes.get(), child_start.get(), (uint64_t)n_runs);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  out->n = n_runs;
  out->codes = run_codes.release();
  out->parent_of_below = scan.release();      // (the compaction turned the scan into the parents' rows)
  out->child_start = child_start.release();
  out->rows = rows.release();
  return BEAR_OK;
}
