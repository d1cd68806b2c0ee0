// kernels_score.h -- scoring variants and sequences under a sampled table on the device (get_var_probs.get_bear_probs[_seqs] with a
// DeviceCounter): symbols -> look-up keys, keys -> table rows, and the sums of log-probability rows over segments.
//
// The text is the symbol text of bear_count.hip (letters 0 .. W - 2, stop W - 1, start W) with every start and stop written
// out, cut into segments by offsets: a variant window, a padded sequence.  Nothing is read across a segment's start.
//
// Also the home of what the unit bear_score.hip writes once: the look-up (scr_last_le, scr_find_row: segments, table rows, the
// generation step of kernels_generate.h) and the chunk rule of the long segments (scr_chunks_of_block, scr_chunk_slot: the sums
// here and those of kernels_marg.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SCR_THREADS 256
#define SCR_WAVE 64                // threads of a block of score_sum_kernel / score_chunk_kernel: one wave over 64 values
#define SCR_CHUNK BEAR_SCORE_CHUNK // transitions of a long segment that one wave sums (include/bear_hip.h: part of the results)
#define SCR_NO_KEY (~0ull)         // no transition at this position (a valid key has at most 63 bits)
#define SCR_SKIP 0xFFu             // ... and its letter
#define SCR_ABSENT 0xFFFFFFFFu     // bear_kmer_find_u64: the key is not in the table

// rank[c] of the symbol code c <= W as a letter of a context: the position of its character among the alphabet's characters and
// '[' in byte order (first letter most significant, so integer order of the keys is the order of the k-mer strings); 0xFF: no
// letter of a context (the stop, any code beyond W)
struct scr_ranks {
  uint8_t rank[32];
};

// the last index i < n with a[i] <= x, or 0 where there is none, of ascending a[0 .. n), n >= 1.  No data-dependent branch: the
// trip count is set by n alone, so every lane of a wave runs the same number of steps.  THE look-up of this unit: the segment
// that holds a position (a = seg, n = n_seg: empty segments in front of it are stepped over; seg[0] <= x is the caller's) and
// the table row of a key (scr_find_row)
__device__ __forceinline__ uint64_t scr_last_le(const uint64_t *__restrict__ a, uint64_t n, uint64_t x) {
  uint64_t lo = 0;                 // the answer lies in [lo, lo + n)
  while (n > 1) {
    const uint64_t half = n >> 1;
    lo = a[lo + half] <= x ? lo + half : lo;
    n -= half;
  }
  return lo;
}

// the row of `key` in the ascending distinct table keys, or SCR_ABSENT (an empty table holds no key)
__device__ __forceinline__ uint32_t scr_find_row(const uint64_t *__restrict__ table, uint64_t n_table, uint64_t key) {
  if (n_table == 0) return SCR_ABSENT;
  const uint64_t lo = scr_last_le(table, n_table, key);
  return table[lo] == key ? (uint32_t)lo : SCR_ABSENT;
}

// offset x of the segments, kept inside the n transitions (whatever the offsets hold, nothing is read beyond the arrays)
__device__ __forceinline__ uint64_t scr_off(const uint64_t *__restrict__ seg, uint64_t x, uint64_t n) {
  const uint64_t o = seg[x];
  return o < n ? o : n;
}

// one thread per symbol: the key of the `lag` symbols in front of it and its letter, or SCR_NO_KEY / SCR_SKIP where the symbol
// stands less than `lag` symbols into its segment (or outside every segment, or, behind the Python layer's refusal, where a
// symbol is no letter of its place)
template <int BITS>
__global__ __launch_bounds__(SCR_THREADS) void score_transitions_kernel(const uint8_t *__restrict__ text,
                                                                        const uint64_t *__restrict__ seg, uint64_t n_sym,
                                                                        uint64_t n_seg, int lag, uint32_t width, scr_ranks R,
                                                                        uint64_t *__restrict__ keys, uint8_t *__restrict__ letters) {
  for (uint64_t i = (uint64_t)blockIdx.x * SCR_THREADS + threadIdx.x; i < n_sym; i += (uint64_t)gridDim.x * SCR_THREADS) {
    uint64_t key = SCR_NO_KEY;
    uint32_t letter = SCR_SKIP;
    if (n_seg > 0 && seg[0] <= i && i < seg[n_seg]) {
      const uint64_t s = scr_last_le(seg, n_seg, i);
      const uint32_t nx = text[i];
      if (i - seg[s] >= (uint64_t)lag && nx < width) {
        uint64_t k = 0;
        bool bad = false;
        for (int j = lag; j >= 1; --j) {       // the first letter of the context is the most significant
          const uint32_t c = text[i - (uint64_t)j];
          const uint32_t r = R.rank[c < 32u ? c : 31u];
          bad |= c > width || r == 0xFFu;
          k = (k << BITS) | (uint64_t)(r & ((1u << BITS) - 1u));
        }
        if (!bad) {
          key = k;
          letter = nx;
        }
      }
    }
    keys[i] = key;
    letters[i] = (uint8_t)letter;
  }
}

// one thread per query: scr_find_row (sorted queries keep neighbouring lanes on neighbouring entries)
__global__ __launch_bounds__(SCR_THREADS) void kmer_find_kernel(const uint64_t *__restrict__ table, uint64_t n_table,
                                                                const uint64_t *__restrict__ query, uint64_t n_query,
                                                                uint32_t *__restrict__ rows) {
  for (uint64_t q = (uint64_t)blockIdx.x * SCR_THREADS + threadIdx.x; q < n_query; q += (uint64_t)gridDim.x * SCR_THREADS)
    rows[q] = scr_find_row(table, n_table, query[q]);
}

// lp[row, letter, v] of transitions [a, b) added to acc in text order; a transition with the letter SCR_SKIP (or a row or letter
// outside the table) adds nothing.  Four loads are in flight while the adds stay in order.
__device__ __forceinline__ double scr_sum_range(const double *__restrict__ lp, uint64_t n_rows, uint32_t width, uint64_t ms,
                                                const uint32_t *__restrict__ rows, const uint8_t *__restrict__ letters, uint64_t a,
                                                uint64_t b, uint64_t v, double acc) {
  for (uint64_t t = a; t < b; t += 4) {
    double x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j] = 0.0;
      if (t + j < b) {
        const uint32_t r = rows[t + j], l = letters[t + j];
        if (l < width && (uint64_t)r < n_rows) x[j] = lp[((uint64_t)r * width + l) * ms + v];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += x[j];
  }
  return acc;
}

// THE chunk rule of this unit (the sums of kernels_score.h over SCR_CHUNK, those of kernels_marg.h over MRG_CHUNK).  The chunks of
// the long segments (more than C positions) are cut from each segment's own start, so that a segment's sum does not depend on
// where it stands in the text.  Block g looks at text positions [g C, (g + 1) C) and sums the chunks that START there: at most two,
// because chunks of one segment start C apart and a long segment that starts inside the range runs past its end -- slot 2 g: the
// chunk of the segment that holds position g C; slot 2 g + 1: chunk 0 of the last segment that starts behind g C.  sum(slot, a, b)
// is called for each chunk [a, b) there is, by the whole block alike; a slot without a chunk is never read (scr_chunk_slot).
// The segment found for position g C must start at or in front of it (s0 <= p0).  For ascending offsets it always does:
// first <= p0 < n_t gives seg[0] <= p0, and the segment found is then the last with seg[s] <= p0 -- the test only keeps offsets
// that do not ascend from placing a chunk in front of its block.
template <uint64_t C, class F>
__device__ __forceinline__ void scr_chunks_of_block(const uint64_t *__restrict__ seg, uint64_t n_seg, uint64_t n_t, uint64_t g,
                                                    F &&sum) {
  const uint64_t p0 = g * C;
  const uint64_t p1 = p0 + C < n_t ? p0 + C : n_t;
  const uint64_t first = scr_off(seg, 0, n_t), end = scr_off(seg, n_seg, n_t);
  if (p0 >= p1 || first >= p1 || end <= p0 || first >= end) return;
  const uint64_t sb = scr_last_le(seg, n_seg, (end < p1 ? end : p1) - 1);
  if (first <= p0) {
    const uint64_t sa = scr_last_le(seg, n_seg, p0);
    const uint64_t s0 = scr_off(seg, sa, n_t), s1 = scr_off(seg, sa + 1, n_t);
    const uint64_t a = s0 + (p0 - s0 + C - 1) / C * C;      // its first chunk start at or behind p0
    if (s0 <= p0 && s1 > s0 && s1 - s0 > C && a < s1) sum(2 * g, a, a + C < s1 ? a + C : s1);
  }
  const uint64_t s0 = scr_off(seg, sb, n_t), s1 = scr_off(seg, sb + 1, n_t);
  if (s0 > p0 && s1 > s0 && s1 - s0 > C) sum(2 * g + 1, s0, s0 + C);
}

// ... and its inverse: the slot of the chunk that starts at `a` of a long segment that starts at s0
template <uint64_t C>
__device__ __forceinline__ uint64_t scr_chunk_slot(uint64_t s0, uint64_t a) {
  const uint64_t g = a / C;
  return 2 * g + (s0 <= g * C ? 0 : 1);
}

// The chunks of the segments of more than SCR_CHUNK transitions: one wave per block of the text and 64 values.
// partials [2 n_blocks, ms]
__global__ __launch_bounds__(SCR_WAVE) void score_chunk_kernel(const double *__restrict__ lp, uint64_t n_rows, uint32_t width,
                                                              uint64_t ms, const uint32_t *__restrict__ rows,
                                                              const uint8_t *__restrict__ letters, const uint64_t *__restrict__ seg,
                                                              uint64_t n_seg, uint64_t n_t, uint64_t n_blocks,
                                                              double *__restrict__ partials) {
  const uint64_t v = (uint64_t)blockIdx.y * SCR_WAVE + threadIdx.x;
  if (v >= ms) return;
  for (uint64_t g = blockIdx.x; g < n_blocks; g += gridDim.x)
    scr_chunks_of_block<SCR_CHUNK>(seg, n_seg, n_t, g, [&](uint64_t slot, uint64_t a, uint64_t b) {
      partials[slot * ms + v] = scr_sum_range(lp, n_rows, width, ms, rows, letters, a, b, v, 0.0);
    });
}

// scores[i, v] of every segment: one wave per segment and 64 values.  A segment of at most SCR_CHUNK transitions is summed here
// in text order; a longer one is the sum of its chunks' partial rows in chunk order (score_chunk_kernel ran before).
__global__ __launch_bounds__(SCR_WAVE) void score_sum_kernel(const double *__restrict__ lp, uint64_t n_rows, uint32_t width, uint64_t ms,
                                                            const uint32_t *__restrict__ rows, const uint8_t *__restrict__ letters,
                                                            const uint64_t *__restrict__ seg, uint64_t n_seg, uint64_t n_t,
                                                            const double *__restrict__ partials, double *__restrict__ scores) {
  const uint64_t v = (uint64_t)blockIdx.y * SCR_WAVE + threadIdx.x;
  if (v >= ms) return;
  for (uint64_t i = blockIdx.x; i < n_seg; i += gridDim.x) {
    const uint64_t s1 = scr_off(seg, i + 1, n_t);
    const uint64_t s0 = scr_off(seg, i, s1);
    double acc = 0.0;
    if (s1 - s0 <= SCR_CHUNK) {
      acc = scr_sum_range(lp, n_rows, width, ms, rows, letters, s0, s1, v, acc);
    } else {
      for (uint64_t a = s0; a < s1; a += SCR_CHUNK) acc += partials[scr_chunk_slot<SCR_CHUNK>(s0, a) * ms + v];
    }
    scores[i * ms + v] = acc;
  }
}
