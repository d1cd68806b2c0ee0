// kernels_score.h -- scoring variants and sequences under a sampled table on the device (get_var_probs.get_bear_probs[_seqs] with a
// DeviceCounter): symbols -> look-up keys, keys -> table rows, and the sums of log-probability rows over segments.
//
// The text is the symbol text of bear_count.hip (letters 0 .. W - 2, stop W - 1, start W) with every start and stop written
// out, cut into segments by offsets: a variant window, a padded sequence.  Nothing is read across a segment's start.
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

// the segment that holds position i: the last s < n_seg with seg[s] <= i (empty segments in front of it are stepped over);
// seg[0] <= i is the caller's
__device__ __forceinline__ uint64_t scr_segment_of(const uint64_t *__restrict__ seg, uint64_t n_seg, uint64_t i) {
  uint64_t lo = 0, n = n_seg;      // the answer lies in [lo, lo + n)
  while (n > 1) {
    const uint64_t half = n >> 1;
    lo = seg[lo + half] <= i ? lo + half : lo;
    n -= half;
  }
  return lo;
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
      const uint64_t s = scr_segment_of(seg, n_seg, i);
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

// one thread per query: lower bound in the sorted distinct table keys without a data-dependent branch (every lane of a wave runs
// the same number of steps; sorted queries keep neighbouring lanes on neighbouring entries)
__global__ __launch_bounds__(SCR_THREADS) void kmer_find_kernel(const uint64_t *__restrict__ table, uint64_t n_table,
                                                                const uint64_t *__restrict__ query, uint64_t n_query,
                                                                uint32_t *__restrict__ rows) {
  for (uint64_t q = (uint64_t)blockIdx.x * SCR_THREADS + threadIdx.x; q < n_query; q += (uint64_t)gridDim.x * SCR_THREADS) {
    uint32_t row = SCR_ABSENT;
    if (n_table > 0) {
      const uint64_t key = query[q];
      uint64_t lo = 0, n = n_table;
      while (n > 1) {
        const uint64_t half = n >> 1;
        lo = table[lo + half] <= key ? lo + half : lo;      // the last entry <= key, or entry 0
        n -= half;
      }
      row = table[lo] == key ? (uint32_t)lo : SCR_ABSENT;
    }
    rows[q] = row;
  }
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

// The chunks of the long segments (more than SCR_CHUNK transitions), cut from each segment's own start so that a segment's sum
// does not depend on where it stands in the text.  Block g looks at text positions [g C, (g + 1) C) and sums the chunks that START
// there: at most two, because chunks of one segment start C apart and a long segment that starts inside the range runs past its
// end -- slot 2 g: the chunk of the segment that holds position g C; slot 2 g + 1: chunk 0 of the last segment that starts behind
// g C.  score_sum_kernel finds a chunk's slot by the same rule.  partials [2 n_blocks, ms]; a slot without a chunk is never read.
__global__ __launch_bounds__(SCR_WAVE) void score_chunk_kernel(const double *__restrict__ lp, uint64_t n_rows, uint32_t width,
                                                              uint64_t ms, const uint32_t *__restrict__ rows,
                                                              const uint8_t *__restrict__ letters, const uint64_t *__restrict__ seg,
                                                              uint64_t n_seg, uint64_t n_t, uint64_t n_blocks,
                                                              double *__restrict__ partials) {
  const uint64_t v = (uint64_t)blockIdx.y * SCR_WAVE + threadIdx.x;
  if (v >= ms) return;
  for (uint64_t g = blockIdx.x; g < n_blocks; g += gridDim.x) {
    const uint64_t p0 = g * SCR_CHUNK;
    const uint64_t p1 = p0 + SCR_CHUNK < n_t ? p0 + SCR_CHUNK : n_t;
    const uint64_t first = scr_off(seg, 0, n_t), end = scr_off(seg, n_seg, n_t);
    if (p0 >= p1 || first >= p1 || end <= p0 || first >= end) continue;
    const uint64_t sb = scr_segment_of(seg, n_seg, (end < p1 ? end : p1) - 1);
    if (first <= p0) {
      const uint64_t sa = scr_segment_of(seg, n_seg, p0);
      const uint64_t s0 = scr_off(seg, sa, n_t), s1 = scr_off(seg, sa + 1, n_t);
      const uint64_t a = s0 + (p0 - s0 + SCR_CHUNK - 1) / SCR_CHUNK * SCR_CHUNK;      // its first chunk start at or behind p0
      if (s1 > s0 && s1 - s0 > SCR_CHUNK && a < s1)
        partials[2 * g * ms + v] = scr_sum_range(lp, n_rows, width, ms, rows, letters, a, a + SCR_CHUNK < s1 ? a + SCR_CHUNK : s1, v, 0.0);
    }
    const uint64_t s0 = scr_off(seg, sb, n_t), s1 = scr_off(seg, sb + 1, n_t);
    if (s0 > p0 && s1 > s0 && s1 - s0 > SCR_CHUNK)
      partials[(2 * g + 1) * ms + v] = scr_sum_range(lp, n_rows, width, ms, rows, letters, s0, s0 + SCR_CHUNK, v, 0.0);
  }
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
      for (uint64_t a = s0; a < s1; a += SCR_CHUNK) {
        const uint64_t g = a / SCR_CHUNK;
        acc += partials[(2 * g + (s0 <= g * SCR_CHUNK ? 0 : 1)) * ms + v];
      }
    }
    scores[i * ms + v] = acc;
  }
}
