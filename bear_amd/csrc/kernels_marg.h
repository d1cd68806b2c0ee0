// kernels_marg.h -- the exact Dirichlet-multinomial marginal of whole segments on the device (get_var_probs.get_bear_probs_seqs
// with get_marg and a DeviceCounter; include/bear_hip.h, bear_score_marg_f64).
//
// The text is that of kernels_score.h, one row number and one letter per position, SORTED inside every segment by (row, letter):
// a run -- a maximal stretch of equal (row, letter) -- is one letter count q_j of a k-mer inside the segment, the stretch of equal
// row (the group) is the k-mer's n.  Per model the segment's score is the sum over its groups of -D(A, n) and over its runs of
// D(a_j, q_j), D(x, c) = lgamma(x + c) - lgamma(x) = bear_dm_item(x, c).D.
//
//   marg_terms_kernel<W>   one thread per position.  The head of a run finds the run's end, the head of a group also the group's,
//                          by binary search inside the segment (lag 1 on a genome has runs of 1e5: nobody walks), and writes
//                          the run's term, plus the group's at a group head, for every model; every other position writes 0.
//                          terms [M, n_t], model-major: a wave's 64 positions are 512 contiguous bytes per model, here and in the sums.
//   marg_chunk_kernel      segments beyond MRG_CHUNK positions, cut from their own start as kernels_score.h cuts them: one wave
//                          sums a chunk of one model.
//   marg_sum_kernel        one wave per segment and model: a short segment is one chunk, a long one its chunks' sums in order.
// A chunk's sum: position p on lane (p - chunk start) mod 64, every lane front to back, the lanes in bear_wave_sum's fixed tree.
// No atomics anywhere, and nothing in a sum depends on where the segment stands: a segment's bits are its content's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bear_math.h"
#include "kernels_score.h"   // scr_last_le, scr_off, the chunk rule: the segments are those of the scoring text

#define MRG_THREADS 256
#define MRG_WAVE 64                      // threads of a block of marg_chunk_kernel / marg_sum_kernel: one wave over 64 positions
#define MRG_CHUNK BEAR_MARG_CHUNK        // positions of a long segment that one wave sums (include/bear_hip.h: part of the results)
#define MRG_MAX_MODELS BEAR_MARG_MAX_MODELS
#define MRG_NO_KEY (~0ull)               // a position without a transition

struct mrg_models {
  int n_h, n_m;                          // BEAR models first, n_m in all
  double w[MRG_MAX_MODELS];              // [0, n_h): 1 / h;  [n_h, n_m): van
};

// (row << 8) | letter of position p, or MRG_NO_KEY where it holds no transition of the table (a negative row, a row or letter
// beyond the table): the only place rows and letters are read, so nothing they hold becomes an index unchecked
__device__ __forceinline__ uint64_t mrg_key(const int32_t *__restrict__ rows, const uint8_t *__restrict__ letters, uint64_t p,
                                            uint32_t width, uint64_t n_rows) {
  const int32_t r = rows[p];
  const uint32_t l = letters[p];
  return (r >= 0 && (uint64_t)r < n_rows && l < width) ? ((uint64_t)(uint32_t)r << 8) | l : MRG_NO_KEY;
}

// the end of the stretch of positions [i, end) inside [i, s1) whose keys, shifted right by `shift`, equal `want` (position i's does):
// the loop of scr_last_le on a computed key -- its trip count is set by s1 - i alone, no branch on what is read.  n = 1: no search.
__device__ __forceinline__ uint64_t mrg_stretch_end(const int32_t *__restrict__ rows, const uint8_t *__restrict__ letters,
                                                    uint64_t i, uint64_t n, uint64_t want, int shift, uint32_t width,
                                                    uint64_t n_rows) {
  uint64_t lo = i;                       // the last position of the stretch lies in [lo, lo + n)
  while (n > 1) {
    const uint64_t half = n >> 1;
    lo = (mrg_key(rows, letters, lo + half, width, n_rows) >> shift) == want ? lo + half : lo;
    n -= half;
  }
  return lo + 1;
}

// What position i of the sorted text is, for the three terms kernels (marg, moments, groups): the position walk, written once.
struct mrg_pos {
  bool run_head, group_head;             // the first position of its run (equal key), of its group (equal row); neither: no term
  uint64_t key, left, seg;               // left: positions from i to the end of its segment `seg` (1 where i is no head)
  uint64_t row;                          // of a run head, else 0: nothing that is no head's becomes an index
  uint32_t letter;
  uint64_t run_end, group_end;           // in (i, i + left], inside the segment and so inside the text; i + 1 where i is no head
};

// first / end: the text's seg[0] and seg[n_seg], hoisted out of the grid-stride loop.  Integer work only.
template <int W>
__device__ __forceinline__ mrg_pos mrg_classify(uint64_t i, const int32_t *__restrict__ rows, const uint8_t *__restrict__ letters,
                                                uint64_t n_t, const uint64_t *__restrict__ seg, uint64_t n_seg, uint64_t first,
                                                uint64_t end, uint64_t n_rows) {
  mrg_pos p;
  p.run_head = p.group_head = false;
  p.key = MRG_NO_KEY;
  p.left = 1;
  p.seg = 0;
  if (first <= i && i < end) {
    p.seg = scr_last_le(seg, n_seg, i);
    const uint64_t s0 = scr_off(seg, p.seg, n_t), s1 = scr_off(seg, p.seg + 1, n_t);
    if (s0 <= i && i < s1) {
      p.key = mrg_key(rows, letters, i, W, n_rows);
      if (p.key != MRG_NO_KEY) {
        const uint64_t prev = i > s0 ? mrg_key(rows, letters, i - 1, W, n_rows) : MRG_NO_KEY;
        p.group_head = (prev >> 8) != (p.key >> 8);
        p.run_head = prev != p.key;
        p.left = s1 - i;
      }
    }
  }
  p.row = p.run_head ? p.key >> 8 : 0;
  p.letter = p.run_head ? (uint32_t)(p.key & 0xFFu) : 0u;
  p.run_end = mrg_stretch_end(rows, letters, i, p.run_head ? p.left : 1, p.key, 0, W, n_rows);
  p.group_end = mrg_stretch_end(rows, letters, i, p.group_head ? p.left : 1, p.key >> 8, 8, W, n_rows);
  return p;
}

// kept out of line: two call sites inside the model loop, ~500 instructions each
__device__ __noinline__ double mrg_item_D(double x, double c) { return bear_dm_item(x, c).D; }

template <int W>
__global__ __launch_bounds__(MRG_THREADS) void marg_terms_kernel(const int32_t *__restrict__ rows, const uint8_t *__restrict__ letters,
                                                                 uint64_t n_t, const uint64_t *__restrict__ seg, uint64_t n_seg,
                                                                 const uint32_t *__restrict__ train, const double *__restrict__ prior,
                                                                 uint64_t n_rows, mrg_models P, double *__restrict__ terms) {
  const uint64_t first = scr_off(seg, 0, n_t), end = scr_off(seg, n_seg, n_t);
  for (uint64_t i = (uint64_t)blockIdx.x * MRG_THREADS + threadIdx.x; i < n_t; i += (uint64_t)gridDim.x * MRG_THREADS) {
    const mrg_pos p = mrg_classify<W>(i, rows, letters, n_t, seg, n_seg, first, end, n_rows);
    const double q = (double)(p.run_end - i), n = (double)(p.group_end - i);
    uint32_t c[W];                                       // the two rows of a group head, read once for every model's A
    double f[W];
    double cl = 0.0, fl = 0.0;                           // ... and the run's own cell
    if (p.group_head) {
#pragma unroll
      for (int j = 0; j < W; ++j) {
        c[j] = train[p.row * W + j];
        f[j] = prior ? prior[p.row * W + j] : 0.0;
      }
    }
    if (p.run_head) {
      cl = (double)train[p.row * W + p.letter];
      fl = prior ? prior[p.row * W + p.letter] : 0.0;
    }
    for (int m = 0; m < P.n_m; ++m) {
      const double w = P.w[m];
      const bool bear = m < P.n_h;
      double t = 0.0;
      if (p.group_head) {
        double A = 0.0;
#pragma unroll
        for (int j = 0; j < W; ++j) A += bear ? __builtin_fma(f[j], w, (double)c[j]) : (double)c[j] + w;
        t = -mrg_item_D(A, n);
      }
      if (p.run_head) t += mrg_item_D(bear ? __builtin_fma(fl, w, cl) : cl + w, q);
      terms[(uint64_t)m * n_t + i] = t;
    }
  }
}

// The sum of t[a .. b), in every lane: position p on lane (p - a) mod 64, a lane's positions front to back (four loads in flight
// while the adds stay in order), then the 64 lanes.  The whole wave takes every step (bear_wave_sum needs all of it).
__device__ __forceinline__ double mrg_sum_range(const double *__restrict__ t, uint64_t a, uint64_t b) {
  double acc = 0.0;
  for (uint64_t p0 = a; p0 < b; p0 += 4 * MRG_WAVE) {
    double x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint64_t p = p0 + (uint64_t)j * MRG_WAVE + threadIdx.x;
      x[j] = p < b ? t[p] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += x[j];
  }
  return bear_wave_sum(acc);
}

// The chunks of the segments of more than MRG_CHUNK positions (scr_chunks_of_block, the rule of kernels_score.h): one wave per
// block of the text and model.  partials [2 n_blocks, M].  blockIdx.y: the model.
__global__ __launch_bounds__(MRG_WAVE) void marg_chunk_kernel(const double *__restrict__ terms, uint32_t n_m,
                                                             const uint64_t *__restrict__ seg, uint64_t n_seg, uint64_t n_t,
                                                             uint64_t n_blocks, double *__restrict__ partials) {
  const uint32_t m = blockIdx.y;
  const double *__restrict__ t = terms + (uint64_t)m * n_t;
  for (uint64_t g = blockIdx.x; g < n_blocks; g += gridDim.x)
    scr_chunks_of_block<MRG_CHUNK>(seg, n_seg, n_t, g, [&](uint64_t slot, uint64_t a, uint64_t b) {
      const double v = mrg_sum_range(t, a, b);
      if (threadIdx.x == 0) partials[slot * n_m + m] = v;
    });
}

// scores[i, m]: one wave per segment and model.  At most MRG_CHUNK positions: the one chunk, summed here; more: the chunks'
// sums (marg_chunk_kernel ran before) added in chunk order, eight loads in flight.
__global__ __launch_bounds__(MRG_WAVE) void marg_sum_kernel(const double *__restrict__ terms, uint32_t n_m,
                                                           const uint64_t *__restrict__ seg, uint64_t n_seg, uint64_t n_t,
                                                           const double *__restrict__ partials, double *__restrict__ scores) {
  const uint32_t m = blockIdx.y;
  const double *__restrict__ t = terms + (uint64_t)m * n_t;
  for (uint64_t i = blockIdx.x; i < n_seg; i += gridDim.x) {
    const uint64_t s1 = scr_off(seg, i + 1, n_t);
    const uint64_t s0 = scr_off(seg, i, s1);
    double acc = 0.0;
    if (s1 - s0 <= MRG_CHUNK) {
      acc = mrg_sum_range(t, s0, s1);
    } else {
      for (uint64_t a = s0; a < s1; a += 8 * (uint64_t)MRG_CHUNK) {
        double x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint64_t aj = a + (uint64_t)j * MRG_CHUNK;
          x[j] = aj < s1 ? partials[scr_chunk_slot<MRG_CHUNK>(s0, aj) * n_m + m] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += x[j];
      }
    }
    if (threadIdx.x == 0) scores[i * n_m + m] = acc;
  }
}
