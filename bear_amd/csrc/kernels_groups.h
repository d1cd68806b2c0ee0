// kernels_groups.h -- the exact Dirichlet-multinomial marginal of whole segments under EVERY group (column) of a count table at
// once, with an optional leave-one-out group per segment (bear_amd.classify; include/bear_hip.h, bear_score_groups_f64).
//
// The text, the runs and the groups of positions are those of kernels_marg.h: what a position is the head of, its run count q_j,
// its k-mer's n and the prior row do not depend on the table's column, so they are found once per position; only the count row
// differs between the table's groups.  (A "group" of POSITIONS -- the stretch of equal row -- is kernels_marg.h's word; a "group" of
// the TABLE is one of its n_groups columns.  Below: k-mer head / k-mer end for the former, group for the latter.)
//
//   groups_terms_kernel<W>  one thread per position: what it heads, its segment, the run's end and the k-mer's end from
//                           mrg_classify (kernels_marg.h), the prior row once, then a loop over the table's groups that reads that
//                           group's count row (k-mer head) and run cell, and inside it marg_terms_kernel's model loop (written out
//                           in each kernel: DESIGN.md, "Exact marginals and Bayes factors: each copied part once").
//                           train [n_rows, n_groups, W]: the rows of one k-mer are adjacent, a k-mer head reads one stretch.
//                           terms [n_groups * n_m, n_t], plane g * n_m + m: marg_chunk_kernel and marg_sum_kernel sum them as they
//                           stand, with n_groups * n_m models.
//   leave-one-out           own[s] = the group whose counts hold segment s itself.  In that group c_j - q_j stands for c_j, an
//                           exact integer subtraction, in the run's cell and in every a_j of A.  A k-mer head needs q_j of every
//                           letter of its k-mer for that: it walks the k-mer's runs (ascending letters, at most W successive
//                           mrg_stretch_end calls) once, before the group loop, and keeps the decremented own row.  c_j < q_j: the
//                           table does not hold the segment -- short_of[s] = 1 (every thread that sees it stores the same byte)
//                           and the position's own-group terms are NaN, so the segment's own-group scores are.
// No atomics: a segment's bits depend on its own content, its own[] value and the table only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_marg.h"

#define GRP_MAX BEAR_GROUPS_MAX

template <int W>
__global__ __launch_bounds__(MRG_THREADS) void groups_terms_kernel(const int32_t *__restrict__ rows, const uint8_t *__restrict__ letters,
                                                                   uint64_t n_t, const uint64_t *__restrict__ seg, uint64_t n_seg,
                                                                   const uint32_t *__restrict__ train, uint32_t n_groups,
                                                                   const double *__restrict__ prior, uint64_t n_rows,
                                                                   const int32_t *__restrict__ own, mrg_models P,
                                                                   double *__restrict__ terms, uint8_t *__restrict__ short_of) {
  const uint64_t first = scr_off(seg, 0, n_t), end = scr_off(seg, n_seg, n_t);
  for (uint64_t i = (uint64_t)blockIdx.x * MRG_THREADS + threadIdx.x; i < n_t; i += (uint64_t)gridDim.x * MRG_THREADS) {
    const mrg_pos p = mrg_classify<W>(i, rows, letters, n_t, seg, n_seg, first, end, n_rows);
    const bool run_head = p.run_head, kmer_head = p.group_head;        // (this file's words, above)
    const uint64_t s = p.seg, key = p.key, row = p.row, qu = p.run_end - i;
    const uint32_t letter = p.letter;
    const double q = (double)qu, n = (double)(p.group_end - i);
    int32_t mine = -1;                                   // the segment's own group: only a head asks
    if (run_head && own) {
      mine = own[s];
      mine = mine < (int32_t)n_groups ? mine : -1;
    }
    const uint32_t *__restrict__ tr = train + row * n_groups * W;      // the k-mer's n_groups rows
    double f[W];                                         // the prior row of a k-mer head, read once for every group and model
    double fl = 0.0;                                     // ... and the run's own cell
    uint32_t less[W];                                    // the own group's row without the segment's own counts
    bool short_kmer = false;
#pragma unroll
    for (int j = 0; j < W; ++j) less[j] = 0u;
    if (kmer_head) {
#pragma unroll
      for (int j = 0; j < W; ++j) f[j] = prior ? prior[row * W + j] : 0.0;
      if (mine >= 0) {                                   // q_j of every letter: the k-mer's runs stand in ascending letters
        const uint32_t *__restrict__ mr = tr + (uint32_t)mine * W;
        const uint64_t kmer_end = p.group_end;
        uint64_t p = i;
#pragma unroll
        for (int j = 0; j < W; ++j) {
          const uint64_t kp = p < kmer_end ? mrg_key(rows, letters, p, W, n_rows) : MRG_NO_KEY;
          const bool here = kp == ((key & ~0xFFull) | (uint64_t)j);
          const uint64_t qj = here ? mrg_stretch_end(rows, letters, p, kmer_end - p, kp, 0, W, n_rows) - p : 0;
          const uint32_t cj = mr[j];
          short_kmer = short_kmer || qj > (uint64_t)cj;
          less[j] = cj - (uint32_t)qj;
          p += qj;
        }
      }
    }
    if (run_head) fl = prior ? prior[row * W + letter] : 0.0;
    const uint32_t own_cell = run_head && mine >= 0 ? tr[(uint32_t)mine * W + letter] : 0u;
    const bool short_run = run_head && mine >= 0 && qu > (uint64_t)own_cell;
    if (short_kmer || short_run) short_of[s] = 1;
    for (uint32_t g = 0; g < n_groups; ++g) {
      const bool is_mine = (int32_t)g == mine;
      const uint32_t *__restrict__ cr = tr + g * W;
      uint32_t c[W];
      double cl = 0.0;
      if (kmer_head) {
#pragma unroll
        for (int j = 0; j < W; ++j) c[j] = is_mine ? less[j] : cr[j];
      }
      if (run_head) cl = (double)(is_mine ? own_cell - (uint32_t)qu : cr[letter]);
      const bool lost = is_mine && (short_kmer || short_run);
      for (int m = 0; m < P.n_m; ++m) {
        const double w = P.w[m];
        const bool bear = m < P.n_h;
        double t = 0.0;
        if (kmer_head) {
          double A = 0.0;
#pragma unroll
          for (int j = 0; j < W; ++j) A += bear ? __builtin_fma(f[j], w, (double)c[j]) : (double)c[j] + w;
          t = -mrg_item_D(A, n);
        }
        if (run_head) t += mrg_item_D(bear ? __builtin_fma(fl, w, cl) : cl + w, q);
        terms[((uint64_t)g * P.n_m + m) * n_t + i] = lost ? __builtin_nan("") : t;
      }
    }
  }
}
