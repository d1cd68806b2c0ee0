// kernels_moments.h -- the exact posterior mean and variance of a segment's score on the device (get_var_probs.get_bear_probs /
// get_bear_probs_seqs with moments=True; include/bear_hip.h, bear_score_moments_f64): what the mc_samples axis of the sampled path
// samples, in closed form.
//
// The text is that of kernels_marg.h, SORTED inside every segment by (row, letter), every position with a weight of +1 or -1 (a
// mutant window's transitions count +1, the wild type's -1; no weights: all +1).  A run -- equal (row, letter) -- is one cell of a
// k-mer with the signed multiplicity m = the sum of its weights, the group -- equal row -- the k-mer with M = the sum of its m.
// With p ~ Dirichlet(a), A = sum_j a_j, the k-mer's contribution S = sum_b m_b log p_b has
//     E[S] = sum_b m_b psi(a_b) - M psi(A),      Var[S] = sum_b m_b^2 psi1(a_b) - M^2 psi1(A)
// and the k-mers of a segment are independent: a segment's moments are the sums of these terms.
//
//   moments_terms_kernel<W>  one thread per position, which mrg_classify (kernels_marg.h) tells what it heads; a run head writes
//                            m psi(a) and m^2 psi1(a) of its cell, a group head also -M psi(A) and -M^2 psi1(A), every other position
//                            0.  The ends of run and group are mrg_classify's, the signed counts come from an inclusive prefix sum of
//                            the sorted weights (two loads; without weights the stretch's length): nobody walks a run.  a and A are
//                            formed as marg_terms_kernel forms them, bit for bit.  m = 0 / M = 0: exact zeros, psi is not evaluated
//                            (the first transition of a substitution: its psi(A) terms cancel exactly, not numerically).
//                            terms [2 M, n_t]: plane 2 * model + 0 the means, 2 * model + 1 the variances.
// The sums are marg_chunk_kernel and marg_sum_kernel, unchanged, over 2 M planes: no atomics, and a segment's bits are its content's.
#pragma once
#include "kernels_marg.h"

// kept out of line, as mrg_item_D: two call sites each inside the model loop
__device__ __noinline__ double mom_psi(double x) { return bear_psi(x); }
__device__ __noinline__ double mom_psi1(double x) { return bear_psi1(x); }

// the signed count of the positions [i, e): wpre[k] = the sum of the weights of the positions in front of k
__device__ __forceinline__ double mom_count(const int64_t *__restrict__ wpre, uint64_t i, uint64_t e) {
  return wpre ? (double)(wpre[e] - wpre[i]) : (double)(e - i);
}

template <int W>
__global__ __launch_bounds__(MRG_THREADS) void moments_terms_kernel(const int32_t *__restrict__ rows, const uint8_t *__restrict__ letters,
                                                                    const int64_t *__restrict__ wpre, uint64_t n_t,
                                                                    const uint64_t *__restrict__ seg, uint64_t n_seg,
                                                                    const uint32_t *__restrict__ train, const double *__restrict__ prior,
                                                                    uint64_t n_rows, mrg_models P, double *__restrict__ terms) {
  const uint64_t first = scr_off(seg, 0, n_t), end = scr_off(seg, n_seg, n_t);
  for (uint64_t i = (uint64_t)blockIdx.x * MRG_THREADS + threadIdx.x; i < n_t; i += (uint64_t)gridDim.x * MRG_THREADS) {
    const mrg_pos p = mrg_classify<W>(i, rows, letters, n_t, seg, n_seg, first, end, n_rows);
    // the ends lie inside the text: wpre [n_t + 1] is read at no other index
    const double q = p.run_head ? mom_count(wpre, i, p.run_end) : 0.0;         // m of the run, M of the group
    const double n = p.group_head ? mom_count(wpre, i, p.group_end) : 0.0;
    const bool cell = p.run_head && q != 0.0, kmer = p.group_head && n != 0.0;
    uint32_t c[W];                                       // the two rows of a group head, read once for every model's A
    double f[W];
    double cl = 0.0, fl = 0.0;                           // ... and the run's own cell
    if (kmer) {
#pragma unroll
      for (int j = 0; j < W; ++j) {
        c[j] = train[p.row * W + j];
        f[j] = prior ? prior[p.row * W + j] : 0.0;
      }
    }
    if (cell) {
      cl = (double)train[p.row * W + p.letter];
      fl = prior ? prior[p.row * W + p.letter] : 0.0;
    }
    for (int m = 0; m < P.n_m; ++m) {
      const double w = P.w[m];
      const bool bear = m < P.n_h;
      double mean = 0.0, var = 0.0;
      if (kmer) {
        double A = 0.0;
#pragma unroll
        for (int j = 0; j < W; ++j) A += bear ? __builtin_fma(f[j], w, (double)c[j]) : (double)c[j] + w;
        mean = -(n * mom_psi(A));
        var = -((n * n) * mom_psi1(A));
      }
      if (cell) {
        const double a = bear ? __builtin_fma(fl, w, cl) : cl + w;
        mean += q * mom_psi(a);
        var += (q * q) * mom_psi1(a);
      }
      terms[(uint64_t)(2 * m) * n_t + i] = mean;
      terms[(uint64_t)(2 * m + 1) * n_t + i] = var;
    }
  }
}
