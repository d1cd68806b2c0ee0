// kernels_refscore.h -- bear_ref models downstream of training: the prior row of a QUERIED k-mer under a reference-mixed model
// (get_var_probs.get_bear_probs[_seqs] and assemble.generate_sequences with ref_model= / ref_counter=).  Such a row is a function
// of the k-mer's reference count row as well as of the k-mer: with A = W - 1 letters, the stop last, ref the uint32 row of the
// reference column (zeros where the reference table lacks the k-mer) and g the net function's row,
//   r_b = ref_b + eps (b < A), r_A = 0;   R = sum_b r_b (rfw_ref_total);   dev_b = r_b / R - 1/A (rfw_dev), dev_A = 0
//   jc_b = fma(E, dev_b, [b < A] / A);   f_b = fma(nw, g_b, jc_b) V (rfw_mix_cell's .f);   prior_b = f_b + eps
// E = exp(-tau), V = 1 / (nw + 1): host values, passed by value.  The cell routines are the training kernels' own
// (rows_wide_common.h), so a row here is bit for bit the f the DM step of kernels_refmix_wide.h forms for the same constants; the
// + eps is load_bear's wrapper of an AR function (ar_func(.) + epsilon), not training's f / h + c + eps.
//
//   ref_prior_rows_kernel<W>   one thread per query key: scr_find_row in the reference column's ascending keys, the count row in
//                              key order, the W cells.  Small and not hot: no atomics, no LDS, no scratch.
// The generation step (kernels_generate.h, gen_run with its reference arguments) forms the same cells, one per letter lane.
#pragma once
#include "kernels_score.h"      // scr_find_row, SCR_THREADS, SCR_ABSENT
#include "rows_wide_common.h"   // rfw_ref_total, rfw_mix_cell

// the reference row of a k-mer the reference table lacks: a row of zeros in memory, so that an absent row is a pointer like any
// other (a per-lane array of zeros indexed by the letter would live in scratch)
static __device__ const uint32_t rfs_zero_row[32] = {0};

template <int W>
__device__ __forceinline__ const uint32_t *rfs_ref_row(const uint32_t *__restrict__ ref_counts, uint32_t row) {
  static_assert(W <= 32, "rfs_zero_row holds 32 entries");
  return row != SCR_ABSENT ? ref_counts + (uint64_t)row * W : rfs_zero_row;
}

// prior_b of the row rf (R its rfw_ref_total, invR = 1 / R) with the net entry g
template <int W>
__device__ __forceinline__ double rfs_prior_cell(const uint32_t *rf, int b, double g, double R, double invR, const bear_params &prm) {
  return rfw_mix_cell<W>(rf, b, g, R, invR, prm).f + prm.eps;
}

// prior [n_query, W]; net_rows: NULL (the stop net function: g = one-hot at the stop) or [n_query, W]
template <int W>
__global__ __launch_bounds__(SCR_THREADS) void ref_prior_rows_kernel(const uint64_t *__restrict__ ref_table,
                                                                     const uint32_t *__restrict__ ref_counts, uint64_t n_ref,
                                                                     const uint64_t *__restrict__ query, uint64_t n_query,
                                                                     const double *__restrict__ net_rows, bear_params prm,
                                                                     double *__restrict__ prior) {
  for (uint64_t q = (uint64_t)blockIdx.x * SCR_THREADS + threadIdx.x; q < n_query; q += (uint64_t)gridDim.x * SCR_THREADS) {
    const uint32_t *rf = rfs_ref_row<W>(ref_counts, scr_find_row(ref_table, n_ref, query[q]));
    const double R = rfw_ref_total<W>(rf, prm.eps), invR = 1.0 / R;
#pragma unroll
    for (int b = 0; b < W; ++b) {
      const double g = net_rows ? net_rows[q * W + b] : (b == W - 1 ? 1.0 : 0.0);
      prior[q * W + b] = rfs_prior_cell<W>(rf, b, g, R, invR, prm);
    }
  }
}
