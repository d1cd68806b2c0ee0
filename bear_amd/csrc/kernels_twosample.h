// kernels_twosample.h -- bear_two_sample_f64: the two-sample and goodness-of-fit Bayes factors of two count columns `a`, `b` of one
// table, in one pass over its rows.  Per context k and model (concentrations alpha_j: prior[k, j] / h of a BEAR model, van of a
// vanilla one; A = alpha_0 + ... + alpha_(W-1) in that order) the log marginal of the transitions as SEQUENCES
//   T(c) = lgamma(A) - lgamma(A + n) + sum_j [lgamma(alpha_j + c_j) - lgamma(alpha_j)],  n = sum_j c_j   (no multinomial coefficient),
// summed over the rows into M_a = sum T(a_k), M_b = sum T(b_k), M_ab = sum T(a_k + b_k) and B = sum B_k with
// B_k = (T(a_k) + T(b_k)) - T(a_k + b_k) formed PER ROW; and, with prior rows, the AR model's L_a = sum a_j log prior[k, j], L_b.
//
// dm_wide_kernel's structure (kernels_wide.h):
//   tile   = TS_TILE(W) contexts: the two count rows (2 x 4 W B) and the prior row (8 W B) as flat streams of 16-byte lane loads into
//            LDS (stage_dwords), one context per thread; strides of W dwords / W doubles, W odd: conflict-free (kernels_wide.h).
//            W = 21: 128 contexts = 2 x 10.5 KiB + 21 KiB, W = 5: 512 contexts = 2 x 10 KiB + 20 KiB; with the log table (2 KiB) and
//            the reduction rows 44.6 / 42.6 KiB a block: THREE blocks per CU of the 160 KiB (TS_BLOCKS_PER_CU), twelve waves a CU,
//            three a SIMD -- which allows 168 VGPRs: the launch bound holds the kernel to them (184 / 169 without it at W = 21 / 5,
//            two waves a SIMD; 168 and no scratch with it: DESIGN.md 4.13).
//   sparse = a lane walks the bit mask of the cells where a_j | b_j is non-zero.  A row with n_a = 0 or n_b = 0 has B_k = 0.0 exactly
//            and T(a + b) IS the T of its non-empty side: the one chain of items is evaluated once (no item for B_k, the same bits in
//            both sums); a row with n_a = n_b = 0 costs its bytes only.  Where only one of a_j, b_j is non-zero the pooled cell's
//            item is that side's, not evaluated again.
//   items  = evs_item_D (kernels_eval.h): bear_dm_item_fast on the staged log table, out of line, its P half dead code.  Pooled
//            counts and totals travel as exact integers in doubles (a cell below 2^33, a row total below 2^38).
//   models = at most TS_CHUNK per launch in register accumulators (four sums each), more models are further launches (as
//            EVS_CHUNK); the first launch also carries L_a, L_b.
//   sums   = per-thread fp64 -> wave -> block partial (TS_NOUT values) -> two_sample_finalize_kernel's fixed-order sum over the
//            blocks: no atomics, equal bits for equal inputs and grid, in both libraries.
//   rows   = row_terms[k, m] = B_k (optional): one 8-byte vector store per context and model.
#pragma once
#include "bear_common.h"
#include "kernels_eval.h"       // evs_item_D
#include "kernels_rows.h"       // stage_dwords
#include "rows_wide_common.h"   // wide_nz_mask

#define TS_THREADS 256
#define TS_WAVES (TS_THREADS / 64)
#define TS_TILE(W) ((W) > 8 ? 128 : 512)
#define TS_BLOCKS_PER_CU 3
#define TS_CHUNK 4
#define TS_NOUT (4 * TS_CHUNK + 2)     // compact partial: {M_a, M_b, M_ab, B}[chunk], L_a, L_b

struct ts_args {
  double w[BEAR_TWO_SAMPLE_MAX_MODELS];   // [0, n_h): 1 / h_m; [n_h, n_models): van
  int n_h, n_models;
};

// log of a prior entry as the AR mode of wide_dm_row takes it (the table log is exact to ~1e-16 absolute: near 1 the polynomial)
__device__ __forceinline__ double ts_log_prior(double p, const double2 *s_log) {
  return fabs(p - 1.0) < 0x1p-8 ? bear_log1p_small(p - 1.0) : (p > 0.0 ? bear_log_tab(p, s_log) : bear_log(p));
}

// use_prior: the launch reads prior rows (a BEAR model among [m0, m0 + m_cnt), or do_ar); do_ar: it also sums L_a, L_b.
// (The second launch bound is waves per SIMD: a block is four waves, one a SIMD, so it is the blocks per CU.)
template <int W>
__global__ __launch_bounds__(TS_THREADS, TS_BLOCKS_PER_CU) void two_sample_kernel(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                               const double *__restrict__ prior, uint64_t n_rows, ts_args A, int m0,
                                                               int m_cnt, int use_prior, int do_ar,
                                                               const double2 *__restrict__ logtab_g, double *__restrict__ partials,
                                                               double *__restrict__ row_terms) {
  static_assert(W <= 32, "the non-zero cells of a row are a 32-bit mask");
  constexpr int T = TS_TILE(W);
  __shared__ __attribute__((aligned(16))) uint32_t s_a[T * W];
  __shared__ __attribute__((aligned(16))) uint32_t s_b[T * W];
  __shared__ __attribute__((aligned(16))) double s_pri[T * W];
  __shared__ double2 s_log[BEAR_LOGTAB_N];
  __shared__ double s_red[TS_WAVES][TS_NOUT];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid < BEAR_LOGTAB_N) s_log[tid] = logtab_g[tid];
  double acc[4 * TS_CHUNK], acc_la = 0.0, acc_lb = 0.0;
#pragma unroll
  for (int k = 0; k < 4 * TS_CHUNK; ++k) acc[k] = 0.0;
  const uint64_t n_tiles = (n_rows + T - 1) / T;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * T;
    const uint32_t rows = (uint32_t)((n_rows - row0 < (uint64_t)T) ? (n_rows - row0) : (uint64_t)T);
    __syncthreads();  // previous tile consumed (and the log table is in place)
    stage_dwords<TS_THREADS>(s_a, a + row0 * W, rows * W);
    stage_dwords<TS_THREADS>(s_b, b + row0 * W, rows * W);
    if (use_prior)
      stage_dwords<TS_THREADS>(reinterpret_cast<uint32_t *>(s_pri), reinterpret_cast<const uint32_t *>(prior + row0 * W), rows * W * 2);
    __syncthreads();
#pragma unroll 1
    for (uint32_t r = tid; r < rows; r += TS_THREADS) {
      const uint32_t *ca = s_a + r * W, *cb = s_b + r * W;
      const double *f = s_pri + r * W;
      const uint32_t za = wide_nz_mask<W>(ca), zb = wide_nz_mask<W>(cb);
      double *rt = row_terms ? row_terms + (row0 + r) * (uint64_t)A.n_models + (uint64_t)m0 : nullptr;
      if (!(za | zb)) {          // no transition in either sample: nothing of this row enters any sum
        if (rt)
          for (int mi = 0; mi < m_cnt; ++mi) rt[mi] = 0.0;
        continue;
      }
      double na = 0.0, nb = 0.0;
#pragma unroll
      for (int j = 0; j < W; ++j) {
        na += (double)ca[j];
        nb += (double)cb[j];
      }
      if (do_ar) {
        double la = 0.0, lb = 0.0;
        for (uint32_t nz = za | zb; nz;) {
          const int j = __builtin_ctz(nz);
          nz &= nz - 1u;
          const double lp = ts_log_prior(f[j], s_log);
          if (ca[j]) la = __builtin_fma((double)ca[j], lp, la);
          if (cb[j]) lb = __builtin_fma((double)cb[j], lp, lb);
        }
        acc_la += la;
        acc_lb += lb;
      }
      const bool both = za && zb;
#pragma unroll 1
      for (int mi = 0; mi < m_cnt; ++mi) {
        const int m = m0 + mi;
        const double w = A.w[m];
        const bool ear = m < A.n_h;
        double S = 0.0;
#pragma unroll
        for (int j = 0; j < W; ++j) S += ear ? f[j] * w : w;
        // the row terms -[lgamma(A + n) - lgamma(A)]; the pooled row of a context seen in one sample only IS that sample's row
        double ta = za ? -evs_item_D(S, na, s_log) : 0.0;
        double tb = zb ? -evs_item_D(S, nb, s_log) : 0.0;
        double tab = both ? -evs_item_D(S, na + nb, s_log) : (za ? ta : tb);
        for (uint32_t nz = za | zb; nz;) {
          const int j = __builtin_ctz(nz);
          nz &= nz - 1u;
          const double x = ear ? f[j] * w : w;
          const uint32_t aj = ca[j], bj = cb[j];
          double da = 0.0, db = 0.0;
          if (aj) {
            da = evs_item_D(x, (double)aj, s_log);
            ta += da;
          }
          if (bj) {
            db = evs_item_D(x, (double)bj, s_log);
            tb += db;
          }
          tab += (aj && bj) ? evs_item_D(x, (double)aj + (double)bj, s_log) : (aj ? da : db);
        }
        const double bk = both ? (ta + tb) - tab : 0.0;
        if (rt) rt[mi] = bk;
#pragma unroll
        for (int k = 0; k < TS_CHUNK; ++k)
          if (k == mi) {
            acc[4 * k] += ta;
            acc[4 * k + 1] += tb;
            acc[4 * k + 2] += tab;
            acc[4 * k + 3] += bk;
          }
      }
    }
  }
  // ---- block reduction -> compact partial
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TS_NOUT; ++k) {
    const double v = bear_wave_sum(k < 4 * TS_CHUNK ? acc[k] : (k == 4 * TS_CHUNK ? acc_la : acc_lb));
    if (lane == 0) s_red[wave][k] = v;
  }
  __syncthreads();
  if (tid < TS_NOUT) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < TS_WAVES; ++w) s += s_red[w][tid];
    partials[(size_t)blockIdx.x * TS_NOUT + tid] = s;
  }
}

// The fixed-order sum over the blocks of compact partial k, one wave per value: the four sums of model m0 + k / 4 into out[m, 4],
// and (out_ar != NULL: the launch that carried them) L_a, L_b into out_ar[2]
__global__ __launch_bounds__(256) void two_sample_finalize_kernel(const double *__restrict__ partials, int n_blocks, int m0, int m_cnt,
                                                                 double *__restrict__ out, double *__restrict__ out_ar) {
  const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= TS_NOUT) return;
  double *dst;
  if (k < 4 * TS_CHUNK) {
    if (k / 4 >= m_cnt) return;
    dst = out + (size_t)(m0 + k / 4) * 4 + (k & 3);
  } else {
    if (!out_ar) return;
    dst = out_ar + (k - 4 * TS_CHUNK);
  }
  double s = 0.0;
  for (int blk = lane; blk < n_blocks; blk += 64) s += partials[(size_t)blk * TS_NOUT + k];
  s = bear_wave_sum(s);
  if (lane == 0) *dst = s;
}
