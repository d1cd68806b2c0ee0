// kernels_wide.h -- mode N and the held-out evaluation at a row width W other than the 4-letter alphabets' 5: the protein
// alphabet (20 letters + stop, W = 21).  Instantiated for W = 5 too, so that the tests can hold these kernels against the
// trusted 5-wide entry points (bear_dm_prior_f64, bear_eval_f64); production DNA / RNA keep their own kernels and plans.
//
//   tile   = WIDE_TILE(W) contexts: count rows (4 W B) and prior rows (8 W B) fetched as one flat stream of 16-byte lane loads
//            into LDS (stage_dwords), then each thread reads its own row back.  Stride W dwords (W odd) is conflict-free for
//            ds_read_b32 (bank (a/4) mod 32); stride W doubles = 2W dwords for ds_read_b64 (bank (a/4) mod 64, 32 lanes per
//            LDS cycle): 2W i mod 64 = 2 (W i mod 32) is distinct for 32 lanes when W is odd, and the pair {2k, 2k+1} covers
//            every bank once -- no padding needed.  Gradient rows (GRAD) are written in place into the staged prior rows (a
//            thread only ever touches its own row) and leave as 16-byte stores: no extra LDS.
//   sparse = protein rows are mostly zeros.  A zero cell adds nothing to LL and only the shared row term -psi(A+n)+psi(A) to its
//            gradient, so a lane walks the bit mask of ITS non-zero cells: a wave runs as many item evaluations as the densest
//            row of the wave has non-zero cells, not W.  The row term is paid once per context with n > 0; a context with n = 0
//            costs only its bytes.
//   sums   = per-thread fp64 -> wave -> block partial -> the last block to arrive sums the partials in fixed order (the planned
//            kernels' block_finish): one launch, no atomics on the sums, bit-reproducible for a given grid in both builds.
//            h_signed is read from device memory (bear_params_of), so the step can be captured into a HIP graph.
#pragma once
#include "bear_common.h"
#include "kernels_eval.h"
#include "kernels_rows.h"
#include "rows_wide_common.h"   // wide_nz_mask, wide_dm_row, wide_store_tile

#define WIDE_THREADS 256
// W = 21: 128 contexts = 10.5 KiB of counts + 21 KiB of prior rows (+ 2 KiB log table): LDS for four blocks per CU (160 KiB); the
// 155 VGPRs of the BEAR form leave three.  The upper half of the block stages and writes back; one context per thread of the lower
// half.  Measured 0.16 of 8 TB/s at 13 % non-zero cells: bound by the fp64 items, not the bytes.
#define WIDE_TILE(W) ((W) > 8 ? 128 : 512)
#define WIDE_BLOCKS_PER_CU 4

template <int W, bool AR, bool GRAD>
__global__ __launch_bounds__(WIDE_THREADS) void dm_wide_kernel(const uint32_t *__restrict__ counts, const double *__restrict__ prior,
                                                              uint64_t n_rows, bear_params prm_arg, double *__restrict__ grad_prior,
                                                              const double2 *__restrict__ logtab_g, double *__restrict__ partials,
                                                              const bear_step_io io) {
  static_assert(W <= 32, "the non-zero cells of a row are a 32-bit mask");
  constexpr int T = WIDE_TILE(W);
  __shared__ __attribute__((aligned(16))) uint32_t s_cnt[T * W];
  __shared__ __attribute__((aligned(16))) double s_pri[T * W];
  __shared__ double2 s_log[BEAR_LOGTAB_N];
  const bear_params prm = bear_params_of(prm_arg, io);
  if (threadIdx.x < BEAR_LOGTAB_N) s_log[threadIdx.x] = logtab_g[threadIdx.x];
  const uint64_t n_tiles = (n_rows + T - 1) / T;
  double acc[2] = {0.0, 0.0};
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * T;
    const uint32_t rows = (uint32_t)((n_rows - row0 < (uint64_t)T) ? (n_rows - row0) : (uint64_t)T);
    __syncthreads();  // previous tile consumed and written back (and the log table is in place)
    stage_dwords<WIDE_THREADS>(s_cnt, counts + row0 * W, rows * W);
    stage_dwords<WIDE_THREADS>(reinterpret_cast<uint32_t *>(s_pri), reinterpret_cast<const uint32_t *>(prior + row0 * W), rows * W * 2);
    __syncthreads();
#pragma unroll 1
    for (uint32_t r = threadIdx.x; r < rows; r += WIDE_THREADS) {
      double *f = s_pri + r * W;
      wide_dm_row<W, AR, GRAD>(s_cnt + r * W, f, f, prm, s_log, acc);   // the gradient row in place
    }
    if (GRAD) {
      __syncthreads();   // every row of the tile holds its gradient: 16-byte stores of the whole tile
      wide_store_tile<WIDE_THREADS, W>(s_pri, grad_prior + row0 * W, rows);
    }
  }
  __syncthreads();
  block_finish<2>(acc, partials, io);
}

// ------------------------------------------------------------------ held-out evaluation at width W
// The output of bear_eval_f64 (kernels_eval.h) for rows of W letters: one context per thread, the rows staged through LDS as
// above, a launch carrying at most EVS_CHUNK DM models (register accumulators; more models are further launches, the first one
// also carries the AR model and the total length) and leaving a compact partial per block (EVS_NOUT values) for
// eval_sorted_finalize_kernel.  Per model the log-likelihood is the row term plus one item per non-zero test cell (the bit-mask
// walk of dm_wide_kernel); the arg-max is decided on the concentrations when the top entry leads by more than 17.5 sigma
// (evl_argmax_clear), else by the noise of the letters still in contention only, in fp64 -- with the cell key row * W + letter, so
// at W = 5 every decision is bear_eval_f64's.
#define EVW_THREADS 128
#define EVW_WAVES (EVW_THREADS / 64)

template <int W>
__device__ __forceinline__ bool evw_argmax_clear(const double (&a)[W], double sigma, int &i1, double &top) {
  i1 = 0;
  double v1 = a[0], v2 = -INFINITY;
#pragma unroll
  for (int b = 1; b < W; ++b) {
    if (a[b] > v1) {
      v2 = v1;
      v1 = a[b];
      i1 = b;
    } else if (a[b] > v2) {
      v2 = a[b];
    }
  }
  top = v1;
  return v1 - v2 > 17.5 * sigma;
}

// evl_argmax_exact at width W: the noise of the contenders only (first index on exact ties, index 0 when nothing contends: NaN).
// Called for ties only and kept out of line: the concentrations are formed again from the staged rows (kind 0: AR model,
// 1: BEAR model of weight w, 2: vanilla model of pseudo-count w), so the caller's copy stays in registers.
struct evw_model {
  int kind, has_train, has_prior;
  double w, eps;
};
template <int W>
__device__ __forceinline__ double evw_conc(const evw_model &M, const uint32_t *tr, const double *f, int b) {
  const double fp = M.has_prior ? f[b] : 1.0;
  if (M.kind == 0) return fp + M.eps;
  const double r = M.has_train ? (double)tr[b] : 0.0;
  return M.kind == 1 ? __builtin_fma(fp, M.w, r) + M.eps : (r + M.w) + M.eps;
}
template <int W>
__device__ __noinline__ int evw_argmax_noisy(evw_model M, const uint32_t *tr, const double *f, double top, double sigma, uint64_t seed,
                                             uint32_t model, uint64_t row, const double2 *logtab) {
  const uint64_t base = mix64(seed + (uint64_t)model);
  int i1 = -1;
  double v1 = -INFINITY;
  for (int b = 0; b < W; ++b) {
    const double ab = evw_conc<W>(M, tr, f, b);
    if (top - ab <= 17.5 * sigma) {
      const double v = __builtin_fma(sigma, evl_gauss(evl_key(base, row * (uint64_t)W + (uint64_t)b), logtab), ab);
      if (v > v1) {
        v1 = v;
        i1 = b;
      }
    }
  }
  return i1 < 0 ? 0 : i1;
}

template <int W>
__global__ __launch_bounds__(EVW_THREADS) void eval_wide_kernel(const uint32_t *__restrict__ test, const uint32_t *__restrict__ train,
                                                               const double *__restrict__ prior, uint64_t n_rows, evl_args A, int m0,
                                                               int m_cnt, int do_common, const double2 *__restrict__ logtab_g,
                                                               double *__restrict__ partials) {
  static_assert(W <= 32, "the non-zero cells of a row are a 32-bit mask");
  constexpr int T = EVW_THREADS;
  __shared__ double2 s_log[BEAR_LOGTAB_N];
  __shared__ __attribute__((aligned(16))) uint32_t s_tst[T * W];
  __shared__ __attribute__((aligned(16))) uint32_t s_trn[T * W];
  __shared__ __attribute__((aligned(16))) double s_pri[T * W];
  __shared__ double s_red[EVW_WAVES][EVS_NOUT];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid < BEAR_LOGTAB_N) s_log[tid] = logtab_g[tid];
  double acc_ll[EVS_CHUNK], acc_cor[EVS_CHUNK], acc_arm = 0.0, acc_carm = 0.0, acc_tot = 0.0;
#pragma unroll
  for (int k = 0; k < EVS_CHUNK; ++k) acc_ll[k] = acc_cor[k] = 0.0;
  const double eps = A.eps, sig_dm = 100.0 * A.eps;
  const uint64_t n_tiles = (n_rows + T - 1) / T;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * T;
    const uint32_t rows = (uint32_t)((n_rows - row0 < (uint64_t)T) ? (n_rows - row0) : (uint64_t)T);
    __syncthreads();
    stage_dwords<EVW_THREADS>(s_tst, test + row0 * W, rows * W);
    if (A.has_train) stage_dwords<EVW_THREADS>(s_trn, train + row0 * W, rows * W);
    if (A.has_prior)
      stage_dwords<EVW_THREADS>(reinterpret_cast<uint32_t *>(s_pri), reinterpret_cast<const uint32_t *>(prior + row0 * W), rows * W * 2);
    __syncthreads();
    if (tid >= rows) continue;
    const uint32_t *t = s_tst + tid * W;
    const uint32_t *tr = s_trn + tid * W;
    const double *f = s_pri + tid * W;
    const uint32_t nz_all = wide_nz_mask<W>(t);
    if (!nz_all) continue;          // no held-out counts: nothing of this row enters any sum
    double n = 0.0;
#pragma unroll
    for (int b = 0; b < W; ++b) n += (double)t[b];
    const uint64_t grow = A.row_base + row0 + tid;
    double a[W];
    if (do_common) {
      acc_tot += n;
      if (A.arm) {
        double ll = 0.0;
#pragma unroll
        for (int b = 0; b < W; ++b) a[b] = (A.has_prior ? f[b] : 1.0) + eps;
        for (uint32_t nz = nz_all; nz;) {
          const int b = __builtin_ctz(nz);
          nz &= nz - 1u;
          ll = __builtin_fma((double)t[b], evl_log_any((A.has_prior ? f[b] : 1.0) + eps, s_log), ll);
        }
        acc_arm += ll;
        int im;
        double top;
        if (!evw_argmax_clear<W>(a, eps, im, top))
          im = evw_argmax_noisy<W>(evw_model{0, A.has_train, A.has_prior, 0.0, eps}, tr, f, top, eps, A.seed, EVL_ID_ARM, grow, s_log);
        acc_carm += (double)t[im];
      }
    }
#pragma unroll 1
    for (int mi = 0; mi < m_cnt; ++mi) {
      const int m = m0 + mi;
      const double w = A.inv_h[m];
      const bool ear = m < A.n_h;
      double S = 0.0;
#pragma unroll
      for (int b = 0; b < W; ++b) {
        const double r = A.has_train ? (double)tr[b] : 0.0;
        a[b] = ear ? __builtin_fma(A.has_prior ? f[b] : 1.0, w, r) + eps : (r + w) + eps;
        S += a[b];
      }
      double ll = -evs_item_D(S, n, s_log);
      for (uint32_t nz = nz_all; nz;) {
        const int b = __builtin_ctz(nz);
        nz &= nz - 1u;
        const double r = A.has_train ? (double)tr[b] : 0.0;
        const double x = ear ? __builtin_fma(A.has_prior ? f[b] : 1.0, w, r) + eps : (r + w) + eps;
        ll += evs_item_D(x, (double)t[b], s_log);
      }
      int im;
      double top;
      if (!evw_argmax_clear<W>(a, sig_dm, im, top))
        im = evw_argmax_noisy<W>(evw_model{ear ? 1 : 2, A.has_train, A.has_prior, w, eps}, tr, f, top, sig_dm, A.seed,
                                 ear ? (uint32_t)m : EVL_ID_VAN + (uint32_t)(m - A.n_h), grow, s_log);
      const double hit = (double)t[im];
#pragma unroll
      for (int k = 0; k < EVS_CHUNK; ++k)
        if (k == mi) {
          acc_ll[k] += ll;
          acc_cor[k] += hit;
        }
    }
  }
  // ---- block reduction -> compact partial (the layout of eval_sorted_kernel's, for eval_sorted_finalize_kernel)
  double vals[EVS_NOUT];
#pragma unroll
  for (int k = 0; k < EVS_CHUNK; ++k) {
    vals[k] = acc_ll[k];
    vals[EVS_CHUNK + k] = acc_cor[k];
  }
  vals[2 * EVS_CHUNK] = acc_arm;
  vals[2 * EVS_CHUNK + 1] = acc_carm;
  vals[2 * EVS_CHUNK + 2] = acc_tot;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < EVS_NOUT; ++k) {
    const double v = bear_wave_sum(vals[k]);
    if (lane == 0) s_red[wave][k] = v;
  }
  __syncthreads();
  if (tid < EVS_NOUT) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < EVW_WAVES; ++w) s += s_red[w][tid];
    partials[(size_t)blockIdx.x * EVS_NOUT + tid] = s;
  }
}
