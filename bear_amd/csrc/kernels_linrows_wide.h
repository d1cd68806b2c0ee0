// kernels_linrows_wide.h -- the linear AR function as prior ROWS at width 21 (the protein alphabet: 20 letters + stop), forward and
// backward (bear_linear_forward_wide_f64 / bear_linear_backward_wide_f64).
//
//   forward:   prior_i = softmax_b(sum_l mat[l, code_i[l], b]),  b = 0..20                       (ar_funcs.py:41-45 at alphabet_size 20)
//   backward:  d L / d mat[l, a, :] = sum over contexts with code_i[l] == a of  f_i (q_i - <f_i, q_i>),  q = d L / d prior
//
// Contexts are the int8 [n, lag] code matrix (0..19 residues, 20 = '[', anything else -- -1 -- an all-zero one-hot row: it adds
// nothing forward and receives nothing backward).  No packed form at this width (pack_kmers is 3 bits per letter): lag bytes per
// context are small next to the 168-byte row.
//   forward : mat [lag, 21, 21] in LDS (3528 B per position); one context per lane, its 21 logits are sums of the LDS rows
//             mat[l][a] -- rows of different letters are 21 doubles apart (odd: conflict-free ds_read_b64, kernels_wide.h), lanes with
//             the same letter broadcast.  Max-shifted softmax on the exp table (bear_exp_tab: arguments <= 0, logits of thousands give
//             finite rows).  A tile's rows leave through LDS as 16-byte stores (a row per lane straight to memory is a 168-byte stride).
//   backward: per tile of 128 contexts the rows g = f (q - <f, q>) are formed once in LDS (in place over the staged q rows), then
//             d mat is the fp64 matrix product  G [lag * 21 x 21] += onehot^T [lag * 21 x K] g [K x 21]  on v_mfma_f64_16x16x4_f64:
//             the rows (l, a) of all positions run on as one index r = 21 l + a and are cut into tiles of 16, the 21 output letters
//             into two (the second one holds 5 and zeros).  A wave owns the row tiles wave, wave + 4, ... with both column tiles; their
//             accumulators stay in registers for the block's whole grid-stride loop.  The one-hot operand is built from the code
//             bytes (0 or 1: exact).  No floating-point atomics anywhere: the accumulators go to the workspace as block partials,
//             which are summed in a fixed order in two levels -- the last block to arrive of every residue class mod 16 sums its
//             class (ascending block number), the last class to finish sums the 16 class sums.  The same inputs on the same grid
//             give the same bits, in both builds of the library (no deterministic twin).
//             Grid: min(tiles of 128 contexts, 2 x CUs) blocks (bear_linear.hip, linwide_bwd_grid) -- part of the result.
//             A tile whose g is zero everywhere (contexts without counts) is skipped.
// The row steps (lnw_forward_row of rows_wide_common.h, lnw_softmax_back_row) and the product (lnw_own_rows, lnw_onehot_product, lnw_store_acc) are routines:
// the fused step (kernels_linear_wide.h) runs the same ones on the same block and tile geometry (LNW_BWD_*).
#pragma once
#include "bear_common.h"
#include "kernels_rows.h"
#include "rows_wide_common.h"   // LNW_W, LNW_MAT, lnw_forward_row, wide_store_tile, wide_stage_codes, lnw_sum_rows / lnw_sum_partials

#define LNW_MAX_GRAD (LINEAR_WIDE_MAX_LAG * LNW_MAT)

// the block of the backward kernel and of the fused step: four waves, tiles of 128 contexts, the (l, a) rows of d mat in tiles of 16
#define LNW_BWD_THREADS 256
#define LNW_BWD_WAVES (LNW_BWD_THREADS / 64)
#define LNW_BWD_TILE 128                               // contexts per tile: 21 KiB of f rows + 21 KiB of q rows + the code bytes
#define LNW_BWD_BLOCKS_PER_CU 2                        // the grid cap (part of the result) and the rows of the partials buffer
#define LNW_MAX_RT ((LINEAR_WIDE_MAX_LAG * LNW_W + 15) / 16)                    // row tiles of 16 (l, a) pairs
#define LNW_RT_PER_WAVE ((LNW_MAX_RT + LNW_BWD_WAVES - 1) / LNW_BWD_WAVES)

// ------------------------------------------------------------------ the steps of one context
// softmax backward in place over the row q = d L / d f:  g = f (q - <f, q>) = d L / d logit; true if any entry is not zero
__device__ __forceinline__ bool lnw_softmax_back_row(const double *f, double *g) {
  double s = 0.0;
#pragma unroll
  for (int b = 0; b < LNW_W; ++b) s = __builtin_fma(f[b], g[b], s);
  bool nz = false;
#pragma unroll
  for (int b = 0; b < LNW_W; ++b) {
    const double v = f[b] * (g[b] - s);
    g[b] = v;
    nz |= v != 0.0;
  }
  return nz;
}

// ------------------------------------------------------------------ d mat += onehot^T g over one staged tile
// this lane's row of the one-hot operand in each of the wave's row tiles: position | letter << 8 (a letter no code has beyond the end)
__device__ __forceinline__ void lnw_own_rows(uint32_t wave, uint32_t lr, int n_rows_g, int (&own)[LNW_RT_PER_WAVE]) {
#pragma unroll
  for (int j = 0; j < LNW_RT_PER_WAVE; ++j) {
    const int row = ((int)wave + LNW_BWD_WAVES * j) * 16 + (int)lr;
    own[j] = row < n_rows_g ? (row / LNW_W) | ((row % LNW_W) << 8) : (1000 << 8);
  }
}

// K = 4 contexts per product; product ks takes the contexts ks, ks + 16, ks + 32, ks + 48 of a group of 64 (k index lq): rows 16
// apart are 336 doubles apart, 16 mod 32 -- the 32 lanes of an LDS cycle read 32 different double banks
__device__ __forceinline__ void lnw_onehot_product(const double *s_g, const int8_t *s_c, int lag, int n_rt, uint32_t wave, uint32_t lq,
                                                   uint32_t lr, const int (&own)[LNW_RT_PER_WAVE], lnw_d4 (&acc)[LNW_RT_PER_WAVE][2]) {
#pragma unroll 2
  for (uint32_t ks = 0; ks < LNW_BWD_TILE / 4; ++ks) {
    const uint32_t ctx = ((ks >> 4) << 6) + (ks & 15u) + 16u * lq;
    const double b0 = s_g[ctx * LNW_W + lr];
    const double b1 = lr < LNW_W - 16 ? s_g[ctx * LNW_W + 16 + lr] : 0.0;
    const int8_t *cd = s_c + ctx * (uint32_t)lag;
#pragma unroll
    for (int j = 0; j < LNW_RT_PER_WAVE; ++j) {
      if ((int)wave + LNW_BWD_WAVES * j < n_rt) {        // wave-uniform
        const double a = (int)cd[own[j] & 255] == (own[j] >> 8) ? 1.0 : 0.0;
        acc[j][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, acc[j][0], 0, 0, 0);
        acc[j][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, acc[j][1], 0, 0, 0);
      }
    }
  }
}

// the accumulators into the block's partial [lag * 21, 21] at dst: result r of a lane is row lq + 4 r, column lr of its 16 x 16 tile
__device__ __forceinline__ void lnw_store_acc(double *dst, int n_rows_g, uint32_t wave, uint32_t lq, uint32_t lr,
                                              const lnw_d4 (&acc)[LNW_RT_PER_WAVE][2]) {
#pragma unroll
  for (int j = 0; j < LNW_RT_PER_WAVE; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = ((int)wave + LNW_BWD_WAVES * j) * 16 + (int)lq + 4 * r;
      if (row < n_rows_g) {
        bear_store_agent(&dst[row * LNW_W + (int)lr], acc[j][0][r]);
        if (lr < LNW_W - 16) bear_store_agent(&dst[row * LNW_W + 16 + (int)lr], acc[j][1][r]);
      }
    }
}

// ------------------------------------------------------------------ forward
#define LNW_FWD_THREADS 512
#define LNW_FWD_TILE LNW_FWD_THREADS                   // one context per thread
// dynamic LDS: exp table | a tile's rows | mat  (142 KiB at the longest lag: one block of eight waves per CU)
#define LNW_FWD_LDS(lag) (sizeof(double) * (BEAR_EXPTAB_N + (size_t)LNW_FWD_TILE * LNW_W + (size_t)(lag) * LNW_MAT))
static_assert(LNW_FWD_LDS(LINEAR_WIDE_MAX_LAG) <= 160 * 1024, "linear rows forward at width 21: LDS");

__global__ __launch_bounds__(LNW_FWD_THREADS) void linear_wide_forward_kernel(const int8_t *__restrict__ codes, uint64_t n, int lag,
                                                                              const double *__restrict__ mat,
                                                                              double *__restrict__ prior) {
  extern __shared__ __attribute__((aligned(16))) double lnw_lds[];
  double *exptab = lnw_lds;
  double *R = lnw_lds + BEAR_EXPTAB_N;                 // (1 KiB in: 16-byte aligned)
  double *M = R + LNW_FWD_TILE * LNW_W;
  const uint32_t tid = threadIdx.x;
  if (tid < BEAR_EXPTAB_N) exptab[tid] = exp2((double)tid * (1.0 / BEAR_EXPTAB_N));
  for (int k = tid; k < lag * LNW_MAT; k += LNW_FWD_THREADS) M[k] = mat[k];
  const uint64_t n_tiles = (n + LNW_FWD_TILE - 1) / LNW_FWD_TILE;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * LNW_FWD_TILE;
    const uint32_t rows = (uint32_t)((n - row0 < (uint64_t)LNW_FWD_TILE) ? (n - row0) : (uint64_t)LNW_FWD_TILE);
    __syncthreads();   // the previous tile has left R (and the tables are in place)
    if (tid < rows) lnw_forward_row(codes + (row0 + tid) * (uint64_t)lag, lag, M, exptab, R + tid * LNW_W);
    __syncthreads();
    wide_store_tile<LNW_FWD_THREADS, LNW_W>(R, prior + row0 * LNW_W, rows);
  }
}

// ------------------------------------------------------------------ backward
__global__ __launch_bounds__(LNW_BWD_THREADS) void linear_wide_backward_kernel(const int8_t *__restrict__ codes, uint64_t n, int lag,
                                                                               const double *__restrict__ prior,
                                                                               const double *__restrict__ grad_prior,
                                                                               double *__restrict__ partials, const bear_arrival arrive,
                                                                               double *__restrict__ grad_mat) {
  __shared__ __attribute__((aligned(16))) double s_f[LNW_BWD_TILE * LNW_W];
  __shared__ __attribute__((aligned(16))) double s_g[LNW_BWD_TILE * LNW_W];      // q rows, then g in place
  __shared__ __attribute__((aligned(16))) int8_t s_c[LNW_BWD_TILE * LINEAR_WIDE_MAX_LAG];
  __shared__ unsigned s_flag;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const uint32_t lq = lane >> 4, lr = lane & 15u;        // MFMA lane coordinates: k / row-group index, row / column index
  const int n_grad = lag * LNW_MAT, n_rows_g = lag * LNW_W;
  const int n_rt = (n_rows_g + 15) / 16;
  int own[LNW_RT_PER_WAVE];
  lnw_own_rows(wave, lr, n_rows_g, own);
  lnw_d4 acc[LNW_RT_PER_WAVE][2];
#pragma unroll
  for (int j = 0; j < LNW_RT_PER_WAVE; ++j) acc[j][0] = acc[j][1] = lnw_d4{0.0, 0.0, 0.0, 0.0};
  const uint64_t n_tiles = (n + LNW_BWD_TILE - 1) / LNW_BWD_TILE;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * LNW_BWD_TILE;
    const uint32_t rows = (uint32_t)((n - row0 < (uint64_t)LNW_BWD_TILE) ? (n - row0) : (uint64_t)LNW_BWD_TILE);
    __syncthreads();   // the previous tile's products are done with the LDS rows
    stage_dwords<LNW_BWD_THREADS>(reinterpret_cast<uint32_t *>(s_f), reinterpret_cast<const uint32_t *>(prior + row0 * LNW_W),
                                  rows * LNW_W * 2);
    stage_dwords<LNW_BWD_THREADS>(reinterpret_cast<uint32_t *>(s_g), reinterpret_cast<const uint32_t *>(grad_prior + row0 * LNW_W),
                                  rows * LNW_W * 2);
    wide_stage_codes<LNW_BWD_THREADS>(s_c, codes, row0, rows, lag);
    __syncthreads();
    bool nz = false;
    if (tid < LNW_BWD_TILE) {      // this thread's context: g = d L / d logit, zero beyond the end
      double *g = s_g + tid * LNW_W;
      if (tid < rows) {
        nz = lnw_softmax_back_row(s_f + tid * LNW_W, g);
      } else {
#pragma unroll
        for (int b = 0; b < LNW_W; ++b) g[b] = 0.0;
      }
    }
    if (!__syncthreads_or(nz ? 1 : 0)) continue;         // contexts without counts: nothing to add (block-uniform)
    lnw_onehot_product(s_g, s_c, lag, n_rt, wave, lq, lr, own, acc);
  }
  lnw_store_acc(partials + (size_t)blockIdx.x * n_grad, n_rows_g, wave, lq, lr, acc);
  // ---- fixed-order sum in two levels over the counters of bear_arrive_last (rows_wide_common.h)
  lnw_sum_partials<LNW_BWD_THREADS>(partials, n_grad, arrive, &s_flag, grad_mat);
}
