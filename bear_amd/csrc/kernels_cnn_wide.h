// kernels_cnn_wide.h -- the convolutional AR function as prior ROWS at width 21 (the protein alphabet: 20 letters + stop), forward
// and backward (bear_cnn_forward_wide_f64 / bear_cnn_backward_wide_f64): ar_funcs.py:78-97 at alphabet_size 20, num_filters 30,
// kmer_layer1_width 16.
//
//   conv[p][f] = sum_w filters[w][code[p + w]][f]            p = 0 .. P - 1, P = lag - fw + 1   (an unknown letter adds nothing)
//   y0 = scale0 * LN_f(conv) + intercept0 ; e0 = elu(y0)     t1[u] = sum_{p,f} e0[p][f] weights1[p][f][u]
//   y1 = scale1 * LN_u(t1) + intercept1 ;   e1 = elu(y1)     prior = softmax_b(intercept2[b] + sum_u e1[u] weights2[u][b]), b = 0..20
//
// Contexts are the int8 [n, lag] code matrix (0..19 residues, 20 = '[', anything else an all-zero one-hot row), as in
// kernels_linrows_wide.h; a batch of protein contexts shares no windows (21^fw of them, no k-mer order), so none of the prefix levels
// or window tables of kernels_cnn.h apply: a plain pair of row kernels.  The elu, the layer norms, the table exponential and the
// max-shifted softmax are kernels_cnn.h's routines: both widths round alike.
// Packed parameter vector (doubles), the reference's order: filters [fw][21][30] | intercept0 [P][30] | weights1 [P][30][16] |
// intercept1 [16] | weights2 [16][21] | intercept2 [21] | scale0 [P][30] | scale1 [16]     (cnw_make_dims; 8129 at lag 12, fw 8)
//
//   forward : one context per lane.  LDS: the filter image (a row (w, a) of 30 doubles at a stride of 31: rows of different letters
//             start an odd number of doubles apart -- conflict-free ds_read_b64, lanes with the same letter broadcast), weights1,
//             scale0 / intercept0 (read at wave-uniform addresses), the exp table, the tile's code bytes and its rows, which leave
//             as 16-byte nontemporal stores (wide_store_tile).  The rows do not depend on the grid.
//   backward: per tile of 64 contexts.  Wave 0 (lane = context) runs everything that is per context: softmax and layer-1 backward
//             (-> dT1 [16]), then position by position the conv row again, its layer norm and elu, d e0 = dT1 weights1[p]^T and back
//             through elu and layer norm to dconv [30]; it leaves its rows in LDS.  EVERY sum over contexts is then an fp64 matrix
//             product on v_mfma_f64_16x16x4_f64 whose K dimension is the tile's contexts, all four waves, accumulators in registers
//             for the block's whole grid-stride loop:
//               d filters [fw 21 x 30]  += onehot(window p)^T dconv_p        rows (w, a) in tiles of 16, columns 16 + 14; the one-hot
//                                                                            operand from the code bytes (0 or 1: exact)
//               d weights1[p] [30 x 16] += e0_p^T dT1                        rows 16 + 14
//               d intercept0 | d scale0 [P x 60] += onehot(p)^T [dy0 | dy0 n0]     row p of ONE row tile (P <= 16), columns 4 x 16
//               d weights2 [16 x 21]    += e1^T dz                            columns 16 + 5
//               d intercept2 | d scale1 | d intercept1 [1 x 53] += ones^T [dz | dy1 n1 | dy1]      row 0 of a tile
//             A wave owns the filter row tiles wave, wave + 4, ... and the positions wave, wave + 4, ... of d weights1; wave 3 the
//             [P x 60] tiles, waves 2, 1, 0 the head's.  One kernel: at most 24 accumulator tiles per wave (192 registers) next to
//             wave 0's per-context values -- no scratch (profiles/kernel_table_cnn_wide.txt).
//             No floating-point atomics, LDS or global: the accumulators go to the workspace as block partials in the parameter
//             layout and are summed in a fixed order in two levels (lnw_sum_partials).  The same inputs on the same grid give the
//             same bits in both builds of the library (no deterministic twin).
//             Grid: min(ceil(n / 64), CUs) blocks, at least one (bear_cnn.hip, cnnwide_bwd_grid) -- part of the result.
//             A tile whose grad_prior rows are all zero is skipped.
//
// bear_net's training step with this AR function (bear_dm_cnn_wide_f64, bear_net_cnn_train_{reduce,step}_wide_f64) is TWO launches:
//   head    : cnn_wide_head_dm_kernel<AR> -- the forward above plus the DM step of kernels_wide.h (wide_dm_row on the tile's staged
//             count rows) plus dz = f (q - <f, q>) while f is still on the CU, a context per lane of all four waves, tiles of 256.  A
//             context without counts forms no row and no item.  Leaves t1 [n, 16] and the dz rows [n, 21] (16-byte nontemporal
//             stores): no prior row and no gradient row reaches memory.  Sum LL and d/dh: thread -> wave -> block partial, the last
//             block sums the partials in a fixed order into packed[0..1] (block_finish).  Grid: min(ceil(n / 256), CUs) blocks.
//   backward: cnn_wide_backward_kernel<true> -- the backward above with the dz rows loaded instead of formed, its
//             fixed-order sum straight into packed + 2; in the step form the block that wrote it runs the Adam update on the whole
//             packed vector (bear_apply_in_block: the head's two sums are complete by stream order).
//   Why two and not one: the backward runs everything that is per context on wave 0 of a one-block-per-CU grid (the other waves hold
//   the MFMA accumulators); the forward and the item walk run there would be on 64 lanes per CU, a quarter of the head kernel's.  Each
//   launch gets its own stamp on the workspace's arrival words (ws_arrival) and leaves them at zero: they run in stream order.
#pragma once
#include "bear_common.h"
#include "kernels_cnn.h"          // cnn_dims, cnn_elu, cnn_rsqrt, cnn_layer1
#include "kernels_rows.h"         // stage_dwords
#include "rows_wide_common.h"     // wide_store_tile, wide_stage_codes, lnw_sum_partials

#define CNW_W 21
#define CNW_FS 31                                      // doubles between the filter rows (w, a) in LDS: odd
#define CNW_FROWS(fw) ((fw) * CNW_W)

// offsets of the parameter tensors at width 21 (cnn_make_dims is the 5-wide twin)
__host__ __device__ static inline constexpr int cnw_total(int lag, int fw) {
  return fw * CNW_W * CNN_NF + (lag - fw + 1) * (2 * CNN_NF + CNN_NF * CNN_L1) + 2 * CNN_L1 + CNN_L1 * CNW_W + CNW_W;
}
static inline cnn_dims cnw_make_dims(int lag, int fw) {
  cnn_dims d;
  d.lag = lag;
  d.fw = fw;
  d.P = lag - fw + 1;
  d.oF = 0;
  d.ob0 = d.oF + fw * CNW_W * CNN_NF;
  d.oW1 = d.ob0 + d.P * CNN_NF;
  d.ob1 = d.oW1 + d.P * CNN_NF * CNN_L1;
  d.oW2 = d.ob1 + CNN_L1;
  d.ob2 = d.oW2 + CNN_L1 * CNW_W;
  d.os0 = d.ob2 + CNW_W;
  d.os1 = d.os0 + d.P * CNN_NF;
  d.total = d.os1 + CNN_L1;
  return d;
}
// the longest parameter vector: the total is linear in fw, the filters (630 per tap) outweigh a position (540)
#define CNW_MAX_TOTAL cnw_total(CNN_WIDE_MAX_LAG, CNN_WIDE_MAX_LAG)
static_assert(cnw_total(12, 8) == 8129, "parameter count at lag 12, filter width 8");
static_assert(cnw_total(CNN_WIDE_MAX_LAG, 1) <= CNW_MAX_TOTAL, "partials row");

// what every position of every context reads, once per block into LDS: scale0 and intercept0 [P][30], weights1 [P][30][16] and the
// filter image (row (w, a) at CNW_FS doubles)
template <int NT>
__device__ __forceinline__ void cnw_stage_params(double *S0, double *B0, double *W1, double *Fs, const double *__restrict__ params,
                                                 const cnn_dims &D) {
  for (int k = threadIdx.x; k < D.P * CNN_NF; k += NT) {
    S0[k] = params[D.os0 + k];
    B0[k] = params[D.ob0 + k];
  }
  for (int k = threadIdx.x; k < D.P * CNN_NF * CNN_L1; k += NT) W1[k] = params[D.oW1 + k];
  for (int k = threadIdx.x; k < CNW_FROWS(D.fw) * CNN_NF; k += NT) {
    const int r = k / CNN_NF, f = k - r * CNN_NF;
    Fs[r * CNW_FS + f] = params[D.oF + k];
  }
}

// conv row of position p from the code bytes c[0 .. lag), then the layer norm over the filter axis (cnn_conv_norm's arithmetic):
// x <- the normalised row, returns 1 / sqrt(var + eps)
__device__ __forceinline__ double cnw_conv_norm(const double *Fs, const int8_t *c, int p, int fw, bool valid, double (&x)[CNN_NF]) {
#pragma unroll
  for (int f = 0; f < CNN_NF; ++f) x[f] = 0.0;
  if (valid) {
    for (int w = 0; w < fw; ++w) {
      const uint32_t a = (uint32_t)(int)c[p + w];
      if (a < (uint32_t)CNW_W) {                         // anything else: an all-zero one-hot row
        const double *row = Fs + (w * CNW_W + (int)a) * CNW_FS;
#pragma unroll
        for (int f = 0; f < CNN_NF; ++f) x[f] += row[f];
      }
    }
  }
  double m6[6] = {x[0], x[1], x[2], x[3], x[4], x[5]};
#pragma unroll
  for (int f = 6; f < CNN_NF; ++f) m6[f % 6] += x[f];
  const double mu = (((m6[0] + m6[1]) + (m6[2] + m6[3])) + (m6[4] + m6[5])) * (1.0 / CNN_NF);
  double v6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int f = 0; f < CNN_NF; ++f) {
    x[f] -= mu;
    v6[f % 6] = __builtin_fma(x[f], x[f], v6[f % 6]);
  }
  const double var = ((v6[0] + v6[1]) + (v6[2] + v6[3])) + (v6[4] + v6[5]);
  const double r = cnn_rsqrt(var * (1.0 / CNN_NF) + CNN_LN_EPS);
#pragma unroll
  for (int f = 0; f < CNN_NF; ++f) x[f] *= r;
  return r;
}

// ------------------------------------------------------------------ forward
#define CNW_FWD_THREADS 256
#define CNW_FWD_TILE CNW_FWD_THREADS                   // one context per thread
// dynamic LDS (doubles): exp table | a tile's rows | the tile's code bytes | scale0, intercept0 [P][30] each | weights1 [P][30][16] |
// the filter image
__host__ __device__ static inline constexpr size_t cnw_fwd_lds(int lag, int fw) {
  return sizeof(double) * (BEAR_EXPTAB_N + (size_t)CNW_FWD_TILE * CNW_W + (size_t)CNW_FWD_TILE * CNN_WIDE_MAX_LAG / 8 +
                           (size_t)(lag - fw + 1) * (2 * CNN_NF + CNN_NF * CNN_L1) + (size_t)CNW_FROWS(fw) * CNW_FS);
}
// (linear in fw at a given lag: 5208 B per tap against 4320 B per position -- the ends are the extremes)
static_assert(cnw_fwd_lds(CNN_WIDE_MAX_LAG, CNN_WIDE_MAX_LAG) <= 160 * 1024 && cnw_fwd_lds(CNN_WIDE_MAX_LAG, 1) <= 160 * 1024,
              "convolutional rows forward at width 21: LDS");

__global__ __launch_bounds__(CNW_FWD_THREADS) void cnn_wide_forward_kernel(const int8_t *__restrict__ codes, uint64_t n, cnn_dims D,
                                                                           const double *__restrict__ params, double *__restrict__ prior,
                                                                           double *__restrict__ t1_save) {
  extern __shared__ __attribute__((aligned(16))) double cnw_lds[];
  double *exptab = cnw_lds;
  double *R = exptab + BEAR_EXPTAB_N;                                  // (1 KiB in: 16-byte aligned)
  int8_t *s_c = reinterpret_cast<int8_t *>(R + CNW_FWD_TILE * CNW_W);  // (a multiple of 16 bytes further)
  double *S0 = R + CNW_FWD_TILE * CNW_W + CNW_FWD_TILE * CNN_WIDE_MAX_LAG / 8;
  double *B0 = S0 + D.P * CNN_NF;
  double *W1 = B0 + D.P * CNN_NF;
  double *Fs = W1 + D.P * CNN_NF * CNN_L1;
  const uint32_t tid = threadIdx.x;
  if (tid < BEAR_EXPTAB_N) exptab[tid] = exp2((double)tid * (1.0 / BEAR_EXPTAB_N));
  cnw_stage_params<CNW_FWD_THREADS>(S0, B0, W1, Fs, params, D);
  const int lag = D.lag;
  const uint64_t n_tiles = (n + CNW_FWD_TILE - 1) / CNW_FWD_TILE;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * CNW_FWD_TILE;
    const uint32_t rows = (uint32_t)((n - row0 < (uint64_t)CNW_FWD_TILE) ? (n - row0) : (uint64_t)CNW_FWD_TILE);
    __syncthreads();   // the previous tile has left R and s_c (and the tables are in place)
    wide_stage_codes<CNW_FWD_THREADS>(s_c, codes, row0, rows, lag);
    __syncthreads();
    if (tid < rows) {
      const int8_t *c = s_c + tid * (uint32_t)lag;
      double t1[CNN_L1];
#pragma unroll
      for (int u = 0; u < CNN_L1; ++u) t1[u] = 0.0;
      for (int p = 0; p < D.P; ++p) {
        double x[CNN_NF];
        cnw_conv_norm(Fs, c, p, D.fw, true, x);
        const double *s0 = S0 + p * CNN_NF, *b0 = B0 + p * CNN_NF;
        const double2 *w1 = reinterpret_cast<const double2 *>(W1 + p * CNN_NF * CNN_L1);
#pragma unroll
        for (int f = 0; f < CNN_NF; ++f) {
          double dv;
          const double e = cnn_elu(__builtin_fma(s0[f], x[f], b0[f]), exptab, dv);
#pragma unroll
          for (int u2 = 0; u2 < CNN_L1 / 2; ++u2) {
            const double2 w = w1[f * (CNN_L1 / 2) + u2];
            t1[2 * u2] = __builtin_fma(e, w.x, t1[2 * u2]);
            t1[2 * u2 + 1] = __builtin_fma(e, w.y, t1[2 * u2 + 1]);
          }
        }
      }
      if (t1_save) {
        double2 *o = reinterpret_cast<double2 *>(t1_save + (row0 + tid) * CNN_L1);
#pragma unroll
        for (int u2 = 0; u2 < CNN_L1 / 2; ++u2) o[u2] = make_double2(t1[2 * u2], t1[2 * u2 + 1]);
      }
      double n1[CNN_L1], e1[CNN_L1], d1[CNN_L1];
      cnn_layer1(t1, params, D, exptab, n1, e1, d1);
      double z[CNW_W], m = -INFINITY;
#pragma unroll
      for (int b = 0; b < CNW_W; ++b) {
        double s = params[D.ob2 + b];
#pragma unroll
        for (int u = 0; u < CNN_L1; ++u) s = __builtin_fma(e1[u], params[D.oW2 + u * CNW_W + b], s);
        z[b] = s;
        m = s > m ? s : m;
      }
      double tot = 0.0;
#pragma unroll
      for (int b = 0; b < CNW_W; ++b) {
        z[b] = bear_exp_tab(z[b] - m, exptab);
        tot += z[b];
      }
      const double rt = bear_rcp(tot);
      double *r = R + tid * CNW_W;
#pragma unroll
      for (int b = 0; b < CNW_W; ++b) r[b] = z[b] * rt;
    }
    __syncthreads();
    wide_store_tile<CNW_FWD_THREADS, CNW_W>(R, prior + row0 * CNW_W, rows);
  }
}

// ------------------------------------------------------------------ backward
#define CNW_BWD_THREADS 256
#define CNW_BWD_WAVES (CNW_BWD_THREADS / 64)
#define CNW_BWD_TILE 64                                // contexts per tile: a context per lane of wave 0, 16 products of K = 4
#define CNW_BWD_BLOCKS_PER_CU 1                        // the grid cap (part of the result) and the rows of the partials buffer
#define CNW_MAX_RT ((CNW_FROWS(CNN_WIDE_MAX_LAG) + 15) / 16)                    // filter row tiles of 16 (w, a) pairs
#define CNW_RT_PER_WAVE ((CNW_MAX_RT + CNW_BWD_WAVES - 1) / CNW_BWD_WAVES)
#define CNW_P_PER_WAVE ((CNN_WIDE_MAX_LAG + CNW_BWD_WAVES - 1) / CNW_BWD_WAVES)
static_assert(CNN_WIDE_MAX_LAG <= 16, "d intercept0 | d scale0: the positions are the rows of one MFMA tile");
// the staged rows of a tile (strides in doubles: odd, lane = context writes without conflicts).  The head's rows share their
// place with the positions': the head's products are done before the first position is staged.
#define CNW_TS 17                                      // dT1 [16]
#define CNW_HS 53                                      // head: dz [21] | dy1 n1 [16] | dy1 [16]
#define CNW_ES 17                                      //       e1 [16]
#define CNW_XS 31                                      // position: e0 [30]; dconv [30]
#define CNW_YS 61                                      //           dy0 [30] | dy0 n0 [30]
#define CNW_HEAD_DOUBLES (CNW_BWD_TILE * (CNW_HS + CNW_ES))
#define CNW_POS_DOUBLES (CNW_BWD_TILE * (2 * CNW_XS + CNW_YS))
static_assert(CNW_HEAD_DOUBLES <= CNW_POS_DOUBLES, "the head's rows fit where the positions' go");
// dynamic LDS (doubles): exp table | dT1 rows | head / position rows | the tile's code bytes | weights1 [P][30][16] | scale0,
// intercept0 [P][30] each | the filter image
#define CNW_BWD_FIXED_DOUBLES (BEAR_EXPTAB_N + CNW_BWD_TILE * CNW_TS + CNW_POS_DOUBLES + CNW_BWD_TILE * CNN_WIDE_MAX_LAG / 8)
static_assert(CNW_BWD_FIXED_DOUBLES % 2 == 0 && (BEAR_EXPTAB_N + CNW_BWD_TILE * CNW_TS + CNW_POS_DOUBLES) % 2 == 0, "16-byte aligned code bytes");
__host__ __device__ static inline constexpr size_t cnw_bwd_lds(int lag, int fw) {
  return sizeof(double) * (CNW_BWD_FIXED_DOUBLES + (size_t)(lag - fw + 1) * (2 * CNN_NF + CNN_NF * CNN_L1) + (size_t)CNW_FROWS(fw) * CNW_FS);
}
// what CNN_WIDE_MAX_LAG stands for: the filter image of fw = lag taps (5208 B each; a position's weights are 4320 B, so the ends of
// the fw range are the extremes) next to a tile's staged rows (72 KiB) and the 272 static bytes in the 160 KiB of a CU: 157.9 KiB
// at 16, and 17 taps would not fit
static_assert(cnw_bwd_lds(CNN_WIDE_MAX_LAG, CNN_WIDE_MAX_LAG) + 512 <= 160 * 1024 && cnw_bwd_lds(CNN_WIDE_MAX_LAG, 1) + 512 <= 160 * 1024,
              "convolutional rows backward at width 21: LDS");
static_assert(cnw_bwd_lds(CNN_WIDE_MAX_LAG + 1, CNN_WIDE_MAX_LAG + 1) + 272 > 160 * 1024, "CNN_WIDE_MAX_LAG is what fits");

// DZ = false: the rows entry (prior and grad_prior rows in, dz formed here; `apply` is not read).  DZ = true: the second launch of the
// fused step -- `prior` holds the dz rows cnn_wide_head_dm_kernel left, grad_prior is not read, grad_params is packed + 2, and the block
// that wrote the fixed-order sum runs the update on the whole packed vector when the launch carries one.
template <bool DZ>
__global__ __launch_bounds__(CNW_BWD_THREADS) void cnn_wide_backward_kernel(const int8_t *__restrict__ codes, uint64_t n, cnn_dims D,
                                                                            const double *__restrict__ params,
                                                                            const double *__restrict__ t1_save,
                                                                            const double *__restrict__ prior,
                                                                            const double *__restrict__ grad_prior,
                                                                            double *__restrict__ partials, const bear_arrival arrive,
                                                                            double *__restrict__ grad_params, const bear_apply_io apply) {
  extern __shared__ __attribute__((aligned(16))) double cnw_lds[];
  __shared__ unsigned s_flag;
  double *exptab = cnw_lds;
  double *DT = exptab + BEAR_EXPTAB_N;
  double *U = DT + CNW_BWD_TILE * CNW_TS;
  double *HB = U, *HE = U + CNW_BWD_TILE * CNW_HS;                                    // the head's rows ...
  double *E0 = U, *DC = U + CNW_BWD_TILE * CNW_XS, *DY = U + 2 * CNW_BWD_TILE * CNW_XS;   // ... then a position's
  int8_t *s_c = reinterpret_cast<int8_t *>(U + CNW_POS_DOUBLES);
  double *W1s = cnw_lds + CNW_BWD_FIXED_DOUBLES;                                      // (an even number of doubles in: 16-byte aligned)
  double *S0 = W1s + D.P * CNN_NF * CNN_L1, *B0 = S0 + D.P * CNN_NF;
  double *Fs = B0 + D.P * CNN_NF;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const uint32_t lq = lane >> 4, lr = lane & 15u;        // MFMA lane coordinates: k / row-group index, row / column index
  const int lag = D.lag, P = D.P;
  const int n_frows = CNW_FROWS(D.fw), n_rt = (n_frows + 15) / 16;
  if (tid < BEAR_EXPTAB_N) exptab[tid] = exp2((double)tid * (1.0 / BEAR_EXPTAB_N));
  cnw_stage_params<CNW_BWD_THREADS>(S0, B0, W1s, Fs, params, D);
  // this lane's row of the one-hot operand in each of the wave's filter row tiles: tap and letter (a letter no code has beyond the end)
  int own_w[CNW_RT_PER_WAVE], own_a[CNW_RT_PER_WAVE];
  lnw_d4 accF[CNW_RT_PER_WAVE][2], accW[CNW_P_PER_WAVE][2], accH[4];
#pragma unroll
  for (int j = 0; j < CNW_RT_PER_WAVE; ++j) {
    const int row = ((int)wave + CNW_BWD_WAVES * j) * 16 + (int)lr;
    const bool ok = row < n_frows;
    own_w[j] = ok ? row / CNW_W : 0;
    own_a[j] = ok ? row % CNW_W : 1000;
    accF[j][0] = accF[j][1] = lnw_d4{0.0, 0.0, 0.0, 0.0};
  }
#pragma unroll
  for (int j = 0; j < CNW_P_PER_WAVE; ++j) accW[j][0] = accW[j][1] = lnw_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < 4; ++j) accH[j] = lnw_d4{0.0, 0.0, 0.0, 0.0};
  const uint64_t n_tiles = (n + CNW_BWD_TILE - 1) / CNW_BWD_TILE;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * CNW_BWD_TILE;
    const uint32_t rows = (uint32_t)((n - row0 < (uint64_t)CNW_BWD_TILE) ? (n - row0) : (uint64_t)CNW_BWD_TILE);
    __syncthreads();   // the previous tile's products are done with the staged rows (and the tables are in place)
    {   // wide_stage_codes, written out: the call costs this kernel, at 256 + 196 registers, further spills of scalar registers
      const uint32_t n_bytes = rows * (uint32_t)lag;
      const int8_t *src = codes + row0 * (uint64_t)lag;
      stage_dwords<CNW_BWD_THREADS>(reinterpret_cast<uint32_t *>(s_c), reinterpret_cast<const uint32_t *>(src), n_bytes >> 2);
      for (uint32_t i = (n_bytes & ~3u) + tid; i < n_bytes; i += CNW_BWD_THREADS) s_c[i] = src[i];
    }
    // ---- the head, a context per lane of wave 0: dz = f (q - <f, q>), layer 1 again from the kept sums, back to dT1
    const bool valid = wave == 0 && lane < rows;
    bool nz = false;
    double dT1[CNN_L1];
#pragma unroll
    for (int u = 0; u < CNN_L1; ++u) dT1[u] = 0.0;
    if (wave == 0) {
      double *hb = HB + lane * CNW_HS, *he = HE + lane * CNW_ES;
      if (valid) {
        const double *fr = prior + (row0 + lane) * CNW_W;
        double dz[CNW_W];
        if (DZ) {                                        // the head kernel's dz rows as they are
#pragma unroll
          for (int b = 0; b < CNW_W; ++b) {
            dz[b] = fr[b];
            nz |= dz[b] != 0.0;
            hb[b] = dz[b];
          }
        } else {
          const double *qr = grad_prior + (row0 + lane) * CNW_W;
          double s = 0.0;
#pragma unroll
          for (int b = 0; b < CNW_W; ++b) {
            const double q = qr[b];
            dz[b] = q;
            nz |= q != 0.0;
          }
#pragma unroll
          for (int b = 0; b < CNW_W; ++b) {
            const double f = fr[b];
            s = __builtin_fma(f, dz[b], s);
            hb[b] = f;                                   // (parked: dz needs the whole sum)
          }
#pragma unroll
          for (int b = 0; b < CNW_W; ++b) {
            dz[b] = hb[b] * (dz[b] - s);
            hb[b] = dz[b];
          }
        }
        double t1[CNN_L1], n1[CNN_L1], e1[CNN_L1], d1[CNN_L1];
        const double2 *tr = reinterpret_cast<const double2 *>(t1_save + (row0 + lane) * CNN_L1);
#pragma unroll
        for (int u2 = 0; u2 < CNN_L1 / 2; ++u2) {
          const double2 v = tr[u2];
          t1[2 * u2] = v.x;
          t1[2 * u2 + 1] = v.y;
        }
        const double r1 = cnn_layer1(t1, params, D, exptab, n1, e1, d1);
        double m1 = 0.0, m2 = 0.0;
#pragma unroll
        for (int u = 0; u < CNN_L1; ++u) {
          double de = 0.0;
#pragma unroll
          for (int b = 0; b < CNW_W; ++b) de = __builtin_fma(dz[b], params[D.oW2 + u * CNW_W + b], de);
          const double dy = de * d1[u];
          he[u] = e1[u];
          hb[CNW_W + u] = dy * n1[u];
          hb[CNW_W + CNN_L1 + u] = dy;
          const double dn = dy * params[D.os1 + u];
          dT1[u] = dn;
          m1 += dn;
          m2 = __builtin_fma(dn, n1[u], m2);
        }
        m1 *= 1.0 / CNN_L1;
        m2 *= 1.0 / CNN_L1;
#pragma unroll
        for (int u = 0; u < CNN_L1; ++u) dT1[u] = r1 * (dT1[u] - m1 - n1[u] * m2);
      } else {                                           // beyond the end: rows of zeros
#pragma unroll
        for (int k = 0; k < CNW_HS; ++k) hb[k] = 0.0;
#pragma unroll
        for (int u = 0; u < CNN_L1; ++u) he[u] = 0.0;
      }
#pragma unroll
      for (int u = 0; u < CNN_L1; ++u) DT[lane * CNW_TS + u] = dT1[u];
    }
    if (!__syncthreads_or(nz ? 1 : 0)) continue;         // contexts without counts: nothing to add (block-uniform)
    // the head's products.  Product ks takes the contexts ks, ks + 16, ks + 32, ks + 48 (k index lq)
    if (wave < 3) {
      const int c0 = wave == 0 ? 32 : 0;                 // waves 1, 0: the column sums of head columns [0, 32), [32, 53) as row 0
#pragma unroll 2
      for (uint32_t ks = 0; ks < CNW_BWD_TILE / 4; ++ks) {
        const uint32_t ctx = ks + 16u * lq;
        const double *hb = HB + ctx * CNW_HS;
        double a, b0, b1;
        if (wave == 2) {                                 // d weights2 = e1^T dz
          a = HE[ctx * CNW_ES + lr];
          b0 = hb[lr];
          b1 = lr < CNW_W - 16 ? hb[16 + lr] : 0.0;
        } else {
          a = lr == 0 ? 1.0 : 0.0;
          b0 = hb[c0 + (int)lr];
          b1 = c0 + 16 + (int)lr < CNW_HS ? hb[c0 + 16 + (int)lr] : 0.0;
        }
        accH[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, accH[0], 0, 0, 0);
        accH[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, accH[1], 0, 0, 0);
      }
    }
    __syncthreads();   // the head's rows are free
    for (int p = 0; p < P; ++p) {
      if (wave == 0) {
        // ---- position p of this lane's context: conv, layer norm, elu; d e0 = dT1 weights1[p]^T; back to dconv
        double x[CNN_NF], dn[CNN_NF];
        const double r0 = cnw_conv_norm(Fs, s_c + lane * (uint32_t)lag, p, D.fw, valid, x);
        // (weights1, scale0, intercept0 from LDS at wave-uniform addresses: one wave per SIMD has nothing to hide the latency of 480
        // scalar loads per position behind)
        const double *s0 = S0 + p * CNN_NF, *b0 = B0 + p * CNN_NF;
        const double2 *w1 = reinterpret_cast<const double2 *>(W1s + p * CNN_NF * CNN_L1);
        double *e0r = E0 + lane * CNW_XS, *dyr = DY + lane * CNW_YS;
        double m1 = 0.0, m2 = 0.0;
#pragma unroll
        for (int f = 0; f < CNN_NF; ++f) {
          const double sc = s0[f];
          double dv;
          const double e = cnn_elu(__builtin_fma(sc, x[f], b0[f]), exptab, dv);
          double de0 = 0.0, de1 = 0.0;                   // two chains
#pragma unroll
          for (int u2 = 0; u2 < CNN_L1 / 2; ++u2) {
            const double2 w = w1[f * (CNN_L1 / 2) + u2];
            de0 = __builtin_fma(dT1[2 * u2], w.x, de0);
            de1 = __builtin_fma(dT1[2 * u2 + 1], w.y, de1);
          }
          const double dy = (de0 + de1) * dv;
          e0r[f] = e;
          dyr[f] = dy;
          dyr[CNN_NF + f] = dy * x[f];
          dn[f] = dy * sc;
          m1 += dn[f];
          m2 = __builtin_fma(dn[f], x[f], m2);
        }
        m1 *= 1.0 / CNN_NF;
        m2 *= 1.0 / CNN_NF;
        double *dcr = DC + lane * CNW_XS;
#pragma unroll
        for (int f = 0; f < CNN_NF; ++f) dcr[f] = r0 * (dn[f] - m1 - x[f] * m2);
      }
      __syncthreads();
      // ---- the products of position p over the tile's contexts
      const int8_t *cp = s_c + p;
      if ((int)wave == (p & 3)) {                        // d weights1[p] = e0^T dT1 (rows 16 + 14)
#pragma unroll
        for (int j = 0; j < CNW_P_PER_WAVE; ++j)
          if (j == (p >> 2)) {
#pragma unroll 2
            for (uint32_t ks = 0; ks < CNW_BWD_TILE / 4; ++ks) {
              const uint32_t ctx = ks + 16u * lq;
              const double b = DT[ctx * CNW_TS + lr];
              const double a0 = E0[ctx * CNW_XS + lr];
              const double a1 = lr < CNN_NF - 16 ? E0[ctx * CNW_XS + 16 + lr] : 0.0;
              accW[j][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, accW[j][0], 0, 0, 0);
              accW[j][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, accW[j][1], 0, 0, 0);
            }
          }
      }
      if (wave == 3) {                                   // d intercept0 | d scale0: row p of [16 x 60]
        const double a = (int)lr == p ? 1.0 : 0.0;
#pragma unroll 2
        for (uint32_t ks = 0; ks < CNW_BWD_TILE / 4; ++ks) {
          const double *dyr = DY + (ks + 16u * lq) * CNW_YS;
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) {
            const double b = ct * 16 + (int)lr < 2 * CNN_NF ? dyr[ct * 16 + (int)lr] : 0.0;
            accH[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, accH[ct], 0, 0, 0);
          }
        }
      }
#pragma unroll 2
      for (uint32_t ks = 0; ks < CNW_BWD_TILE / 4; ++ks) {   // d filters += onehot(window p)^T dconv (columns 16 + 14)
        const uint32_t ctx = ks + 16u * lq;
        const double b0 = DC[ctx * CNW_XS + lr];
        const double b1 = lr < CNN_NF - 16 ? DC[ctx * CNW_XS + 16 + lr] : 0.0;
        const int8_t *c = cp + ctx * (uint32_t)lag;
#pragma unroll
        for (int j = 0; j < CNW_RT_PER_WAVE; ++j) {
          if ((int)wave + CNW_BWD_WAVES * j < n_rt) {     // wave-uniform
            const double a = (int)c[own_w[j]] == own_a[j] ? 1.0 : 0.0;
            accF[j][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, accF[j][0], 0, 0, 0);
            accF[j][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, accF[j][1], 0, 0, 0);
          }
        }
      }
      __syncthreads();   // done with this position's rows
    }
  }
  // ---- block partial in the parameter layout: result r of a lane is row lq + 4 r, column lr of its 16 x 16 tile
  double *mine = partials + (size_t)blockIdx.x * D.total;
#pragma unroll
  for (int j = 0; j < CNW_RT_PER_WAVE; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = ((int)wave + CNW_BWD_WAVES * j) * 16 + (int)lq + 4 * r;
      if (row < n_frows) {
        bear_store_agent(&mine[D.oF + row * CNN_NF + (int)lr], accF[j][0][r]);
        if (lr < CNN_NF - 16) bear_store_agent(&mine[D.oF + row * CNN_NF + 16 + (int)lr], accF[j][1][r]);
      }
    }
#pragma unroll
  for (int j = 0; j < CNW_P_PER_WAVE; ++j) {
    const int p = (int)wave + CNW_BWD_WAVES * j;
    if (p < P) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = (int)lq + 4 * r;
        bear_store_agent(&mine[D.oW1 + (p * CNN_NF + f) * CNN_L1 + (int)lr], accW[j][0][r]);
        if (f + 16 < CNN_NF) bear_store_agent(&mine[D.oW1 + (p * CNN_NF + f + 16) * CNN_L1 + (int)lr], accW[j][1][r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = (int)lq + 4 * r;
    if (wave == 3) {                                     // row = position: d intercept0 | d scale0
      if (row < P) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const int col = ct * 16 + (int)lr;
          if (col < CNN_NF) bear_store_agent(&mine[D.ob0 + row * CNN_NF + col], accH[ct][r]);
          else if (col < 2 * CNN_NF) bear_store_agent(&mine[D.os0 + row * CNN_NF + col - CNN_NF], accH[ct][r]);
        }
      }
    } else if (wave == 2) {                              // d weights2 [16 x 21]
      bear_store_agent(&mine[D.oW2 + row * CNW_W + (int)lr], accH[0][r]);
      if (lr < CNW_W - 16) bear_store_agent(&mine[D.oW2 + row * CNW_W + 16 + (int)lr], accH[1][r]);
    } else if (row == 0) {                               // row 0: the sums of the head columns d intercept2 | d scale1 | d intercept1
      const int c0 = wave == 0 ? 32 : 0;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const int col = c0 + ct * 16 + (int)lr;
        if (col < CNW_W) bear_store_agent(&mine[D.ob2 + col], accH[ct][r]);
        else if (col < CNW_W + CNN_L1) bear_store_agent(&mine[D.os1 + col - CNW_W], accH[ct][r]);
        else if (col < CNW_HS) bear_store_agent(&mine[D.ob1 + col - CNW_W - CNN_L1], accH[ct][r]);
      }
    }
  }
  if (DZ) {
    // the fused step: packed[0..1] are complete by stream order (the head kernel's launch), packed + 2 is written here
    if (lnw_sum_partials<CNW_BWD_THREADS>(partials, D.total, arrive, &s_flag, grad_params)) bear_apply_in_block(apply, grad_params - 2);
  } else {
    lnw_sum_partials<CNW_BWD_THREADS>(partials, D.total, arrive, &s_flag, grad_params);
  }
}

// ------------------------------------------------------------------ the fused step's first launch: forward + DM step
// A context per lane, every lane of the block: the forward of cnn_wide_forward_kernel on its tile (256 contexts, the same routines, so
// the row f has the bits of the row entry), then wide_dm_row on the tile's staged count rows -- q = d LL / d f in place of f in LDS,
// f itself kept in registers -- and dz = f (q - <f, q>) in the arithmetic of the backward kernel's head.  What leaves: t1 [16] per
// context (zeros for a context without counts: the backward reads every row) and the tile's dz rows; sum LL and d/dh as in
// dm_wide_kernel (block_finish).
#define CNW_HEAD_THREADS 256
#define CNW_HEAD_TILE CNW_HEAD_THREADS                 // one context per thread
#define CNW_HEAD_BLOCKS_PER_CU 1                       // the grid cap (part of the two sums): the count tile leaves no room for a second block
// dynamic LDS (doubles): exp table | log table | a tile's f / q / dz rows | its uint32 count rows | its code bytes | scale0,
// intercept0 [P][30] each | weights1 [P][30][16] | the filter image
#define CNW_HEAD_FIXED_DOUBLES \
  (BEAR_EXPTAB_N + 2 * BEAR_LOGTAB_N + CNW_HEAD_TILE * CNW_W + CNW_HEAD_TILE * CNW_W / 2 + CNW_HEAD_TILE * CNN_WIDE_MAX_LAG / 8)
static_assert((BEAR_EXPTAB_N % 2 == 0) && (CNW_HEAD_TILE * CNW_W) % 4 == 0 && (CNW_HEAD_TILE * CNN_WIDE_MAX_LAG / 8) % 2 == 0,
              "16-byte aligned tables, rows, counts and code bytes");
__host__ __device__ static inline constexpr size_t cnw_head_lds(int lag, int fw) {
  return sizeof(double) * (CNW_HEAD_FIXED_DOUBLES + (size_t)(lag - fw + 1) * (2 * CNN_NF + CNN_NF * CNN_L1) + (size_t)CNW_FROWS(fw) * CNW_FS);
}
// (the ends of the fw range are the extremes, as above; 1168 static bytes of block_finish next to it: 156.7 KiB at fw = lag = 16)
static_assert(cnw_head_lds(CNN_WIDE_MAX_LAG, CNN_WIDE_MAX_LAG) + 1280 <= 160 * 1024 && cnw_head_lds(CNN_WIDE_MAX_LAG, 1) + 1280 <= 160 * 1024,
              "convolutional step head at width 21: LDS");

template <bool AR>
__global__ __launch_bounds__(CNW_HEAD_THREADS) void cnn_wide_head_dm_kernel(const uint32_t *__restrict__ counts, const int8_t *__restrict__ codes,
                                                                           uint64_t n, cnn_dims D, const double *__restrict__ params,
                                                                           bear_params prm_arg, const double2 *__restrict__ logtab_g,
                                                                           double *__restrict__ t1_save, double *__restrict__ dz_rows,
                                                                           double *__restrict__ partials, const bear_step_io io) {
  extern __shared__ __attribute__((aligned(16))) double cnw_lds[];
  double *exptab = cnw_lds;
  double2 *s_log = reinterpret_cast<double2 *>(exptab + BEAR_EXPTAB_N);
  double *R = exptab + BEAR_EXPTAB_N + 2 * BEAR_LOGTAB_N;
  uint32_t *s_cnt = reinterpret_cast<uint32_t *>(R + CNW_HEAD_TILE * CNW_W);
  int8_t *s_c = reinterpret_cast<int8_t *>(R + CNW_HEAD_TILE * CNW_W + CNW_HEAD_TILE * CNW_W / 2);
  double *S0 = cnw_lds + CNW_HEAD_FIXED_DOUBLES;
  double *B0 = S0 + D.P * CNN_NF;
  double *W1 = B0 + D.P * CNN_NF;
  double *Fs = W1 + D.P * CNN_NF * CNN_L1;
  const uint32_t tid = threadIdx.x;
  const bear_params prm = bear_params_of(prm_arg, io);
  if (tid < BEAR_EXPTAB_N) exptab[tid] = exp2((double)tid * (1.0 / BEAR_EXPTAB_N));
  if (tid < BEAR_LOGTAB_N) s_log[tid] = logtab_g[tid];
  cnw_stage_params<CNW_HEAD_THREADS>(S0, B0, W1, Fs, params, D);
  const int lag = D.lag;
  double acc[2] = {0.0, 0.0};
  const uint64_t n_tiles = (n + CNW_HEAD_TILE - 1) / CNW_HEAD_TILE;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * CNW_HEAD_TILE;
    const uint32_t rows = (uint32_t)((n - row0 < (uint64_t)CNW_HEAD_TILE) ? (n - row0) : (uint64_t)CNW_HEAD_TILE);
    __syncthreads();   // the previous tile has left R, s_cnt and s_c (and the tables are in place)
    stage_dwords<CNW_HEAD_THREADS>(s_cnt, counts + row0 * CNW_W, rows * CNW_W);
    wide_stage_codes<CNW_HEAD_THREADS>(s_c, codes, row0, rows, lag);
    __syncthreads();
    if (tid < rows) {
      const uint32_t *cnt = s_cnt + tid * CNW_W;
      double *r = R + tid * CNW_W;
      double2 *o = reinterpret_cast<double2 *>(t1_save + (row0 + tid) * CNN_L1);
      if (wide_nz_mask<CNW_W>(cnt) != 0u) {
        const int8_t *c = s_c + tid * (uint32_t)lag;
        double t1[CNN_L1];
#pragma unroll
        for (int u = 0; u < CNN_L1; ++u) t1[u] = 0.0;
        for (int p = 0; p < D.P; ++p) {
          double x[CNN_NF];
          cnw_conv_norm(Fs, c, p, D.fw, true, x);
          const double *s0 = S0 + p * CNN_NF, *b0 = B0 + p * CNN_NF;
          const double2 *w1 = reinterpret_cast<const double2 *>(W1 + p * CNN_NF * CNN_L1);
#pragma unroll
          for (int f = 0; f < CNN_NF; ++f) {
            double dv;
            const double e = cnn_elu(__builtin_fma(s0[f], x[f], b0[f]), exptab, dv);
#pragma unroll
            for (int u2 = 0; u2 < CNN_L1 / 2; ++u2) {
              const double2 w = w1[f * (CNN_L1 / 2) + u2];
              t1[2 * u2] = __builtin_fma(e, w.x, t1[2 * u2]);
              t1[2 * u2 + 1] = __builtin_fma(e, w.y, t1[2 * u2 + 1]);
            }
          }
        }
#pragma unroll
        for (int u2 = 0; u2 < CNN_L1 / 2; ++u2) o[u2] = make_double2(t1[2 * u2], t1[2 * u2 + 1]);
        double n1[CNN_L1], e1[CNN_L1], d1[CNN_L1];
        cnn_layer1(t1, params, D, exptab, n1, e1, d1);
        double z[CNW_W], m = -INFINITY;
#pragma unroll
        for (int b = 0; b < CNW_W; ++b) {
          double s = params[D.ob2 + b];
#pragma unroll
          for (int u = 0; u < CNN_L1; ++u) s = __builtin_fma(e1[u], params[D.oW2 + u * CNW_W + b], s);
          z[b] = s;
          m = s > m ? s : m;
        }
        double tot = 0.0;
#pragma unroll
        for (int b = 0; b < CNW_W; ++b) {
          z[b] = bear_exp_tab(z[b] - m, exptab);
          tot += z[b];
        }
        const double rt = bear_rcp(tot);
#pragma unroll
        for (int b = 0; b < CNW_W; ++b) {
          z[b] *= rt;                                    // the row f: kept here, and in LDS for the item walk
          r[b] = z[b];
        }
        wide_dm_row<CNW_W, AR, true>(cnt, r, r, prm, s_log, acc);   // q = d LL / d f in place
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < CNW_W; ++b) s = __builtin_fma(z[b], r[b], s);
#pragma unroll
        for (int b = 0; b < CNW_W; ++b) r[b] = z[b] * (r[b] - s);
      } else {                                           // no counts: no row, no item; exact zeros
#pragma unroll
        for (int b = 0; b < CNW_W; ++b) r[b] = 0.0;
#pragma unroll
        for (int u2 = 0; u2 < CNN_L1 / 2; ++u2) o[u2] = make_double2(0.0, 0.0);
      }
    }
    __syncthreads();
    wide_store_tile<CNW_HEAD_THREADS, CNW_W>(R, dz_rows + row0 * CNW_W, rows);
  }
  __syncthreads();
  block_finish<2>(acc, partials, io);
}
