// kernels_linear_wide.h -- bear_net's training step with the linear AR function at width 21 (the protein alphabet) as ONE kernel:
// bear_dm_linear_wide_f64, bear_net_linear_train_{reduce,step}_wide_f64.  What linear_wide_forward_kernel, dm_wide_kernel<21, AR, true>
// and linear_wide_backward_kernel do in three launches with two row arrays through memory (168 B per context written twice and read
// three times); here a row never leaves the CU.
//
//   block  = 256 threads, tiles of 128 contexts in a grid-stride loop.  Once per block: mat [lag, 21, 21] (dynamic LDS, 3528 B per
//            position: a short lag leaves room for a second block per CU), the exp table, the log table.  h_signed and mat come from the
//            device-resident theta = [h_signed, mat...] when the launch carries one (bear_params_of): the step can be captured.
//   stage  = the tile's uint32 count rows (10.5 KiB) and int8 code bytes as 16-byte loads (stage_dwords).
//   forward= one context per lane of the lower two waves.  A context without counts forms no row and no item (exact zeros).  Else the
//            logits from the LDS rows of mat, the max-shifted softmax on the exp table: the same routine as
//            linear_wide_forward_kernel's (lnw_forward_row) -- the row f (LDS) has the bits of the row entry.
//   DM     = wide_dm_row<21, AR, true> (rows_wide_common.h, the body of dm_wide_kernel) on the staged counts and f: q = d LL / d f into a
//            second LDS row array, sum LL and d / d h per lane.
//   back   = g = f (q - <f, q>) in place over q (lnw_softmax_back_row), then the fp64 MFMA product onehot^T g of
//            linear_wide_backward_kernel (lnw_onehot_product, on that kernel's block and tile: LNW_BWD_*): row tiles of 16 over
//            r = 21 l + a, column tiles 16 + 5, a wave owns the row tiles wave, wave + 4, ..., accumulators in registers for the
//            whole grid-stride loop, the one-hot operand from the code bytes, a tile whose g is zero everywhere skipped.
//   finish = no floating-point atomics.  A block leaves one partial row [sum LL, d/dh, d/d mat] (2 + 441 lag doubles: the packed layout)
//            in the workspace; lnw_sum_partials sums the rows in a fixed order in two levels straight into `packed`; the block that does
//            the final sum then runs the Adam update and the loss record (bear_apply_in_block) when the launch carries one.
//            The same inputs on the same grid give the same bits, in both builds of the library (no deterministic twin).
//   grid   = min(tiles of 128 contexts, LSW_BLOCKS_PER_CU = 2 x CUs) blocks (bear_linear.hip, linstep_wide_grid) -- part of the result.
#pragma once
#include "bear_common.h"
#include "kernels_rows.h"
#include "kernels_linrows_wide.h"   // LNW_MAT, LNW_MAX_GRAD, LNW_BWD_*, the row steps and the product; rows_wide_common.h

#define LSW_THREADS LNW_BWD_THREADS
// the tile and the grid cap (part of the result) as kernels.py names them: those of the product, whose buffer linw_partials is
#define LSW_TILE 128
#define LSW_BLOCKS_PER_CU 2
static_assert(LSW_TILE == LNW_BWD_TILE && LSW_BLOCKS_PER_CU == LNW_BWD_BLOCKS_PER_CU, "the fused step runs lnw_onehot_product");
#define LSW_MAX_PACKED (2 + LNW_MAX_GRAD)              // doubles of a partial row and of `packed`
#define LSW_LDS(lag) (sizeof(double) * (size_t)(lag) * LNW_MAT)     // dynamic: mat

template <bool AR>
__global__ __launch_bounds__(LSW_THREADS, 2) void dm_linear_wide_kernel(const uint32_t *__restrict__ counts, const int8_t *__restrict__ codes,
                                                                     uint64_t n, int lag, const double *__restrict__ mat,
                                                                     bear_params prm_arg, const double2 *__restrict__ logtab_g,
                                                                     double *__restrict__ partials, const bear_step_io io,
                                                                     const bear_apply_io apply) {
  extern __shared__ __attribute__((aligned(16))) double lsw_mat[];
  __shared__ __attribute__((aligned(16))) uint32_t s_cnt[LNW_BWD_TILE * LNW_W];
  __shared__ __attribute__((aligned(16))) double s_f[LNW_BWD_TILE * LNW_W];
  __shared__ __attribute__((aligned(16))) double s_g[LNW_BWD_TILE * LNW_W];      // q rows, then g in place
  __shared__ __attribute__((aligned(16))) int8_t s_c[LNW_BWD_TILE * LINEAR_WIDE_MAX_LAG];
  __shared__ double2 s_log[BEAR_LOGTAB_N];
  __shared__ double s_exp[BEAR_EXPTAB_N];
  __shared__ double s_red[LNW_BWD_WAVES][2];
  __shared__ unsigned s_flag;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const uint32_t lq = lane >> 4, lr = lane & 15u;        // MFMA lane coordinates: k / row-group index, row / column index
  const int n_grad = lag * LNW_MAT, n_rows_g = lag * LNW_W;
  const int n_rt = (n_rows_g + 15) / 16;
  const bear_params prm = bear_params_of(prm_arg, io);
  if (tid < BEAR_LOGTAB_N) s_log[tid] = logtab_g[tid];
  if (tid < BEAR_EXPTAB_N) s_exp[tid] = exp2((double)tid * (1.0 / BEAR_EXPTAB_N));
  for (int k = tid; k < n_grad; k += LSW_THREADS) lsw_mat[k] = mat[k];
  lnw_d4 acc[LNW_RT_PER_WAVE][2];
#pragma unroll
  for (int j = 0; j < LNW_RT_PER_WAVE; ++j) acc[j][0] = acc[j][1] = lnw_d4{0.0, 0.0, 0.0, 0.0};
  double sums[2] = {0.0, 0.0};
  const uint64_t n_tiles = (n + LNW_BWD_TILE - 1) / LNW_BWD_TILE;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * LNW_BWD_TILE;
    const uint32_t rows = (uint32_t)((n - row0 < (uint64_t)LNW_BWD_TILE) ? (n - row0) : (uint64_t)LNW_BWD_TILE);
    __syncthreads();   // the previous tile's products are done with the LDS rows (and the tables are in place)
    stage_dwords<LSW_THREADS>(s_cnt, counts + row0 * LNW_W, rows * LNW_W);
    wide_stage_codes<LSW_THREADS>(s_c, codes, row0, rows, lag);
    __syncthreads();
    bool nz = false;
    if (tid < LNW_BWD_TILE) {
      const uint32_t *c = s_cnt + tid * LNW_W;
      double *f = s_f + tid * LNW_W;
      double *g = s_g + tid * LNW_W;
      if (tid < rows && wide_nz_mask<LNW_W>(c) != 0u) {
        lnw_forward_row(s_c + tid * (uint32_t)lag, lag, lsw_mat, s_exp, f);
        wide_dm_row<LNW_W, AR, true>(c, f, g, prm, s_log, sums);   // q = d LL / d f into g's row
        nz = lnw_softmax_back_row(f, g);                           // g = d LL / d logit
      } else {                                           // no counts, or beyond the end: nothing forward, zeros backward
#pragma unroll
        for (int b = 0; b < LNW_W; ++b) g[b] = 0.0;
      }
    }
    if (!__syncthreads_or(nz ? 1 : 0)) continue;         // contexts without counts: nothing to add (block-uniform)
    // The lane's rows of the one-hot operand are formed per tile, behind an opaque copy of the lane's coordinate: held across the
    // item walk above, these registers and the 96 of the accumulators would not leave it the 256 of two blocks per CU without scratch.
    uint32_t lr_t = lr;
    asm volatile("" : "+v"(lr_t));
    int own[LNW_RT_PER_WAVE];
    lnw_own_rows(wave, lr_t, n_rows_g, own);
    lnw_onehot_product(s_g, s_c, lag, n_rt, wave, lq, lr, own, acc);
  }
  // ---- block partial in the packed layout: [sum LL, d/dh, d/d mat [lag * 21, 21]]
  const int n_packed = 2 + n_grad;
  double *mine = partials + (size_t)blockIdx.x * n_packed;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double v = bear_wave_sum(sums[k]);
    if (lane == 0) s_red[wave][k] = v;
  }
  __syncthreads();
  if (tid < 2) bear_store_agent(&mine[tid], (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]));
  lnw_store_acc(mine + 2, n_rows_g, wave, lq, lr, acc);
  // ---- fixed-order sum in two levels (rows_wide_common.h); the block that wrote `packed` runs the update behind it
  if (lnw_sum_partials<LSW_THREADS>(partials, n_packed, io.arrive(), &s_flag, io.out)) bear_apply_in_block(apply, io.out);
}
