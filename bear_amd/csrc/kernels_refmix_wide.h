// kernels_refmix_wide.h -- bear_ref's training step at a row width W other than 5 (the protein alphabet, W = 21): the reference
// mixing of bear_ref.py:63-68 inside the DM step, from the uint32 count rows the resident batches hold.  Instantiated for W = 5
// too, so that the tests can hold these kernels against the trusted 5-wide entries (bear_dm_ref_f64, bear_dm_refmix_plan_grad_f64).
//
// With A = W - 1 letters and the stop column last (oracle/bear_oracle.py: bear_ref_step):
//   r_b   = ref_b + eps (b < A), r_A = 0;   R = sum_b r_b;   dev_b = r_b / R - 1/A (b < A), dev_A = 0
//   jc_b  = [b < A] / A + E dev_b;   f_b = (nw g_b + jc_b) V;   E = exp(-tau), V = 1 / (nw + 1), tau = exp(tau_signed), nw = exp(nu_signed)
//   d f_b / d tau_signed = -tau E dev_b V;   d f_b / d nu_signed = nw (g_b - f_b) V
//   BEAR mode: alpha_b = f_b / h + eps, d LL / d f_b = (P_b [c_b > 0] - P_n) / h;   AR mode: p_b = f_b + eps, d LL / d f_b = c_b / p_b
//
//   dm_ref_wide_kernel     the stop net function (g = one-hot at the stop column): train and reference rows in (8 W B per context),
//                          [sum LL, d/dh_signed, d/dtau_signed, d/dnu_signed] out; no prior row exists anywhere.  The finish is
//                          dm_ref_rows_kernel's: the last block's fixed-order sum and, for a whole step, the Adam update behind it.
//   dm_refmix_wide_kernel  a net function with parameters: its rows g (fp64) in as well, the same four sums and
//                          d sum LL / d g = d LL / d f  nw V out, written in place over the staged rows (16 W B in, 8 W B out).
//                          Nothing is assumed of g but g >= 0: sum g and sum f are formed from the row.
//
// Both have dm_wide_kernel's structure (kernels_wide.h): tiles through LDS as 16-byte lane loads (stride W dwords / W doubles, W odd:
// conflict-free), a context per lane, a dm_row_item per NON-ZERO training cell (the bit mask of the row) and one for the row term; a
// context without training counts adds exact zeros and costs its bytes only.  A zero cell needs no item: its d LL / d f is the row
// term -P_n / h alone, so the zero cells' share of a gradient is the row term times (the sum over ALL cells) - (the sum over the
// non-zero cells) of d f / d parameter -- and the sums over all cells are sum dev, sum g and sum f, which one static pass over the
// row yields without an item.
// sum dev is formed, not taken as zero: for a reference row that is flat (a context the reference never saw: all eps) every dev_b is
// the same rounding residue of r / R - 1/A, the gradient of tau is that residue times a sum of O(1) terms, and only the residue the
// oracle's arithmetic leaves is "right" to the 2e-13 of the L1 mass the tests hold a gradient to.  So R is summed in the order NumPy
// sums a row (rfw_ref_total), r / R is rounded as a division rounds it (rfw_dev) and 1/A is subtracted unfused.
// No floating-point atomics: block partials and block_finish only -- equal inputs, equal bits for a given grid, in both builds.
#pragma once
#include "bear_common.h"
#include "kernels_rows.h"
#include "kernels_wide.h"
#include "rows_wide_common.h"   // wide_nz_mask, wide_store_tile; rfw_ref_total, rfw_dev, rfw_mix_cell (shared with the scoring unit)

#define RFW_THREADS 256
// dm_ref_wide_kernel, W = 21: 256 contexts = two count tiles of 21 KiB (+ 2 KiB log table): a context on every thread, three blocks
// per CU by LDS and by registers alike (profiles/kernel_table_refmix_wide.txt).
#define RFW_TILE(W) ((W) > 8 ? 256 : 512)
#define RFW_BLOCKS_PER_CU 3
// dm_refmix_wide_kernel, W = 21: 128 contexts = 21 KiB of counts + 21 KiB of net rows: three blocks per CU; the upper half of the
// block stages and writes back only (as dm_wide_kernel).
#define RMW_TILE(W) ((W) > 8 ? 128 : 512)
#define RMW_BLOCKS_PER_CU 3

// sum_b dev_b over the letters (all W cells: dev of the stop column is zero)
template <int W>
__device__ __forceinline__ double rfw_dev_total(const uint32_t *ref, double eps, double R, double invR) {
  double s = 0.0;
#pragma unroll
  for (int b = 0; b < W - 1; ++b) s += rfw_dev<W>((double)ref[b] + eps, R, invR);
  return s;
}

// c log p of the multinomial mode, as dm_wide_kernel forms it (near p = 1 -- the stop entry under a large net weight -- the
// polynomial on p - 1 keeps the table log's absolute error relative)
__device__ __forceinline__ double rfw_log(double p, const double2 *s_log) {
  return fabs(p - 1.0) < 0x1p-8 ? bear_log1p_small(p - 1.0) : (p > 0.0 ? bear_log_tab(p, s_log) : bear_log(p));
}

// One context of either kernel: c and rf its staged count and reference rows; acc += [LL, d/dh_signed, d/dtau_signed, d/dnu_signed].
//   MIX   g its net row in, d sum LL / d g out in place (a context without training counts: exact zeros)
//   else  the stop net function: g_b = [b == W - 1] and sum g = 1 are constants, g is not touched and no row is written.  The
//         expressions are the same ones (no contraction: fma(nw, 1, x) is nw + x), so a stop row through MIX gives these bits.
template <int W, bool AR, bool MIX>
__device__ __forceinline__ void rfw_row(const uint32_t *c, const uint32_t *rf, double *g, const bear_params &prm, const double2 *s_log,
                                        double (&acc)[4]) {
  uint32_t nz = wide_nz_mask<W>(c);
  if (!nz) {                         // no training counts: nothing of this context enters any sum
    if (MIX) {
#pragma unroll
      for (int b = 0; b < W; ++b) g[b] = 0.0;
    }
    return;
  }
  const double nwV = prm.nw * prm.V;
  const double R = rfw_ref_total<W>(rf, prm.eps), invR = 1.0 / R;
  double ll = 0.0, dh = 0.0, dt = 0.0, dn = 0.0, scale = 1.0, g0 = 0.0;   // sums over the cells of P_b (AR: c_b / p_b) times f, df/dtau, df/dnu
  bear_dp tn = {0.0, 0.0};
  if (!AR) {
    double n = 0.0, sg = MIX ? 0.0 : 1.0;
#pragma unroll
    for (int b = 0; b < W; ++b) {
      n += (double)c[b];
      if (MIX) sg += g[b];
    }
    const double sdev = rfw_dev_total<W>(rf, prm.eps, R, invR);
    const double sf = __builtin_fma(prm.nw, sg, __builtin_fma(prm.E, sdev, 1.0)) * prm.V;
    tn = dm_row_item(__builtin_fma(sf, prm.inv_h, (double)W * prm.eps), n, s_log);
    ll = -tn.D;
    dh = -tn.P * sf;
    dt = tn.P * (prm.tauE * prm.V * sdev);
    dn = -tn.P * (nwV * (sg - sf));
    scale = prm.inv_h;
    g0 = -tn.P * prm.inv_h * nwV;
  }
  if (MIX) {
#pragma unroll
    for (int b = 0; b < W; ++b)
      if (!((nz >> b) & 1u)) g[b] = g0;
  }
  while (nz) {
    const int b = __builtin_ctz(nz);
    nz &= nz - 1u;
    const double cb = (double)c[b];
    const rfw_cell m = rfw_mix_cell<W>(rf, b, MIX ? g[b] : (b == W - 1 ? 1.0 : 0.0), R, invR, prm);
    double q;
    if (AR) {
      const double p = m.f + prm.eps;
      ll = __builtin_fma(cb, rfw_log(p, s_log), ll);
      q = cb * bear_rcp(p);
      if (MIX) g[b] = q * nwV;
    } else {
      const bear_dp tb = dm_row_item(__builtin_fma(m.f, prm.inv_h, prm.eps), cb, s_log);
      ll += tb.D;
      q = tb.P;
      dh = __builtin_fma(q, m.f, dh);
      if (MIX) g[b] = (tb.P - tn.P) * prm.inv_h * nwV;
    }
    dt = __builtin_fma(q, m.dft, dt);
    dn = __builtin_fma(q, m.dfn, dn);
  }
  acc[0] += ll;
  acc[1] -= dh * scale;              // d alpha_b / d h_signed = -f_b / h (AR: dh stays zero)
  acc[2] += dt * scale;
  acc[3] += dn * scale;
}

// ------------------------------------------------------------------ the stop net function
template <int W, bool AR>
__global__ __launch_bounds__(RFW_THREADS) void dm_ref_wide_kernel(const uint32_t *__restrict__ train, const uint32_t *__restrict__ ref,
                                                                 uint64_t n_rows, bear_params prm_arg, const double2 *__restrict__ logtab_g,
                                                                 double *__restrict__ partials, const bear_step_io io,
                                                                 const bear_apply_io apply) {
  static_assert(W <= 32, "the non-zero cells of a row are a 32-bit mask");
  constexpr int T = RFW_TILE(W);
  __shared__ __attribute__((aligned(16))) uint32_t s_trn[T * W];
  __shared__ __attribute__((aligned(16))) uint32_t s_ref[T * W];
  __shared__ double2 s_log[BEAR_LOGTAB_N];
  const bear_params prm = bear_params_of(prm_arg, io);
  if (threadIdx.x < BEAR_LOGTAB_N) s_log[threadIdx.x] = logtab_g[threadIdx.x];
  const uint64_t n_tiles = (n_rows + T - 1) / T;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * T;
    const uint32_t rows = (uint32_t)((n_rows - row0 < (uint64_t)T) ? (n_rows - row0) : (uint64_t)T);
    __syncthreads();  // previous tile consumed (and the log table is in place)
    stage_dwords<RFW_THREADS>(s_trn, train + row0 * W, rows * W);
    stage_dwords<RFW_THREADS>(s_ref, ref + row0 * W, rows * W);
    __syncthreads();
#pragma unroll 1
    for (uint32_t r = threadIdx.x; r < rows; r += RFW_THREADS)
      rfw_row<W, AR, false>(s_trn + r * W, s_ref + r * W, nullptr, prm, s_log, acc);
  }
  __syncthreads();
  block_finish<4>(acc, partials, io, apply);
}

// ------------------------------------------------------------------ a net function with parameters
template <int W, bool AR>
__global__ __launch_bounds__(RFW_THREADS) void dm_refmix_wide_kernel(const uint32_t *__restrict__ counts, const double *__restrict__ net_rows,
                                                                    const uint32_t *__restrict__ ref, uint64_t n_rows,
                                                                    const double *__restrict__ h_s, const double *__restrict__ tau_s,
                                                                    const double *__restrict__ nw_s, double eps,
                                                                    const double2 *__restrict__ logtab_g, double *__restrict__ grad_net_rows,
                                                                    double *__restrict__ partials, const bear_step_io io) {
  static_assert(W <= 32, "the non-zero cells of a row are a 32-bit mask");
  constexpr int T = RMW_TILE(W);
  __shared__ __attribute__((aligned(16))) uint32_t s_cnt[T * W];
  __shared__ __attribute__((aligned(16))) uint32_t s_ref[T * W];
  __shared__ __attribute__((aligned(16))) double s_net[T * W];   // g in, d sum LL / d g out
  __shared__ double2 s_log[BEAR_LOGTAB_N];
  const bear_params prm = bear_params_dev(eps, true, h_s, tau_s, nw_s);
  if (threadIdx.x < BEAR_LOGTAB_N) s_log[threadIdx.x] = logtab_g[threadIdx.x];
  const uint64_t n_tiles = (n_rows + T - 1) / T;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * T;
    const uint32_t rows = (uint32_t)((n_rows - row0 < (uint64_t)T) ? (n_rows - row0) : (uint64_t)T);
    __syncthreads();  // previous tile consumed and written back (and the log table is in place)
    stage_dwords<RFW_THREADS>(s_cnt, counts + row0 * W, rows * W);
    stage_dwords<RFW_THREADS>(s_ref, ref + row0 * W, rows * W);
    stage_dwords<RFW_THREADS>(reinterpret_cast<uint32_t *>(s_net), reinterpret_cast<const uint32_t *>(net_rows + row0 * W), rows * W * 2);
    __syncthreads();
#pragma unroll 1
    for (uint32_t r = threadIdx.x; r < rows; r += RFW_THREADS)
      rfw_row<W, AR, true>(s_cnt + r * W, s_ref + r * W, s_net + r * W, prm, s_log, acc);
    __syncthreads();   // every row of the tile holds its gradient: 16-byte stores of the whole tile
    wide_store_tile<RFW_THREADS, W>(s_net, grad_net_rows + row0 * W, rows);
  }
  __syncthreads();
  block_finish<4>(acc, partials, io);
}
