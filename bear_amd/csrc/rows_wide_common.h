// rows_wide_common.h -- device routines the kernels of the protein alphabet's width share (kernels_wide.h, kernels_refmix_wide.h,
// kernels_linrows_wide.h, kernels_linear_wide.h, kernels_cnn_wide.h), each step written once: the DM step of one staged context (the
// sparse item walk, wide_dm_row), a tile of fp64 rows out of LDS (wide_store_tile), a tile's int8 code bytes into LDS
// (wide_stage_codes), the rows of a partials buffer (WIDE_PARTIAL_ROWS), the fixed-order sum over them (lnw_sum_partials) and the
// forward row of the linear function (lnw_forward_row: kernels_linrows_wide.h, kernels_linear_wide.h and, in the unit
// bear_score.hip, kernels_generate.h) and the reference mixing of one row (rfw_ref_total, rfw_dev, rfw_mix_cell:
// kernels_refmix_wide.h and, in bear_score.hip, kernels_refscore.h and kernels_generate.h).  The steps of the linear function
// that need its MFMA geometry (lnw_softmax_back_row,
// lnw_own_rows, lnw_onehot_product, lnw_store_acc) sit at the top of kernels_linrows_wide.h.  No kernels here.
#pragma once
#include "bear_common.h"
#include "kernels_rows.h"   // dm_row_item

#define LNW_W 21
#define LNW_MAT (LNW_W * LNW_W)                        // doubles of mat per position

typedef double lnw_d4 __attribute__((ext_vector_type(4)));
typedef uint32_t lnw_v4u __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ the DM step of one context at width W
template <int W>
__device__ __forceinline__ uint32_t wide_nz_mask(const uint32_t *row) {
  uint32_t m = 0;
#pragma unroll
  for (int b = 0; b < W; ++b) m |= (row[b] != 0u ? 1u : 0u) << b;
  return m;
}

// Mode N of one context out of LDS: counts c[W], prior row f[W]; acc[0] += LL, acc[1] += d LL / d h_signed (BEAR mode), and with GRAD
// the row q[W] = d LL / d f.  A lane walks the bit mask of ITS non-zero cells (kernels_wide.h, "sparse"); a zero cell gets the shared
// row term only.  q may be f itself (dm_wide_kernel: the gradient row in place): every cell is read before it is written.
template <int W, bool AR, bool GRAD>
__device__ __forceinline__ void wide_dm_row(const uint32_t *c, const double *f, double *q, const bear_params &prm, const double2 *s_log,
                                            double (&acc)[2]) {
  uint32_t nz = wide_nz_mask<W>(c);
  if (AR) {      // core.py:138-139 with probs = prior + eps (bear_net.py:68)
    if (GRAD) {
#pragma unroll
      for (int b = 0; b < W; ++b)
        if (!((nz >> b) & 1u)) q[b] = 0.0;
    }
    while (nz) {
      const int b = __builtin_ctz(nz);
      nz &= nz - 1u;
      const double p = f[b] + prm.eps, cb = (double)c[b];
      // the table log is exact to ~1e-16 ABSOLUTE (e ln2 - log r_i cancel for p just above 1): at p = 1 + eps (a one-hot prior
      // row) that is 1e-9 of log p.  Near 1 the polynomial on p - 1 (exact there) keeps it relative.
      const double lp = fabs(p - 1.0) < 0x1p-8 ? bear_log1p_small(p - 1.0) : (p > 0.0 ? bear_log_tab(p, s_log) : bear_log(p));
      acc[0] += cb * lp;
      if (GRAD) q[b] = cb * bear_rcp(p);
    }
  } else {
    double n = 0.0, A = 0.0, sf = 0.0;
#pragma unroll
    for (int b = 0; b < W; ++b) {
      n += (double)c[b];
      A += __builtin_fma(f[b], prm.inv_h, prm.eps);
      sf += f[b];
    }
    if (n == 0.0) {
      if (GRAD) {
#pragma unroll
        for (int b = 0; b < W; ++b) q[b] = 0.0;
      }
      return;
    }
    const bear_dp tn = dm_row_item(A, n, s_log);
    double ll = -tn.D, dh = -tn.P * sf;          // dh = sum_b g_b f_b with g_b = -tn.P + [c_b > 0] item_b.P
    const double g0 = -tn.P * prm.inv_h;
    if (GRAD) {
#pragma unroll
      for (int b = 0; b < W; ++b)
        if (!((nz >> b) & 1u)) q[b] = g0;
    }
    while (nz) {
      const int b = __builtin_ctz(nz);
      nz &= nz - 1u;
      const double fb = f[b];
      const bear_dp tb = dm_row_item(__builtin_fma(fb, prm.inv_h, prm.eps), (double)c[b], s_log);
      ll += tb.D;
      dh = __builtin_fma(tb.P, fb, dh);
      if (GRAD) q[b] = (tb.P - tn.P) * prm.inv_h;
    }
    acc[0] += ll;
    acc[1] -= dh * prm.inv_h;  // d alpha_b / d h_signed = -f_b / h
  }
}

// ------------------------------------------------------------------ the reference mixing of one row at width W
// bear_ref's prior row f = (nw g + jukes_cantor(ref, tau)) / (nw + 1) cell by cell (the formulas: kernels_refmix_wide.h), for the
// training kernels there and, in the unit bear_score.hip, for the rows of queried k-mers (kernels_refscore.h) and the generation
// step (kernels_generate.h).
// R = sum of the letters' r_b = ref_b + eps over a row whose stop entry is zero, added in the order NumPy's add.reduce takes over W
// contiguous doubles: below 8 entries one after the other; else eight running sums over the whole blocks of eight, combined pairwise,
// then the rest one after the other.  (The zero of the stop column changes no partial sum: r >= 0.)
template <int W>
__device__ __forceinline__ double rfw_ref_total(const uint32_t *ref, double eps) {
  constexpr int A = W - 1;
  if (W < 8) {
    double s = (double)ref[0] + eps;
#pragma unroll
    for (int b = 1; b < A; ++b) s += (double)ref[b] + eps;
    return s;
  }
  constexpr int FULL = W - W % 8;
  double q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) q[j] = j < A ? (double)ref[j] + eps : 0.0;
#pragma unroll
  for (int i = 8; i < FULL; i += 8)
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (i + j < A) q[j] += (double)ref[i + j] + eps;
  double s = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
#pragma unroll
  for (int i = FULL; i < A; ++i) s += (double)ref[i] + eps;
  return s;
}

// dev = r / R - 1/A with the quotient rounded as the division rounds it: q = r invR (invR = 1 / R correctly rounded) is within an
// ulp, the remainder r - q R is exact in one fma, and one step on it gives the rounded quotient -- three instructions instead of a
// division sequence per cell.  The subtraction is not fused (the Makefile's -ffp-contract=off).
template <int W>
__device__ __forceinline__ double rfw_dev(double r, double R, double invR) {
  const double q = r * invR;
  const double q1 = __builtin_fma(__builtin_fma(-q, R, r), invR, q);
  return q1 - 1.0 / (W - 1);
}

// cell b of a row whose net entry is g: f_b, d f_b / d tau_signed, d f_b / d nu_signed
struct rfw_cell {
  double f, dft, dfn;
};
template <int W>
__device__ __forceinline__ rfw_cell rfw_mix_cell(const uint32_t *ref, int b, double g, double R, double invR, const bear_params &prm) {
  const bool letter = b < W - 1;
  const double dev = letter ? rfw_dev<W>((double)ref[b] + prm.eps, R, invR) : 0.0;
  const double jc = __builtin_fma(prm.E, dev, letter ? 1.0 / (W - 1) : 0.0);
  rfw_cell o;
  o.f = __builtin_fma(prm.nw, g, jc) * prm.V;
  o.dft = -prm.tauE * dev * prm.V;
  o.dfn = prm.nw * (g - o.f) * prm.V;
  return o;
}

// ------------------------------------------------------------------ the forward row of the linear function at width 21
// f = softmax_b(sum_l M[l, cd[l], b]): the logits from the LDS image M of mat, the max-shifted softmax on the exp table
__device__ __forceinline__ void lnw_forward_row(const int8_t *cd, int lag, const double *M, const double *exptab, double *f) {
  double z[LNW_W];
#pragma unroll
  for (int b = 0; b < LNW_W; ++b) z[b] = 0.0;
  for (int l = 0; l < lag; ++l) {
    const uint32_t a = (uint32_t)(int)cd[l];
    if (a < (uint32_t)LNW_W) {                           // anything else: an all-zero one-hot row
      const double *m = M + (l * LNW_W + (int)a) * LNW_W;
#pragma unroll
      for (int b = 0; b < LNW_W; ++b) z[b] += m[b];
    }
  }
  double zmax = z[0];
#pragma unroll
  for (int b = 1; b < LNW_W; ++b) zmax = __builtin_fmax(zmax, z[b]);
  double s = 0.0;
#pragma unroll
  for (int b = 0; b < LNW_W; ++b) {
    z[b] = bear_exp_tab(z[b] - zmax, exptab);
    s += z[b];
  }
  const double inv = 1.0 / s;                            // s >= 1: the largest logit contributes exp(0)
#pragma unroll
  for (int b = 0; b < LNW_W; ++b) f[b] = z[b] * inv;
}

// rows [0, rows) of an LDS tile of W-wide fp64 rows to dst (16-byte aligned) as 16-byte stores; nontemporal: not read again here
template <int NT, int W>
__device__ __forceinline__ void wide_store_tile(const double *tile, double *__restrict__ dst, uint32_t rows) {
  const uint32_t n_dw = rows * W * 2, n_vec = n_dw >> 2;
  const lnw_v4u *s4 = reinterpret_cast<const lnw_v4u *>(tile);
  lnw_v4u *d4 = reinterpret_cast<lnw_v4u *>(dst);
  for (uint32_t i = threadIdx.x; i < n_vec; i += NT) __builtin_nontemporal_store(s4[i], d4 + i);
  const uint32_t *s1 = reinterpret_cast<const uint32_t *>(tile);
  uint32_t *d1 = reinterpret_cast<uint32_t *>(dst);
  for (uint32_t i = (n_vec << 2) + threadIdx.x; i < n_dw; i += NT) d1[i] = s1[i];
}

// the code bytes of rows [row0, row0 + rows) of the int8 [n, lag] matrix into s_c (row0 lag a multiple of 16, codes 16-byte aligned):
// whole dwords as 16-byte loads, the last bytes one by one -- nothing is read beyond the matrix
template <int NT>
__device__ __forceinline__ void wide_stage_codes(int8_t *s_c, const int8_t *__restrict__ codes, uint64_t row0, uint32_t rows, int lag) {
  const uint32_t n_bytes = rows * (uint32_t)lag;
  const int8_t *src = codes + row0 * (uint64_t)lag;
  stage_dwords<NT>(reinterpret_cast<uint32_t *>(s_c), reinterpret_cast<const uint32_t *>(src), n_bytes >> 2);
  for (uint32_t i = (n_bytes & ~3u) + threadIdx.x; i < n_bytes; i += NT) s_c[i] = src[i];
}

// rows of a partials buffer that lnw_sum_partials sums: one per block of a grid capped at blocks_per_cu per CU, then one per residue
// class of the block numbers (bear_arrive_last's counters)
#define WIDE_PARTIAL_ROWS(num_cu, blocks_per_cu) ((size_t)(num_cu) * (blocks_per_cu) + BEAR_ARRIVE_SUBS)

// dst[k] = src[first][k] + src[first + step][k] + ... (cnt rows of n_grad doubles, in that order), k over the block's NT threads
template <int NT, bool AGENT>
__device__ __forceinline__ void lnw_sum_rows(const double *__restrict__ src, uint32_t first, uint32_t step, uint32_t cnt, int n_grad,
                                             double *__restrict__ dst) {
  for (int k = threadIdx.x; k < n_grad; k += NT) {
    double s = 0.0;
    for (uint32_t i = 0; i < cnt; i += 8) {              // eight independent loads in flight, added in order
      double v[8];
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) v[j] = i + j < cnt ? src[(size_t)(first + (i + j) * step) * n_grad + k] : 0.0;
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) s += v[j];
    }
    if (AGENT) bear_store_agent(&dst[k], s);
    else dst[k] = s;
  }
}

// The fixed-order sum of a grid's block partials (rows of n_grad doubles at `partials`, one per block, written with
// bear_store_agent; 16 more rows behind them) in two levels over the counters of bear_arrive_last: a block arrives at the counter
// of its number mod 16; the last one there sums that class, ascending, into the row behind the blocks' and arrives at the top
// word; the last one there sums the class rows into `out`.  Which block does either is arbitrary, what it adds in which order is
// not.  Called by every thread of every block once its own row is stored; s_flag: a word of the block's LDS.  True (block-uniform)
// in the block that wrote `out`.
template <int NT>
__device__ __forceinline__ bool lnw_sum_partials(double *__restrict__ partials, int n_grad, const bear_arrival &arrive, unsigned *s_flag,
                                                 double *__restrict__ out) {
  const uint32_t tid = threadIdx.x;
  const unsigned grid = gridDim.x, sub = blockIdx.x % BEAR_ARRIVE_SUBS;
  const unsigned in_sub = (grid - sub + BEAR_ARRIVE_SUBS - 1u) / BEAR_ARRIVE_SUBS;
  const unsigned subs = grid < BEAR_ARRIVE_SUBS ? grid : BEAR_ARRIVE_SUBS;
  const unsigned long long tag = (unsigned long long)arrive.epoch << 24;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this block's partials are acknowledged (bear_arrive_last)
  __syncthreads();
  if (tid == 0) *s_flag = bear_arrive_count(arrive.word + (1u + sub) * BEAR_ARRIVE_STRIDE, tag, in_sub) ? 1u : 0u;
  __syncthreads();
  if (!*s_flag) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  double *classes = partials + (size_t)grid * n_grad;
  lnw_sum_rows<NT, true>(partials, sub, BEAR_ARRIVE_SUBS, in_sub, n_grad, classes + (size_t)sub * n_grad);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) *s_flag = bear_arrive_count(arrive.word, tag, subs) ? 1u : 0u;
  __syncthreads();
  if (!*s_flag) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  lnw_sum_rows<NT, false>(classes, 0, 1, subs, n_grad, out);
  if (tid == 0) bear_arrive_reset(arrive);
  return true;
}
