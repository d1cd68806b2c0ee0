// rows_wide_common.h -- device routines the row kernels of the protein alphabet's width share (kernels_linrows_wide.h,
// kernels_cnn_wide.h): a tile of 21-wide rows out of LDS, and the fixed-order sum over rows of block partials.  No kernels here.
#pragma once
#include "bear_common.h"

#define LNW_W 21

typedef double lnw_d4 __attribute__((ext_vector_type(4)));
typedef uint32_t lnw_v4u __attribute__((ext_vector_type(4)));

// rows [0, rows) of an LDS tile of 21-wide fp64 rows to dst (16-byte aligned) as 16-byte stores; nontemporal: not read again here
template <int NT>
__device__ __forceinline__ void lnw_store_tile(const double *tile, double *__restrict__ dst, uint32_t rows) {
  const uint32_t n_dw = rows * LNW_W * 2, n_vec = n_dw >> 2;
  const lnw_v4u *s4 = reinterpret_cast<const lnw_v4u *>(tile);
  lnw_v4u *d4 = reinterpret_cast<lnw_v4u *>(dst);
  for (uint32_t i = threadIdx.x; i < n_vec; i += NT) __builtin_nontemporal_store(s4[i], d4 + i);
  const uint32_t *s1 = reinterpret_cast<const uint32_t *>(tile);
  uint32_t *d1 = reinterpret_cast<uint32_t *>(dst);
  for (uint32_t i = (n_vec << 2) + threadIdx.x; i < n_dw; i += NT) d1[i] = s1[i];
}

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
// not.  Called by every thread of every block once its own row is stored; s_flag: a word of the block's LDS.
template <int NT>
__device__ __forceinline__ void lnw_sum_partials(double *__restrict__ partials, int n_grad, const bear_arrival &arrive, unsigned *s_flag,
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
  if (!*s_flag) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  double *classes = partials + (size_t)grid * n_grad;
  lnw_sum_rows<NT, true>(partials, sub, BEAR_ARRIVE_SUBS, in_sub, n_grad, classes + (size_t)sub * n_grad);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) *s_flag = bear_arrive_count(arrive.word, tag, subs) ? 1u : 0u;
  __syncthreads();
  if (!*s_flag) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  lnw_sum_rows<NT, false>(classes, 0, 1, subs, n_grad, out);
  if (tid == 0) bear_arrive_reset(arrive);
}
