// kernels_probe.h -- the device math routines one at a time (tests / diagnostics, as dm_items_kernel): every routine of
// bear_math.h and the item routines of both kernel families, called as the production kernels call them -- the routine itself,
// never a copy -- on tables staged as those kernels stage them (the log table of the workspace into LDS, the exp table by
// exp2((double)k / 128) on the device).  tests/test_math_probe_gpu.py holds each to a 40-digit reference, value by value.
#pragma once
#include "bear_common.h"
#include "sorted_common.h"   // srt_general, srt_general_fast, srt_general_auto
#include "kernels_rows.h"    // dm_row_item

// out0[i] (and out1[i], the item routines' P) = routine `op` (BEAR_PROBE_*, include/bear_hip.h) of a[i] (and b[i], the item
// routines' count as a double)
static inline bool probe_is_item(int op) { return op >= BEAR_PROBE_SRT_GENERAL && op <= BEAR_PROBE_ROW_ITEM; }

// One element per thread; `op` is uniform over the launch, so every wave is whole (64 lanes, elements past n read as 0) in the two
// reductions, where every lane writes its own copy of the wave's result.
__global__ __launch_bounds__(256) void math_probe_kernel(int op, const double *__restrict__ a, const double *__restrict__ b, uint64_t n,
                                                         const double2 *__restrict__ logtab_g, double *__restrict__ out0,
                                                         double *__restrict__ out1) {
  __shared__ double2 logtab[BEAR_LOGTAB_N];
  __shared__ double exptab[BEAR_EXPTAB_N];
  if (threadIdx.x < BEAR_LOGTAB_N) logtab[threadIdx.x] = logtab_g[threadIdx.x];
  for (int k = threadIdx.x; k < BEAR_EXPTAB_N; k += 256) exptab[k] = exp2((double)k * (1.0 / BEAR_EXPTAB_N));
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool on = i < n;
  const double x = on ? a[i] : 0.0;
  const double c = on && b ? b[i] : 1.0;
  double r0 = 0.0, r1 = 0.0;
  bear_dp o;
  switch (op) {
    case BEAR_PROBE_RCP: r0 = bear_rcp(x); break;
    case BEAR_PROBE_LOG_TAB: r0 = bear_log_tab<false>(x, logtab); break;
    case BEAR_PROBE_LOG_TAB_V: r0 = bear_log_tab<true>(x, logtab); break;
    case BEAR_PROBE_LOG1P_SMALL: r0 = bear_log1p_small<false>(x); break;
    case BEAR_PROBE_LOG1P_SMALL_V: r0 = bear_log1p_small<true>(x); break;
    case BEAR_PROBE_LOG1P_POS: r0 = bear_log1p_pos(x); break;
    case BEAR_PROBE_EXP_TAB: r0 = bear_exp_tab(x, exptab); break;
    case BEAR_PROBE_CNN_EXP_NEG: r0 = cnn_exp_neg(x, exptab); break;
    case BEAR_PROBE_LIN_EXP_UNITS: r0 = lin_exp_units(x, exptab); break;
    case BEAR_PROBE_STIR_LG: r0 = bear_stir_lg(x); break;
    case BEAR_PROBE_STIR_PSI: r0 = bear_stir_psi(x); break;
    case BEAR_PROBE_WAVE_SUM: r0 = bear_wave_sum(x); break;
    case BEAR_PROBE_WAVE_MAX: r0 = bear_wave_max(x); break;
    case BEAR_PROBE_SRT_GENERAL: o = srt_general(x, c); r0 = o.D; r1 = o.P; break;
    case BEAR_PROBE_SRT_GENERAL_FAST: o = srt_general_fast(x, c, logtab); r0 = o.D; r1 = o.P; break;
    case BEAR_PROBE_SRT_GENERAL_AUTO: o = srt_general_auto(x, c, logtab); r0 = o.D; r1 = o.P; break;
    case BEAR_PROBE_ROW_ITEM_TAB: o = dm_row_item(x, c, logtab); r0 = o.D; r1 = o.P; break;
    case BEAR_PROBE_ROW_ITEM: o = dm_row_item(x, c, nullptr); r0 = o.D; r1 = o.P; break;
    case BEAR_PROBE_PSI: r0 = bear_psi(x); break;
    case BEAR_PROBE_PSI1: r0 = bear_psi1(x); break;
    default: break;
  }
  if (on) {
    out0[i] = r0;
    if (out1) out1[i] = r1;
  }
}
