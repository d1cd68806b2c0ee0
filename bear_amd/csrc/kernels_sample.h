// kernels_sample.h -- posterior sampling of transition probabilities.
//
// Replaces, for a batch of k-mer contexts, the sampling half of get_var_probs.get_pdf
// (bear_model/get_var_probs.py:91-194) and the sampler it calls, log_gamma.log_gamma
// (bear_model/log_gamma.py:17-76):
//   concs[m, k, :] = ar_vals[k, :] / h_m + counts[k, :]      (BEAR models, get_var_probs.py:141-149)
//                  = van_m + counts[k, :]                    (vanilla models, :138, :149)
//                  = ar_vals[k, :]                           (AR model, MAP only, :150-153)
//   sampling:  g ~ logGamma(concs) independently, log_probs = g - logsumexp_b g   (:176-178)
//              = the log of a Dirichlet(concs) draw, taken in log space so that tiny
//              concentrations do not underflow (the point of log_gamma.py)
//   MAP:       log_probs = log(concs / sum_b concs)                               (:174-175)
// written in the reference's output='numpy' layout [k-mer, letter, model, mc_sample] (:181-183), for rows of 5 letters
// (dna / rna) or 21 (protein: 20 letters + stop).
//
// The reference draws from numpy's global Mersenne twister by vectorised rejection rounds; a GPU has no
// such stream.  Here every draw is a pure function of (seed, model, sample, global row, letter):
// Marsaglia-Tsang squeeze-free rejection for shape >= 1 evaluated in log space, and for shape a < 1 the
// boost  log G_a = log G_{a+1} + log(U) / a,  which is exact and, like the reference's scheme, never forms
// exp() of a large negative number.  Same distribution as the reference (tests: the reference's own KS
// criterion and its closed-form Beta expectations); the oracle restates this hash sampler bit for bit.
#pragma once
#include "sample_common.h"   // smp_log_gamma, smp_cell_key: the draw and its keys (shared with kernels_generate.h)

#define SMP_THREADS 256
#define SMP_MAX_MODELS 64

struct smp_args {
  int n_h, n_van, arm, has_counts, has_prior, map;
  uint32_t mc;
  uint64_t seed, row_base;
  double w[SMP_MAX_MODELS];   // [0, n_h): 1 / h_j ; [n_h, n_h + n_van): van_k
};

// log_gamma.log_gamma(concs, size): out[s * n + i] = logGamma(conc[i]) draw, s < n_samples
__global__ __launch_bounds__(SMP_THREADS) void log_gamma_kernel(const double *__restrict__ conc, uint64_t n,
                                                                uint64_t n_samples, uint64_t seed,
                                                                double *__restrict__ out) {
  const uint64_t total = n * n_samples;
  for (uint64_t e = (uint64_t)blockIdx.x * SMP_THREADS + threadIdx.x; e < total; e += (uint64_t)gridDim.x * SMP_THREADS) {
    const uint64_t s = e / n, i = e - s * n;
    out[e] = smp_log_gamma(conc[i], smp_cell_key(seed, 0u, s, i));
  }
}

// sum of a[0..N) in a fixed pairwise order: the largest power of two below N first, then the rest.  N = 5 gives
// ((a0 + a1) + (a2 + a3)) + a4, the order of the 5-wide MAP table.  (H is a constexpr variable: called in place as a
// function argument, smp_pow2_below stayed an out-of-line call, whose stack frame cost 56 VGPRs and 16 B of scratch.)
__host__ __device__ constexpr int smp_pow2_below(int n) { return n <= 2 ? 1 : 2 * smp_pow2_below((n + 1) / 2); }
template <int N>
__device__ __forceinline__ double smp_sum(const double *a) {
  constexpr int H = smp_pow2_below(N);
  if constexpr (N == 1) return a[0];
  else return smp_sum<H>(a) + smp_sum<N - H>(a + H);
}

// g[b] = v with b known only at run time, as W compile-time-indexed selects: g stays in registers when the loop around it is
// not unrolled (W = 21), where g[b] itself would put the array in scratch
template <int W>
__device__ __forceinline__ void smp_set(double (&g)[W], int b, double v) {
#pragma unroll
  for (int c = 0; c < W; ++c) g[c] = c == b ? v : g[c];
}

// one thread per (row, model, sample) of rows W wide (5: dna / rna, 21: protein): W draws, normalise, W strided stores
// (consecutive lanes = consecutive samples).  Per element the arithmetic is the same at every W: the concentrations, then
// either W draws, their max, sum exp(g - max) in letter order and g - lse, or the MAP table log(a / sum a).  The key of a
// draw is (seed, model, sample, (row_base + row) * W + letter), so any cut of the rows gives the same table.
// Registers (gfx950, -O3): W = 5 unrolls the draw loop and reads a[b] from registers, 115 VGPRs, 4 waves per SIMD, as the
// 5-wide kernel before it; W = 21 does not unroll it (21 inlined samplers), so a draw forms its concentration again from
// the two loads and stores through smp_set: 169 VGPRs, 2 waves per SIMD, no scratch (a[b] or g[b] at a run-time b: 352 B).
template <int W>
__global__ __launch_bounds__(SMP_THREADS) void logdir_sample_kernel(const uint32_t *__restrict__ counts,
                                                                    const double *__restrict__ prior, uint64_t n_rows,
                                                                    smp_args A, double *__restrict__ out) {
  const uint32_t M = (uint32_t)(A.arm + A.n_h + A.n_van);
  const uint64_t per_row = (uint64_t)M * A.mc;
  const uint64_t total = n_rows * per_row;
  for (uint64_t e = (uint64_t)blockIdx.x * SMP_THREADS + threadIdx.x; e < total; e += (uint64_t)gridDim.x * SMP_THREADS) {
    const uint64_t k = e / per_row;
    const uint32_t rem = (uint32_t)(e - k * per_row);
    const uint32_t m = rem / A.mc, s = rem - m * A.mc;
    const int j = (int)m - A.arm;           // -1: the AR model; [0, n_h): BEAR; then vanilla
    auto conc = [&](int b) {
      const double cnt = A.has_counts ? (double)counts[k * W + b] : 0.0;
      const double f = A.has_prior ? prior[k * W + b] : 0.0;
      return j < 0 ? f : (j < A.n_h ? __builtin_fma(f, A.w[j], cnt) : A.w[j] + cnt);
    };
    double a[W];
#pragma unroll
    for (int b = 0; b < W; ++b) a[b] = conc(b);
    double g[W];
    if (A.map) {
      const double tot = smp_sum<W>(a);
#pragma unroll
      for (int b = 0; b < W; ++b) g[b] = log(a[b] / tot);
    } else {
      const uint64_t grow = A.row_base + k;
      double mx = -INFINITY;
#pragma unroll
      for (int b = 0; b < W; ++b) g[b] = 0.0;
#pragma unroll
      for (int b = 0; b < W; ++b) {
        const double v = smp_log_gamma(W <= 8 ? a[b] : conc(b), smp_cell_key(A.seed, m, s, grow * W + b));
        smp_set<W>(g, b, v);
        mx = v > mx ? v : mx;
      }
      double se = 0.0;
#pragma unroll
      for (int b = 0; b < W; ++b) se += exp(g[b] - mx);
      const double lse = mx + log(se);
#pragma unroll
      for (int b = 0; b < W; ++b) g[b] -= lse;
    }
#pragma unroll
    for (int b = 0; b < W; ++b) out[((k * W + b) * M + m) * A.mc + s] = g[b];
  }
}
