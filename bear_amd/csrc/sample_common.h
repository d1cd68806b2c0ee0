// sample_common.h -- the counter-based log-Gamma draw and its keys, shared by the units that sample: kernels_sample.h (the
// posterior tables, bear_hip.hip) and kernels_generate.h (sequence generation, bear_score.hip).  No kernels.
#pragma once
#include "bear_common.h"
#include "synth_hash.h"

#define SMP_MAX_ROUNDS 64   // acceptance >= 0.95 per round: 64 misses in a row has probability < 1e-83

// one logGamma(a) draw, a > 0, from the counter stream `key`
__device__ __forceinline__ double smp_log_gamma(double a, uint64_t key) {
  const bool small = a < 1.0;
  const double a1 = small ? a + 1.0 : a;
  const double d = a1 - 1.0 / 3.0;
  const double c = 1.0 / sqrt(9.0 * d);
  const double ld = log(d);
  double lg = ld;
  for (uint32_t t = 0; t < SMP_MAX_ROUNDS; ++t) {
    const double x = gauss(key + 2ull * t + 1ull);
    const double u = u01(mix64(key + 2ull * t + 2ull));
    const double w = __builtin_fma(c, x, 1.0);
    if (w <= 0.0) continue;
    const double v = w * w * w;
    const double lv = log(v);
    lg = ld + lv;
    if (log(u) < __builtin_fma(0.5 * x, x, d) - d * v + d * lv) break;
  }
  if (small) lg += log(u01(mix64(key))) / a;
  return lg;
}

__device__ __forceinline__ uint64_t smp_cell_key(uint64_t seed, uint32_t model, uint64_t sample, uint64_t cell) {
  return mix64(mix64(mix64(seed + (uint64_t)model) + sample) ^ cell);
}
