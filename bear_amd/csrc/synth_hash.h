// synth_hash.h -- the counter-based hash and the variates drawn from it (synthetic tables, evaluation noise, samplers,
// the row shuffle).  No kernels.
#pragma once
#include "bear_common.h"

// ------------------------------------------------------------------ synthetic table
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ double u01(uint64_t h) { return ((double)(h >> 11) + 0.5) * (1.0 / 9007199254740992.0); }
__device__ __forceinline__ double gauss(uint64_t k) {
  return sqrt(-2.0 * log(u01(mix64(k)))) * cos(6.283185307179586 * u01(mix64(k ^ 0x5851F42D4C957F2Dull)));
}
__device__ uint32_t poisson(double mu, uint64_t k) {
  if (!(mu > 0.0)) return 0u;
  if (mu < 12.0) {
    double u = u01(mix64(k)), p = exp(-mu), s = p;
    uint32_t n = 0;
    while (u > s && n < 200u) {
      ++n;
      p *= mu / (double)n;
      s += p;
    }
    return n;
  }
  double v = floor(mu + sqrt(mu) * gauss(k) + 0.5);
  return v > 0.0 ? (v < 4.0e9 ? (uint32_t)v : 4000000000u) : 0u;
}
