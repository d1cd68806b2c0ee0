// kernels_finalize.h -- the fixed-order sum of block partials as a launch of its own (the kernels that are not handed a
// bear_step_io; bear_finalize_in_block, bear_common.h, is the same arithmetic inside the producing launch).
#pragma once
#include "bear_common.h"

// ------------------------------------------------------------------ finalize: fixed-order sum of block partials
__global__ __launch_bounds__(256) void finalize_kernel(const double *__restrict__ partials, int n_blocks,
                                                       int n_out, double *__restrict__ out) {
  __shared__ double red[4][BEAR_MAX_OUT];
  double acc[BEAR_MAX_OUT] = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < n_blocks; b += 256)
#pragma unroll
    for (int k = 0; k < BEAR_MAX_OUT; ++k)
      if (k < n_out) acc[k] += partials[(size_t)b * BEAR_MAX_OUT + k];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < BEAR_MAX_OUT; ++k) {
    double v = bear_wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < n_out) out[threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

