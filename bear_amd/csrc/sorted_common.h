// sorted_common.h -- constants and device helpers of the sorted-work-item formulation (kernels_sorted.h), shared with the
// planned kernels.  No kernels.
#pragma once
#include "bear_common.h"

#define SRT_THREADS 512
#define SRT_WAVES (SRT_THREADS / 64)
#define SRT_TILE 512
#define SRT_NKEY 32  // key = min(c, 32) - 1
#define SRT_REP 8
#define SRT_NHIST (SRT_NKEY * SRT_REP)
#ifndef SRT_CL
#define SRT_CL 24
#endif
// product path for c <= SRT_CL (keys 0 .. SRT_CL-1), Stirling path above
#define SRT_XMAX 0x1p30  // products of <= 31 factors stay finite below this
#define SRT_ILP 2        // light items evaluated per lane per step (independent dependency chains)
#define SRT_UNIT (64 * SRT_ILP)
#define SRT_SUM1_TOL 4.5e-16  // |sum(prior row) - 1| below which A = u + 5 eps is shared (2 ulp)

static_assert(SRT_TILE == SRT_THREADS, "phase A maps one context to one thread");
static_assert((SRT_TILE * 20) % 1024 == 0 && (SRT_TILE * 40) % 1024 == 0, "tiles are whole 1 KiB DMA pieces");

// ---- shared pieces ----------------------------------------------------------------------
__device__ __forceinline__ uint32_t srt_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t srt_key(uint32_t c) { return (c > SRT_NKEY ? SRT_NKEY : c) - 1; }  // c >= 1

// Workgroup barrier that makes prior LDS traffic of every wave visible but leaves vector-memory
// (LDS-DMA) operations in flight -- __syncthreads() would wait for vmcnt(0) as well.
__device__ __forceinline__ void srt_sync() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void srt_wait_dma() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Synchronous, guarded staging (ragged last tile): 16-byte lane loads, dword tail.
__device__ __forceinline__ void srt_stage(uint32_t *lds, const uint32_t *src, uint32_t n_dwords) {
  const uint32_t n_vec = n_dwords >> 2;
  const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
  uint4 *d4 = reinterpret_cast<uint4 *>(lds);
  for (uint32_t i = threadIdx.x; i < n_vec; i += SRT_THREADS) d4[i] = s4[i];
  for (uint32_t i = (n_vec << 2) + threadIdx.x; i < n_dwords; i += SRT_THREADS) lds[i] = src[i];
}

// Asynchronous staging of a whole tile slab (`bytes` a multiple of 1 KiB): wave w moves pieces
// w, w + 8, ...; each piece is one global_load_lds_dwordx4 (lane l: 16 B at +16 l, LDS address
// M0 + 16 l, contiguous).  Issued from inline asm on purpose: through the builtin the compiler
// assumes every later LDS access may alias the in-flight DMA and puts s_waitcnt vmcnt(0) in front
// of it, which serialises the prefetch with the evaluation of the current tile.  Ordering is
// explicit instead: srt_wait_dma() + srt_sync() at the top of the next iteration.
__device__ __forceinline__ void srt_dma(void *lds, const void *src, uint32_t bytes, uint32_t wave, uint32_t lane) {
  const uint32_t d = (uint32_t)(uintptr_t)lds;  // LDS byte address (low 32 bits of the generic pointer)
  const unsigned char *s = static_cast<const unsigned char *>(src) + lane * 16u;
  for (uint32_t piece = wave; piece < (bytes >> 10); piece += SRT_WAVES) {
    const unsigned char *g = s + (piece << 10);
    const uint32_t m = srt_uniform(d + (piece << 10));
    {
      // M0 is compiler-reserved: saved and restored inside the statement that uses it (no "m0" clobber: that is undefined behaviour)
      uint32_t keep_m0;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep_m0)
                   : "v"(g), "s"(m)
                   : "memory");
    }
  }
}

// Exclusive scan of one uint32 per thread over the block.  `scratch` holds SRT_WAVES words.
__device__ __forceinline__ uint32_t srt_block_exscan(uint32_t v, uint32_t *scratch, uint32_t *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    uint32_t o = (uint32_t)__shfl_up((int)incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) scratch[wave] = incl;
  srt_sync();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < SRT_WAVES; ++w) {
    uint32_t t = scratch[w];
    if (w < wave) base += t;
    tot += t;
  }
  *total = tot;
  return base + incl - v;
}

// The general routine, kept out of line so the hot loops stay small (registers, I-cache).
__device__ __noinline__ bear_dp srt_general(double x, double c) {
  if (!(x > 0.0)) return bear_dp{__builtin_nan(""), __builtin_nan("")};
  return bear_dm_item(x, c);
}
// The same on the table log (LDS or global table): ~3x fewer instructions.
// `used`: the routine stays the one written here in every unit that includes it.  Left internal, the compiler re-specialises it
// per unit to the address space its callers there happen to pass for `tab` (all LDS in one unit, LDS and global in another), and
// the kernels around the call change with it: the same kernel would differ from unit to unit (scripts/dev/kernel_table.py).
__device__ __noinline__ __attribute__((used)) bear_dp srt_general_fast(double x, double c, const double2 *tab);
// the table-log form wherever its argument is in that routine's domain (x > 0 and finite), the library form elsewhere: the heavy
// items of the UNPLANNED sorted kernels (round 6: they had kept the ~500-instruction form; a dense table ran 2.24 ms per 2e7 contexts)
__device__ __forceinline__ bear_dp srt_general_auto(double x, double c, const double2 *tab) {
  return x > 0.0 && x < INFINITY ? srt_general_fast(x, c, tab) : srt_general(x, c);
}
__device__ __noinline__ bear_dp srt_general_fast(double x, double c, const double2 *tab) {
  if (!(x > 0.0) || !(x < 0x1p1000)) return bear_dp{__builtin_nan(""), __builtin_nan("")};
  return bear_dm_item_fast(x, c, tab);
}

// Product-path evaluation of ILP light items per lane: D = log prod_{j<c}(x+j), P = sum 1/(x+j).
// Every lane runs `cmin` un-predicated factors (wave-uniform lower bound of the occupied lanes'
// counts; unoccupied lanes carry c == 0 and a harmless x), then the ragged remainder up to `cmax`
// under predication.  c == 0 yields D = P = 0.
// `in_domain` (wave-uniform): the CALLER guarantees 0 < x <= SRT_XMAX for every occupied lane (the linear step: x = f u + eps with
// f a softmax output it formed itself), so the per-unit domain test -- eight vector instructions of a unit's ~95 -- is skipped.
template <int ILP, bool COEF_V = false>      // (COEF_V: bear_log1p_small)
__device__ __forceinline__ void srt_light(const double (&x)[ILP], const uint32_t (&c)[ILP], uint32_t cmin, uint32_t cmax,
                                          const double2 *logtab, bear_dp (&o)[ILP], bool in_domain = false) {
  double p[ILP], dp[ILP], t[ILP];
#pragma unroll
  for (int i = 0; i < ILP; ++i) {
    p[i] = 1.0;
    dp[i] = 0.0;
    t[i] = x[i];
  }
  // One factor: dp = dp t + p, p = p t, t = t + 1 -- three VOP3 instructions, spelled out: left to itself the compiler forms the
  // first as v_fmac (accumulator = a COPY of p) and shuffles the pairs around it, five instructions per factor instead of three;
  // under predication it turned the three results into six v_cndmask instead of masking the lanes (-ffp-contract=off: the same
  // three roundings either way).
#define SRT_FACTOR(dp, p, t) \
  asm("v_fma_f64 %0, %0, %2, %1\n\tv_mul_f64 %1, %1, %2\n\tv_add_f64 %2, %2, 1.0" : "+v"(dp), "+v"(p), "+v"(t))
  uint32_t j = 0;
  for (; j < cmin; ++j) {
#pragma unroll
    for (int i = 0; i < ILP; ++i) SRT_FACTOR(dp[i], p[i], t[i]);
  }
  for (; j < cmax; ++j) {
#pragma unroll
    for (int i = 0; i < ILP; ++i) {
      if (j < c[i]) SRT_FACTOR(dp[i], p[i], t[i]);
    }
  }
#undef SRT_FACTOR
  bool odd = false;
#pragma unroll
  for (int i = 0; i < ILP; ++i) {
    const bool live = c[i] != 0;
    o[i].D = live ? bear_log_tab<COEF_V>(p[i], logtab) : 0.0;
    o[i].P = live ? dp[i] * bear_rcp(p[i]) : 0.0;
    if (!in_domain) odd |= live && !(x[i] > 0.0 && x[i] <= SRT_XMAX);
  }
  // Out-of-domain / out-of-range arguments take the general routine (rare, wave-uniform test).
  if (!in_domain && __builtin_amdgcn_ballot_w64(odd)) {
#pragma unroll
    for (int i = 0; i < ILP; ++i)
      if (c[i] != 0 && !(x[i] > 0.0 && x[i] <= SRT_XMAX)) o[i] = srt_general(x[i], (double)c[i]);
  }
}

// Smallest / largest count of a unit of ascending-sorted items [base, min(base + SRT_UNIT, end)):
// the first lane of the first slice and the last occupied lane of the last occupied slice.
__device__ __forceinline__ void srt_unit_range(const uint32_t (&c)[SRT_ILP], uint32_t base, uint32_t end, uint32_t *cmin,
                                               uint32_t *cmax) {
  uint32_t cm = 0;
#pragma unroll
  for (int i = 0; i < SRT_ILP; ++i) {
    const uint32_t lo = base + 64u * i;
    if (end > lo) {
      const uint32_t n = end - lo > 64u ? 64u : end - lo;
      const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)c[i], (int)(n - 1u));
      cm = v > cm ? v : cm;
    }
  }
  *cmax = cm;
  // un-predicated factors are only safe when every lane of every slice is occupied
  *cmin = end - base >= SRT_UNIT ? (uint32_t)__builtin_amdgcn_readlane((int)c[0], 0) : 0u;
}
