// kernels_ksample.h -- bear_k_sample_f64: the Bayes factors among G = 2..16 count columns of one table in one pass over its rows:
// per model and group M_g = sum_k T(c_g), per pair (g, g') the pooled M_gg' = sum_k T(c_g + c_g') and B_gg' = sum_k [(T(c_g) +
// T(c_g')) - T(c_g + c_g')], over all groups M_all = sum_k T(sum_g c_g) and B_all = sum_k [(sum_g T(c_g)) - T(sum_g c_g)], every
// bracket formed PER ROW; with prior rows the AR model's L_g = sum_k sum_j c_gj log prior[k, j].  T, the models and the item
// routine are kernels_twosample.h's; a column is read once and T(c_g) evaluated once, whatever G.
//
//   tile   = KS_TILE(W, GP) contexts, GP = G rounded up to 2, 4, 8, 16: every column's count rows (flat 16-byte lane loads, four in
//            flight a thread) and the prior row into LDS.  The tile shrinks as GP grows -- 128, 64, 48, 24 contexts at W = 21 and
//            256, 128, 96, 48 at W = 5 for GP = 2, 4, 8, 16 -- so that every instantiation stays below 64 KiB (sixteen staged
//            columns of width 21 are 1344 B a context, 2248 B with what phase 1 leaves): TWO blocks per CU of the 160 KiB
//            (KS_BLOCKS_PER_CU), two waves a SIMD, up to 256 VGPRs.
//   phase 1  a thread per (context, group), group = thread % GP for the whole launch: the mask of its non-zero cells, n_g and, per
//            model, T(c_g) into LDS; T(c_g) and the AR term into the thread's accumulators of ITS group.
//   phase 2  a thread per slot = thread % KS_SLOTS(GP) for the whole launch: slot p < P is pair p, slot P is "all groups"; the
//            threads of one slot split the tile's contexts (thread / slots, in steps of 256 / slots).  A slot is a list of groups
//            (first, last, step) and both kinds run ONE code path, so the lanes of a wave make their item calls together.  At most
//            one non-empty group in the list: the pooled row is that group's T from LDS (the sum with the others' +0.0) and the
//            bracket +0.0: no item.  Otherwise the pooled row is -D(S, sum n_g) and one item per cell of the union, on the exact
//            integer sum of the counts (below 2^33 of a pair, 2^36 of sixteen, a row total below 2^41), and the bracket is the sum
//            of the T(c_g) in group order less it.  The all-groups slot also writes row_terms.
//   sums   = no atomics: each accumulator goes through LDS, a thread per group / slot adds the block's values in thread order ->
//            block partial (KS_NPART(GP) doubles in the CALLER's scratch) -> k_sample_finalize_kernel's fixed-order sum over the
//            blocks.  Equal bits for equal inputs, n_rows and G, in both libraries.
//   models = at most KS_CHUNK per launch; more are further launches, each with the bits of a call of its own.
#pragma once
#include "bear_common.h"
#include "kernels_eval.h"        // evs_item_D
#include "kernels_rows.h"        // stage_dwords
#include "kernels_twosample.h"   // ts_log_prior
#include "rows_wide_common.h"    // wide_nz_mask

#define KS_THREADS 256
#define KS_BLOCKS_PER_CU 2
#define KS_CHUNK 4
#define KS_MAX_BLOCKS 1024                                   // of any launch: the scratch query does not depend on the device
#define KS_TILE(W, GP) \
  ((W) > 8 ? ((GP) == 2 ? 128 : (GP) == 4 ? 64 : (GP) == 8 ? 48 : 24) : ((GP) == 2 ? 256 : (GP) == 4 ? 128 : (GP) == 8 ? 96 : 48))
#define KS_SLOTS(GP) ((GP) == 2 ? 2 : (GP) == 4 ? 8 : (GP) == 8 ? 32 : 128)      // >= GP (GP - 1) / 2 + 1, a divisor of KS_THREADS
// block partial: {T[chunk], L}[GP] by group, then {M, B}[chunk][slots] by slot
#define KS_NPART(GP) ((KS_CHUNK + 1) * (GP) + 2 * KS_CHUNK * KS_SLOTS(GP))

struct ks_args {
  double w[BEAR_TWO_SAMPLE_MAX_MODELS];        // [0, n_h): 1 / h_m; [n_h, n_models): van
  uint64_t col[BEAR_K_SAMPLE_MAX_GROUPS];      // the first row of every column
  int n_h, n_models, n_groups;
};

// one accumulator of every thread -> the sums over the threads with equal (thread % N), added in thread order, into dst[0 .. N)
template <int N>
__device__ __forceinline__ void ks_fold(double v, double *s_red, double *dst) {
  const uint32_t tid = threadIdx.x;
  __syncthreads();
  s_red[tid] = v;
  __syncthreads();
  if (tid < (uint32_t)N) {
    double s = 0.0;
    for (int q = 0; q < KS_THREADS / N; ++q) s += s_red[q * N + tid];
    dst[tid] = s;
  }
}

// 16-byte piece i of the flat stream of a tile's G columns (nv pieces a column): where it comes from, where it goes
template <int W>
__device__ __forceinline__ const uint4 *ks_src(const uint32_t *counts, const uint64_t *s_col, uint64_t row0, uint32_t nv, uint32_t i) {
  const uint32_t g = i / nv;
  return reinterpret_cast<const uint4 *>(counts + (s_col[g] + row0) * W) + (i - g * nv);
}
template <int TW>
__device__ __forceinline__ uint4 *ks_dst(uint32_t *s_cnt, uint32_t nv, uint32_t i) {
  const uint32_t g = i / nv;
  return reinterpret_cast<uint4 *>(s_cnt + g * TW) + (i - g * nv);
}

template <int W, int GP>
__global__ __launch_bounds__(KS_THREADS, KS_BLOCKS_PER_CU) void k_sample_kernel(const uint32_t *__restrict__ counts,
                                                                               const double *__restrict__ prior, uint64_t n_rows,
                                                                               ks_args A, int m0, int m_cnt, int use_prior, int do_ar,
                                                                               const double2 *__restrict__ logtab_g,
                                                                               double *__restrict__ partials,
                                                                               double *__restrict__ row_terms) {
  static_assert(W <= 32, "the non-zero cells of a row are a 32-bit mask");
  constexpr int T = KS_TILE(W, GP), TW = T * W, SL = KS_SLOTS(GP), RL = KS_THREADS / SL, R1 = KS_THREADS / GP;
  static_assert(TW % 4 == 0, "a tile of a column starts on a 16-byte boundary");
  __shared__ __attribute__((aligned(16))) uint32_t s_cnt[GP * TW];
  __shared__ __attribute__((aligned(16))) double s_pri[TW];
  __shared__ double s_T[KS_CHUNK][T * GP];
  __shared__ double s_n[T * GP];
  __shared__ uint32_t s_z[T * GP];
  __shared__ double s_S[KS_CHUNK][T];
  __shared__ double2 s_log[BEAR_LOGTAB_N];
  __shared__ double s_red[KS_THREADS];
  __shared__ uint64_t s_col[GP];
  const uint32_t tid = threadIdx.x;
  const int G = A.n_groups, P = G * (G - 1) / 2;
  if (tid < BEAR_LOGTAB_N) s_log[tid] = logtab_g[tid];
#pragma unroll
  for (int g = 0; g < GP; ++g)
    if (tid == (uint32_t)g) s_col[g] = g < G ? A.col[g] : 0;
  // phase 1: this thread's group and first context; phase 2: its slot (a pair, or all groups) and first context
  const int g1 = (int)(tid % GP);
  const uint32_t r1 = tid / GP;
  const int slot = (int)(tid % SL);
  const uint32_t q2 = tid / SL;
  int g_first = 0, g_last = G - 1, g_step = 1;      // the groups of the slot: all of them, or the two of pair `slot`
  if (slot < P) {
    int p = slot;
    while (p >= G - 1 - g_first) {
      p -= G - 1 - g_first;
      ++g_first;
    }
    g_last = g_first + 1 + p;
    g_step = g_last - g_first;
  }
  double acc_g[KS_CHUNK], acc_m[KS_CHUNK], acc_b[KS_CHUNK], acc_l = 0.0;
#pragma unroll
  for (int k = 0; k < KS_CHUNK; ++k) acc_g[k] = acc_m[k] = acc_b[k] = 0.0;
  const uint64_t n_tiles = (n_rows + T - 1) / T;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t row0 = tile * T;
    const uint32_t rows = (uint32_t)((n_rows - row0 < (uint64_t)T) ? (n_rows - row0) : (uint64_t)T);
    __syncthreads();  // previous tile consumed (and the log table, the column starts are in place)
    // ---- the G column tiles as one flat stream of 16-byte loads, four in flight a thread
    const uint32_t nd = rows * W, nv = nd >> 2, total = (uint32_t)G * nv;
    for (uint32_t i0 = tid; i0 < total; i0 += 4 * KS_THREADS) {
      const uint32_t i1 = i0 + KS_THREADS, i2 = i1 + KS_THREADS, i3 = i2 + KS_THREADS;
      // (a piece beyond the stream re-reads piece i0: a valid address, never stored)
      const uint4 v0 = *ks_src<W>(counts, s_col, row0, nv, i0), v1 = *ks_src<W>(counts, s_col, row0, nv, i1 < total ? i1 : i0),
                  v2 = *ks_src<W>(counts, s_col, row0, nv, i2 < total ? i2 : i0), v3 = *ks_src<W>(counts, s_col, row0, nv, i3 < total ? i3 : i0);
      *ks_dst<TW>(s_cnt, nv, i0) = v0;
      if (i1 < total) *ks_dst<TW>(s_cnt, nv, i1) = v1;
      if (i2 < total) *ks_dst<TW>(s_cnt, nv, i2) = v2;
      if (i3 < total) *ks_dst<TW>(s_cnt, nv, i3) = v3;
    }
    if (nd & 3u)     // (the last tile only)
      for (int g = 0; g < G; ++g)
        for (uint32_t i = (nv << 2) + tid; i < nd; i += KS_THREADS) s_cnt[g * TW + i] = counts[(s_col[g] + row0) * W + i];
    if (use_prior)
      stage_dwords<KS_THREADS>(reinterpret_cast<uint32_t *>(s_pri), reinterpret_cast<const uint32_t *>(prior + row0 * W), nd * 2);
    __syncthreads();
    // ---- phase 1: (context, group) -> mask, n_g, T(c_g) per model
    if (g1 < G) {
#pragma unroll 1
      for (uint32_t r = r1; r < rows; r += R1) {
        const uint32_t *c = s_cnt + g1 * TW + r * W;
        const double *f = s_pri + r * W;
        const uint32_t idx = r * GP + g1, z = wide_nz_mask<W>(c);
        s_z[idx] = z;
        if (!z) {          // no transition of this group: +0.0 everywhere, no item
          s_n[idx] = 0.0;
          for (int mi = 0; mi < m_cnt; ++mi) s_T[mi][idx] = 0.0;
          continue;
        }
        double n = 0.0;
#pragma unroll
        for (int j = 0; j < W; ++j) n += (double)c[j];
        s_n[idx] = n;
        if (do_ar) {
          double l = 0.0;
          for (uint32_t nz = z; nz;) {
            const int j = __builtin_ctz(nz);
            nz &= nz - 1u;
            l = __builtin_fma((double)c[j], ts_log_prior(f[j], s_log), l);
          }
          acc_l += l;
        }
#pragma unroll 1
        for (int mi = 0; mi < m_cnt; ++mi) {
          const int m = m0 + mi;
          const double w = A.w[m];
          const bool ear = m < A.n_h;
          double S = 0.0;
#pragma unroll
          for (int j = 0; j < W; ++j) S += ear ? f[j] * w : w;
          double t = -evs_item_D(S, n, s_log);
          for (uint32_t nz = z; nz;) {
            const int j = __builtin_ctz(nz);
            nz &= nz - 1u;
            t += evs_item_D(ear ? f[j] * w : w, (double)c[j], s_log);
          }
          s_T[mi][idx] = t;
          s_S[mi][r] = S;       // (every non-empty group of the context writes the same bits)
#pragma unroll
          for (int k = 0; k < KS_CHUNK; ++k)
            if (k == mi) acc_g[k] += t;
        }
      }
    }
    __syncthreads();
    // ---- phase 2: this thread's groups (a pair, or all of them) over its contexts of the tile -- ONE path for both kinds of slot:
    // the lanes of a wave run the item calls together (two branches would run one after the other)
    if (slot <= P) {
#pragma unroll 1
      for (uint32_t r = q2; r < rows; r += RL) {
        uint32_t zu = 0u;
        int ne = 0;
        double ntot = 0.0;
        for (int g = g_first; g <= g_last; g += g_step) {
          const uint32_t z = s_z[r * GP + g];
          zu |= z;
          ne += z ? 1 : 0;
          ntot += s_n[r * GP + g];
        }
        double *rt = (row_terms && slot == P) ? row_terms + (row0 + r) * (uint64_t)A.n_models + (uint64_t)m0 : nullptr;
        if (!zu) {
          if (rt)
            for (int mi = 0; mi < m_cnt; ++mi) rt[mi] = 0.0;
          continue;
        }
        const double *f = s_pri + r * W;
#pragma unroll 1
        for (int mi = 0; mi < m_cnt; ++mi) {
          double sum_t = 0.0;       // T(c_g) of the groups in their order (+0.0 of an empty one changes no bit)
          for (int g = g_first; g <= g_last; g += g_step) sum_t += s_T[mi][r * GP + g];
          double pooled = sum_t, bk = 0.0;     // one non-empty group: the pooled row IS its row, and no item
          if (ne > 1) {
            const int m = m0 + mi;
            const double w = A.w[m];
            const bool ear = m < A.n_h;
            pooled = -evs_item_D(s_S[mi][r], ntot, s_log);
            for (uint32_t nz = zu; nz;) {
              const int j = __builtin_ctz(nz);
              nz &= nz - 1u;
              double cj = 0.0;      // exact: below 2^33 of a pair, 2^36 of sixteen
              for (int g = g_first; g <= g_last; g += g_step) cj += (double)s_cnt[g * TW + r * W + j];
              pooled += evs_item_D(ear ? f[j] * w : w, cj, s_log);
            }
            bk = sum_t - pooled;
          }
          if (rt) rt[mi] = bk;
#pragma unroll
          for (int k = 0; k < KS_CHUNK; ++k)
            if (k == mi) {
              acc_m[k] += pooled;
              acc_b[k] += bk;
            }
        }
      }
    }
  }
  // ---- block partial: every accumulator through LDS, added in thread order
  double *part = partials + (size_t)blockIdx.x * KS_NPART(GP);
#pragma unroll
  for (int k = 0; k < KS_CHUNK; ++k) ks_fold<GP>(acc_g[k], s_red, part + k * GP);
  ks_fold<GP>(acc_l, s_red, part + KS_CHUNK * GP);
#pragma unroll
  for (int k = 0; k < KS_CHUNK; ++k) {
    ks_fold<SL>(acc_m[k], s_red, part + (KS_CHUNK + 1) * GP + (2 * k) * SL);
    ks_fold<SL>(acc_b[k], s_red, part + (KS_CHUNK + 1) * GP + (2 * k + 1) * SL);
  }
}

// The fixed-order sum over the blocks of value v of the block partial, one wave per value, to where it belongs: out_group[m, G],
// out_ar[G] (out_ar != NULL: the launch that carried it), out_pair[m, P, 2], out_all[m, 2]
__global__ __launch_bounds__(256) void k_sample_finalize_kernel(const double *__restrict__ partials, int n_blocks, int gp, int sl, int G,
                                                               int m0, int m_cnt, double *__restrict__ out_group,
                                                               double *__restrict__ out_pair, double *__restrict__ out_all,
                                                               double *__restrict__ out_ar) {
  const int lane = threadIdx.x & 63, v = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n_part = (KS_CHUNK + 1) * gp + 2 * KS_CHUNK * sl, P = G * (G - 1) / 2;
  if (v >= n_part) return;
  double *dst = nullptr;
  if (v < KS_CHUNK * gp) {
    const int mi = v / gp, g = v % gp;
    if (mi < m_cnt && g < G) dst = out_group + (size_t)(m0 + mi) * G + g;
  } else if (v < (KS_CHUNK + 1) * gp) {
    const int g = v - KS_CHUNK * gp;
    if (out_ar && g < G) dst = out_ar + g;
  } else {
    const int u = v - (KS_CHUNK + 1) * gp, k = u / sl, s = u % sl, mi = k >> 1;
    if (mi < m_cnt && s < P) dst = out_pair + ((size_t)(m0 + mi) * P + s) * 2 + (k & 1);
    else if (mi < m_cnt && s == P) dst = out_all + (size_t)(m0 + mi) * 2 + (k & 1);
  }
  if (!dst) return;
  double s = 0.0;
  for (int blk = lane; blk < n_blocks; blk += 64) s += partials[(size_t)blk * n_part + v];
  s = bear_wave_sum(s);
  if (lane == 0) *dst = s;
}
