// kernels_generate.h -- sequence generation on the device (assemble.assemble_no_ends and assemble.generate_sequences with a
// DeviceCounter): every sequence grows letter by letter from its end k-mer, the transition table row of that k-mer is looked up in
// the sorted key table of a column and sampled (or taken at its MAP value) where it is needed, and the letter is a Gumbel-max draw
// over the row.
//
// The host loop of assemble.py keeps "one posterior sample of the transition table per generated sequence" (assemble.py:126) as an
// array, because it cannot draw the same row again later.  Here a table value is a pure function of (seed, sequence's sample index,
// k-mer key, letter): a sequence that returns to a k-mer forms the same row again, and nothing is stored.
//
// ONE body, gen_run<BITS, W, STOP, Ref...>, under three kernels.  generate_steps_kernel (STOP = false) grows flanks of given lengths and never
// draws the stop: the NL = W - 1 letters take part.  generate_whole_kernel (STOP = true) draws over all NL = W letters -- the stop
// b = W - 1 is a letter like the others (same two streams, so a cell b < W - 1 holds bit for bit the value it holds without the
// stop) -- and a sequence ends when it wins (assemble.generate_sequences).  generate_whole_ref_kernel (STOP and REF) is that kernel
// under a bear_ref model: the AR function's row of the end k-mer is the reference-mixed row of kernels_refscore.h, formed inside
// the step from the k-mer's row in a second key table, the reference column's.
//
// Lane mapping: the letters of one sequence sit on neighbouring lanes, GEN_GROUP(NL) lanes per sequence -- 4 and 8 at W = 5 (every
// lane a letter; three lanes of the 8 only take part in the exchange), 32 at W = 21.  Per step the first lane of a group finds the
// row (scr_find_row) and hands it round, every letter lane forms ONE concentration, ONE log-Gamma draw and ONE Gumbel draw, and the
// arg-max is log2(group) lane exchanges of (value, letter).  A sequence per lane would run W - 1 rejection samplers one behind the
// other (and hold them all in registers: the 169 VGPRs of logdir_sample_kernel<21>).
// No atomics and no sum across lanes: the letters are the same in both libraries and for any cut of the steps into launches.
#pragma once
#include "kernels_refscore.h"   // rfs_ref_row, rfs_prior_cell: the reference-mixed row of generate_whole_ref_kernel
#include "kernels_score.h"   // scr_ranks, scr_find_row: keys are those of bear_score_transitions_u64
#include "rows_wide_common.h"   // LNW_W, LNW_MAT, lnw_forward_row: the linear AR function's row inside generate_whole_kernel<5, 21>
#include "sample_common.h"

#define GEN_THREADS 256
#define GEN_ID_GUMBEL 3000u   // the model id of the Gumbel stream (the table values are model 0; beside EVL_ID_ARM / EVL_ID_VAN)
#define GEN_GROUP(NL) ((NL) <= 4 ? 4 : ((NL) <= 8 ? 8 : 32))   // lanes per sequence for NL letter lanes

struct gen_args {
  int lag, mode, map;          // mode: BEAR_GEN_BMM / BEAR_GEN_BEAR / BEAR_GEN_AR (include/bear_hip.h)
  double inv_h, van;
  uint64_t seed, step0, n_steps, stride;
  uint64_t rank[3];            // byte c: the rank of the letter code c < W - 1 (scr_ranks, eight to a word: selected, never indexed)
  uint64_t code[4];            // byte r: the core.encode_kmers code of the rank r
};

// byte i of words held in scalar registers, as selects (indexing the argument block per lane would put it in scratch)
__device__ __forceinline__ uint32_t gen_byte3(const uint64_t (&w)[3], uint32_t i) {
  const uint64_t x = i < 8u ? w[0] : (i < 16u ? w[1] : w[2]);
  return (uint32_t)(x >> ((i & 7u) * 8u)) & 0xFFu;
}
__device__ __forceinline__ uint32_t gen_byte4(const uint64_t (&w)[4], uint32_t i) {
  const uint64_t x = i < 16u ? (i < 8u ? w[0] : w[1]) : (i < 24u ? w[2] : w[3]);
  return (uint32_t)(x >> ((i & 7u) * 8u)) & 0xFFu;
}

// the core.encode_kmers code of letter p (0: the first) of the k-mer with the key q
template <int BITS>
__device__ __forceinline__ int8_t gen_code_at(const gen_args &A, uint64_t q, int p) {
  return (int8_t)gen_byte4(A.code, (uint32_t)(q >> (BITS * (A.lag - 1 - p))) & ((1u << BITS) - 1u));
}

// With mat (W = 21, STOP) every block stages mat, so the grid is capped and strides over the sequences.  Dynamic LDS: exp table |
// a row per group | mat | 16 code bytes per group.
#define GEN_WHOLE_MAT_BLOCKS 512
#define GEN_WHOLE_MAT_LDS(lag) \
  (sizeof(double) * (BEAR_EXPTAB_N + (size_t)(GEN_THREADS / GEN_GROUP(21)) * LNW_W + (size_t)(lag) * LNW_MAT) + \
   (size_t)(GEN_THREADS / GEN_GROUP(21)) * 16)
static_assert(GEN_WHOLE_MAT_LDS(12) <= 64 * 1024, "generate_whole_kernel with mat: LDS");

// Steps step0 .. step0 + n_steps - 1 of every sequence that has steps left (left[i] of them: it takes them until n_steps are done
// or, with STOP, the stop wins, and left[i] goes down by the steps taken).  keys[i]: the end key, read and written.  table /
// counts: the ascending distinct keys of a column and their count rows in that order (an absent k-mer: a row of zeros).
// STOP: when the stop wins stopped[i] = 1, left[i] = 0, nothing is written to letters and the key is not advanced; length[i] counts
// the letters written.  keys, left, length and stopped are the whole state: any cut of the steps into launches that continue at
// step0 gives the same bytes.  Without STOP length, stopped and mat are not read (NULL).
//
// f, the AR function's row of the current end k-mer, is prior: NULL, or [n_seq, W] rows (then n_steps <= 1: the host forms the
// next rows from `codes`) -- or, with STOP at W = 21, formed here from mat [lag, 21, 21]: lnw_forward_row on the LDS image of mat
// and the exp table, the row bear_linear_forward_wide_f64 writes for the same codes ('[' = 20), bit for bit -- whole sequences under a
// trained linear model in one launch.  The group's lanes p < lag put the k-mer's code bytes into LDS, its first lane forms the row
// there, every lane reads its own entry back.  A group lies inside one wave, whose LDS accesses complete in order: the hand-over
// needs no barrier, only that the compiler keeps the order (the wave-scope fences).
// Every loop runs the same number of times on all lanes of a wave (a finished sequence idles), so each exchange finds its group whole.
//
// REF (with STOP): a bear_ref model.  What prior or mat yields -- or, with neither (net 0), the one-hot at the stop -- is the NET
// function's row g, and f_b = rfs_prior_cell(ref row of the end k-mer, b, g_b): the group's first lane finds the row in ref_table
// as it finds the train row and hands both round, every letter lane forms R = rfw_ref_total of that row itself -- the same
// loads in the same order, so all lanes hold the same bits and nothing is summed across lanes -- and then its own cell.
struct gen_ref_args {
  const uint64_t *table;       // the reference column's ascending distinct keys
  const uint32_t *counts;      // ... and their count rows in that order (an absent k-mer: rfs_zero_row)
  uint64_t n_table;
  int net;                     // BEAR_GEN_NET_STOP / _ROWS / _MAT (include/bear_hip.h)
  bear_params prm;             // E, nw, V, eps (host values)
};

// (The reference arguments are a parameter pack -- empty, or one gen_ref_args -- and everything REF adds sits in one block of its
// own, so that without them the body is, token for token, the one generate_steps_kernel and generate_whole_kernel had before.)
__device__ __forceinline__ const gen_ref_args &gen_ref_of(const gen_ref_args &ref) { return ref; }

template <int BITS, int W, bool STOP, class... Ref>
__device__ __forceinline__ void gen_run(const uint64_t *__restrict__ table, const uint32_t *__restrict__ counts, uint64_t n_table,
                                        const double *__restrict__ prior, const double *__restrict__ mat, uint64_t *__restrict__ keys,
                                        const uint64_t *__restrict__ sample, uint32_t *__restrict__ left, uint32_t *__restrict__ length,
                                        uint8_t *__restrict__ stopped, uint64_t n_seq, const gen_args &A, uint8_t *__restrict__ letters,
                                        int8_t *__restrict__ codes, const Ref &...ref_args) {
  constexpr bool REF = sizeof...(Ref) == 1;
  static_assert(sizeof...(Ref) <= 1 && (STOP || !REF), "a reference model generates whole sequences only");
  constexpr int NL = STOP ? W : W - 1;                           // the letters that are drawn
  constexpr int G = GEN_GROUP(NL);
  constexpr uint32_t PER_BLOCK = GEN_THREADS / G;
  constexpr bool MAT = STOP && W == 21;
  const uint32_t b = threadIdx.x % G, g = threadIdx.x / G;
  const uint64_t mask = (1ull << (BITS * A.lag)) - 1ull;         // BITS * lag <= 63
  [[maybe_unused]] double *exptab = nullptr, *R = nullptr, *M = nullptr;
  [[maybe_unused]] int8_t *s_cd = nullptr;
  if constexpr (MAT) {
    extern __shared__ __attribute__((aligned(16))) double gen_lds[];
    exptab = gen_lds;
    R = gen_lds + BEAR_EXPTAB_N;                                 // [PER_BLOCK][W]: the row of every group
    M = R + PER_BLOCK * W;                                       // [lag][W][W]
    s_cd = reinterpret_cast<int8_t *>(M + A.lag * W * W);        // [PER_BLOCK][16]: the code bytes of every group's k-mer
    if (mat) {                                                   // (the same for every thread of the launch)
      if (threadIdx.x < BEAR_EXPTAB_N) exptab[threadIdx.x] = exp2((double)threadIdx.x * (1.0 / BEAR_EXPTAB_N));
      for (int k = threadIdx.x; k < A.lag * W * W; k += GEN_THREADS) M[k] = mat[k];
      __syncthreads();
    }
  }
  for (uint64_t base = (uint64_t)blockIdx.x * PER_BLOCK; base < n_seq; base += (uint64_t)gridDim.x * PER_BLOCK) {
    const uint64_t i = base + g;
    const bool have = i < n_seq;
    uint64_t q = have ? keys[i] : 0ull;
    const uint64_t s = have ? sample[i] : 0ull;
    uint32_t rem = have ? left[i] : 0u;
    [[maybe_unused]] uint32_t len = 0u;
    [[maybe_unused]] bool stop = false;
    if constexpr (STOP) len = have ? length[i] : 0u;
    const uint32_t n_steps = (uint32_t)A.n_steps;                // (the entries refuse more than 2^32 - 1 steps)
    for (uint32_t k = 0; __any(k < n_steps && rem > 0u); ++k) {
      const bool live = k < n_steps && rem > 0u;       // the same on all lanes of a group
      const uint64_t t = A.step0 + k;
      uint32_t row = SCR_ABSENT;
      if (live && b == 0) row = scr_find_row(table, n_table, q);
      row = (uint32_t)__shfl((int)row, 0, G);
      double f = 0.0;
      if constexpr (MAT) {
        if (mat) {
          if (live && (int)b < A.lag) s_cd[g * 16 + b] = gen_code_at<BITS>(A, q, (int)b);
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          if (live && b == 0) lnw_forward_row(s_cd + g * 16, A.lag, M, exptab, R + g * W);
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          if (live && b < NL) f = R[g * W + b];
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // ... before the next step's row overwrites it
        }
      }
      if constexpr (REF) {     // f (so far the net function's row g, or nothing) becomes the reference-mixed row
        const gen_ref_args &ref = gen_ref_of(ref_args...);
        uint32_t ref_row = SCR_ABSENT;
        if (live && b == 0) ref_row = scr_find_row(ref.table, ref.n_table, q);
        ref_row = (uint32_t)__shfl((int)ref_row, 0, G);
        if (live && b < NL) {
          const uint32_t *rf = rfs_ref_row<W>(ref.counts, ref_row);
          const double Rt = rfw_ref_total<W>(rf, ref.prm.eps);
          const double gb = ref.net == BEAR_GEN_NET_STOP ? (b == (uint32_t)(W - 1) ? 1.0 : 0.0) : (prior ? prior[i * W + b] : f);
          f = rfs_prior_cell<W>(rf, (int)b, gb, Rt, 1.0 / Rt, ref.prm);
        }
      }
      double v = -INFINITY;
      if (live && b < NL) {
        const double c = row != SCR_ABSENT ? (double)counts[(uint64_t)row * W + b] : 0.0;
        if (!REF && prior) f = prior[i * W + b];                   // (never beside mat: the entry refuses the two together)
        const double conc = A.mode == BEAR_GEN_BMM ? A.van + c : (A.mode == BEAR_GEN_BEAR ? __builtin_fma(f, A.inv_h, c) : f);
        const double tv = A.map ? log(conc) : smp_log_gamma(conc, smp_cell_key(A.seed, 0u, s, mix64(q) + b));
        v = tv - log(-log(u01(smp_cell_key(A.seed, GEN_ID_GUMBEL, s, t * W + b))));
      }
      uint32_t best = b;       // the lowest letter with the largest value; an idle lane holds -inf under a letter beyond the row
#pragma unroll
      for (int off = G / 2; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off, G);
        const uint32_t ob = (uint32_t)__shfl_xor((int)best, off, G);
        const bool take = ov > v || (ov == v && ob < best);
        v = take ? ov : v;
        best = take ? ob : best;
      }
      best = (uint32_t)__shfl((int)best, 0, G);      // (one answer per group whatever a NaN did to the comparisons)
      if (live) {
        if (STOP && best == (uint32_t)(W - 1)) {     // the stop won: the sequence ends, its key stays
          stop = true;
          rem = 0u;
        } else {
          q = ((q << BITS) | (uint64_t)gen_byte3(A.rank, best)) & mask;
          if (b == 0) letters[i * A.stride + t] = (uint8_t)best;
          ++len;
          --rem;
        }
      }
    }
    if (have) {
      if (b == 0) {
        keys[i] = q;
        left[i] = rem;
        if constexpr (STOP) {
          length[i] = len;
          if (stop) stopped[i] = 1;
        }
      }
      if (codes)
        for (int p = (int)b; p < A.lag; p += G) codes[i * (uint64_t)A.lag + p] = gen_code_at<BITS>(A, q, p);
    }
  }
}

// The three kernels: each carries the arguments its body reads and nothing else (no LDS, length, stopped or mat without STOP; the
// reference column and the mixing constants with REF only).
template <int BITS, int W>
__global__ __launch_bounds__(GEN_THREADS) void generate_steps_kernel(const uint64_t *__restrict__ table,
                                                                     const uint32_t *__restrict__ counts, uint64_t n_table,
                                                                     const double *__restrict__ prior, uint64_t *__restrict__ keys,
                                                                     const uint64_t *__restrict__ sample, uint32_t *__restrict__ left,
                                                                     uint64_t n_seq, gen_args A, uint8_t *__restrict__ letters,
                                                                     int8_t *__restrict__ codes) {
  gen_run<BITS, W, false>(table, counts, n_table, prior, nullptr, keys, sample, left, nullptr, nullptr, n_seq, A, letters, codes);
}

template <int BITS, int W>
__global__ __launch_bounds__(GEN_THREADS) void generate_whole_kernel(const uint64_t *__restrict__ table,
                                                                     const uint32_t *__restrict__ counts, uint64_t n_table,
                                                                     const double *__restrict__ prior, const double *__restrict__ mat,
                                                                     uint64_t *__restrict__ keys, const uint64_t *__restrict__ sample,
                                                                     uint32_t *__restrict__ left, uint32_t *__restrict__ length,
                                                                     uint8_t *__restrict__ stopped, uint64_t n_seq, gen_args A,
                                                                     uint8_t *__restrict__ letters, int8_t *__restrict__ codes) {
  gen_run<BITS, W, true>(table, counts, n_table, prior, mat, keys, sample, left, length, stopped, n_seq, A, letters, codes);
}

template <int BITS, int W>
__global__ __launch_bounds__(GEN_THREADS) void generate_whole_ref_kernel(const uint64_t *__restrict__ table,
                                                                         const uint32_t *__restrict__ counts, uint64_t n_table,
                                                                         const double *__restrict__ prior, const double *__restrict__ mat,
                                                                         uint64_t *__restrict__ keys, const uint64_t *__restrict__ sample,
                                                                         uint32_t *__restrict__ left, uint32_t *__restrict__ length,
                                                                         uint8_t *__restrict__ stopped, uint64_t n_seq, gen_args A,
                                                                         uint8_t *__restrict__ letters, int8_t *__restrict__ codes,
                                                                         gen_ref_args ref) {
  gen_run<BITS, W, true>(table, counts, n_table, prior, mat, keys, sample, left, length, stopped, n_seq, A, letters, codes, ref);
}
