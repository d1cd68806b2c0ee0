// kernels_segment.h -- WHERE in a sequence which group of a count table speaks (bear_amd.classify.segment; include/bear_hip.h,
// bear_score_emit_groups_f64 and bear_hmm_groups_f64): the posterior-predictive log-probability of every position's letter under
// every group, and a hidden-Markov chain over the groups -- the best path, every position's posterior and the evidence.
//
//   emit_groups_kernel<W>   one thread per position in TEXT order (nothing is sorted: a position is one transition, not a run).
//                           The checked key of mrg_key, the prior row once, then a loop over the table's groups that reads that
//                           group's count row, and inside it the model loop: a_j and A as groups_terms_kernel forms them,
//                           e = log(a_l) - log(A).  emit [n_m, n_t, G]: a position's G values are adjacent, as the chain reads them.
//
// The chain is a recurrence over the steps of a segment; a cut into chunks of HMM_CHUNK steps makes it parallel.  A chunk acts on
// the forward vector that enters it as an S x S matrix in the semiring of the pass -- (logsumexp, +) for the evidence and the
// posterior, (max, +) for the best path -- and, read the other way, on the backward vector that leaves it.  Every kernel is
// written once over the semiring SR (hmm_lse / hmm_max) and over LW, the lanes of a lane group: state g of a vector lives on lane
// g of its group (LW = 4 for S <= 4, else 16; 64 / LW groups to a wave), a step gathers the vector with LW shuffles inside the
// group and reduces S terms in state order.  log_trans is staged in LDS once per block; a lane keeps its column and its row of it
// in registers.
//
//   hmm_matrix_kernel   segments of more than one chunk only (the chunk rule of kernels_score.h, scr_chunks_of_block): one lane
//                       group per chunk and row i -- the forward recurrence from the unit vector of state i.  mats [slot, S, S].
//   hmm_carry_kernel    one lane group per long segment and direction: the vector that enters every chunk (from log_start, in
//                       chunk order) and the one that leaves it (from 0, in reverse chunk order), by one vector-matrix product
//                       per chunk, four matrices in flight.  carry [slot, 2, S].
//   hmm_chunk_kernel    one lane group per chunk -- a segment of at most HMM_CHUNK steps is its one chunk, found by its own
//                       index: no matrix, no carry -- recomputes the forward values from the entering vector (kept in `fwd`),
//                       then the backward values from the leaving one, and writes log_post (SR = hmm_lse) or path (hmm_max) of
//                       every step, and at a segment's last chunk its scalar.  fwd = NULL: forward only, the scalar alone,
//                       by the last chunks alone.
//   hmm_normalise_kernel  one thread per step: takes log_evidence off the alpha + beta that the chunks of a segment beyond one
//                       chunk have written, so that log_post is alpha + beta - log_evidence to the bit in every chunk.
// No atomics, and every reduction runs in state order inside chunks cut from the segment's own start: a segment's bits depend on
// its own emissions and the chain only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kernels_marg.h"    // mrg_models, mrg_key; kernels_score.h: scr_last_le, scr_off, the chunk rule

#define EMT_THREADS 256
#define HMM_CHUNK BEAR_HMM_CHUNK           // steps of a chunk (include/bear_hip.h: part of the results)
#define HMM_MAX_STATES BEAR_HMM_MAX_STATES
#define HMM_THREADS 64                     // one wave: HMM_THREADS / LW lane groups
#define HMM_NO_STATE 0xFFu                 // path[t] where every path is -inf

template <int W>
__global__ __launch_bounds__(EMT_THREADS) void emit_groups_kernel(const int32_t *__restrict__ rows, const uint8_t *__restrict__ letters,
                                                                  uint64_t n_t, const uint32_t *__restrict__ train, uint32_t n_groups,
                                                                  const double *__restrict__ prior, uint64_t n_rows, mrg_models P,
                                                                  double *__restrict__ emit) {
  for (uint64_t i = (uint64_t)blockIdx.x * EMT_THREADS + threadIdx.x; i < n_t; i += (uint64_t)gridDim.x * EMT_THREADS) {
    const uint64_t key = mrg_key(rows, letters, i, W, n_rows);
    const bool live = key != MRG_NO_KEY;
    const uint64_t row = live ? key >> 8 : 0;            // nothing that is no transition's becomes an index
    const uint32_t letter = live ? (uint32_t)(key & 0xFFu) : 0u;
    const uint32_t *__restrict__ tr = train + row * n_groups * W;      // the k-mer's n_groups rows
    double f[W];                                         // the prior row, read once for every group and model
#pragma unroll
    for (int j = 0; j < W; ++j) f[j] = live && prior ? prior[row * W + j] : 0.0;
    for (uint32_t g = 0; g < n_groups; ++g) {
      uint32_t c[W];
#pragma unroll
      for (int j = 0; j < W; ++j) c[j] = live ? tr[g * W + j] : 0u;
      for (int m = 0; m < P.n_m; ++m) {
        const double w = P.w[m];
        const bool bear = m < P.n_h;
        double A = 0.0, al = 0.0;
#pragma unroll
        for (int j = 0; j < W; ++j) {
          const double aj = bear ? __builtin_fma(f[j], w, (double)c[j]) : (double)c[j] + w;
          A += aj;
          al = (uint32_t)j == letter ? aj : al;
        }
        emit[((uint64_t)m * n_t + i) * n_groups + g] = live ? log(al) - log(A) : 0.0;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ the chain
struct hmm_chain {
  double lt[HMM_MAX_STATES * HMM_MAX_STATES];            // log_trans [S, S], from-state by row
  double start[HMM_MAX_STATES];
  int S;
};

#define HMM_NEG_INF (-__builtin_huge_val())

// The two semirings: reduce = the "sum" of x[0 .. S) in state order (S is the same in every lane: the tests on it are the wave's).
struct hmm_max {
  template <int LW>
  static __device__ __forceinline__ double reduce(const double (&x)[LW], int S) {
    double m = x[0];
#pragma unroll
    for (int h = 1; h < LW; ++h)
      if (h < S) m = fmax(m, x[h]);
    return m;
  }
};

struct hmm_lse {
  // max + log(sum of exp(x - max)); over only -inf: -inf, never NaN
  template <int LW>
  static __device__ __forceinline__ double reduce(const double (&x)[LW], int S) {
    const double m = hmm_max::reduce<LW>(x, S);
    double s = 0.0;
#pragma unroll
    for (int h = 0; h < LW; ++h)
      if (h < S) s += exp(x[h] - m);
    return m == HMM_NEG_INF ? m : m + log(s);
  }
};

// the vector v of a lane group (state h on its lane h), in every lane
template <int LW>
__device__ __forceinline__ void hmm_gather(double v, double (&x)[LW]) {
#pragma unroll
  for (int h = 0; h < LW; ++h) x[h] = __shfl(v, h, LW);
}

// reduce over h of v(h) + w[h]: a vector-matrix product's entry of the lane that holds column (or row) w
template <class SR, int LW>
__device__ __forceinline__ double hmm_mix(double v, const double (&w)[LW], int S) {
  double x[LW];
  hmm_gather<LW>(v, x);
#pragma unroll
  for (int h = 0; h < LW; ++h) x[h] += w[h];
  return SR::template reduce<LW>(x, S);
}

// reduce over the states of v
template <class SR, int LW>
__device__ __forceinline__ double hmm_all(double v, int S) {
  double x[LW];
  hmm_gather<LW>(v, x);
  return SR::template reduce<LW>(x, S);
}

// log_trans into LDS, by the whole block
__device__ __forceinline__ void hmm_stage(const hmm_chain &P, double *lt) {
  for (int i = threadIdx.x; i < HMM_MAX_STATES * HMM_MAX_STATES; i += HMM_THREADS) lt[i] = P.lt[i];
  __syncthreads();
}

// the segment that holds the chunk start a of a long segment: its index and its ends inside the text
struct hmm_seg {
  uint64_t s, s0, s1;
};
__device__ __forceinline__ hmm_seg hmm_segment_of(const uint64_t *__restrict__ seg, uint64_t n_seg, uint64_t n_t, uint64_t a) {
  hmm_seg r;
  r.s = scr_last_le(seg, n_seg, a);                      // (empty segments that start at a stand in front of it)
  r.s0 = scr_off(seg, r.s, n_t);
  r.s1 = scr_off(seg, r.s + 1, n_t);
  return r;
}

// One forward step of lane `lane`'s state: e_t + reduce_h(v(h) + col[h]); at a segment's first step the vector that enters is
// the start and no transition is taken.
template <class SR, int LW>
__device__ __forceinline__ double hmm_forward_step(double v, double e, bool no_transition, const double (&col)[LW], int S) {
  return no_transition ? v + e : e + hmm_mix<SR, LW>(v, col, S);
}

template <class SR, int LW>
__global__ __launch_bounds__(HMM_THREADS) void hmm_matrix_kernel(const double *__restrict__ emit, uint64_t n_t,
                                                                 const uint64_t *__restrict__ seg, uint64_t n_seg, uint64_t n_blocks,
                                                                 hmm_chain P, double *__restrict__ mats) {
  __shared__ double lt[HMM_MAX_STATES * HMM_MAX_STATES];
  hmm_stage(P, lt);
  constexpr int GROUPS = HMM_THREADS / LW;
  const int S = P.S, lane = threadIdx.x % LW, grp = threadIdx.x / LW;
  const bool held = lane < S;                            // this lane holds a state
  double col[LW];
#pragma unroll
  for (int h = 0; h < LW; ++h) col[h] = held && h < S ? lt[h * S + lane] : HMM_NEG_INF;
  const uint64_t n_items = n_blocks * (uint64_t)S;       // (block of the text, row of the matrix)
  for (uint64_t item = (uint64_t)blockIdx.x * GROUPS + grp; item < n_items; item += (uint64_t)gridDim.x * GROUPS) {
    const uint64_t g = item / (uint64_t)S;
    const int i = (int)(item % (uint64_t)S);
    scr_chunks_of_block<HMM_CHUNK>(seg, n_seg, n_t, g, [&](uint64_t slot, uint64_t a, uint64_t b) {
      const bool first = hmm_segment_of(seg, n_seg, n_t, a).s0 == a;
      double v = lane == i ? 0.0 : HMM_NEG_INF;
      double e = held ? emit[a * S + lane] : HMM_NEG_INF;                      // (a chunk has a step)
      for (uint64_t t = a; t < b; ++t) {
        const double next = held && t + 1 < b ? emit[(t + 1) * S + lane] : HMM_NEG_INF;   // in flight during the step
        v = hmm_forward_step<SR, LW>(v, e, first && t == a, col, S);
        e = next;
      }
      if (held) mats[(slot * S + i) * S + lane] = v;
    });
  }
}

// carry [slot, 2, S]: [slot, 0] the forward vector in front of the chunk's first step (log_start at chunk 0), [slot, 1] the
// backward vector at its last step (0 at the last chunk); without `backward` only the former.
template <class SR, int LW>
__global__ __launch_bounds__(HMM_THREADS) void hmm_carry_kernel(const uint64_t *__restrict__ seg, uint64_t n_seg, uint64_t n_t,
                                                                hmm_chain P, const double *__restrict__ mats, bool backward,
                                                                double *__restrict__ carry) {
  constexpr int GROUPS = HMM_THREADS / LW;
  const int S = P.S, lane = threadIdx.x % LW, grp = threadIdx.x / LW;
  const bool held = lane < S;
  const double start = held ? P.start[lane] : HMM_NEG_INF;
  for (uint64_t item = (uint64_t)blockIdx.x * GROUPS + grp; item < 2 * n_seg; item += (uint64_t)gridDim.x * GROUPS) {
    const uint64_t s = item >> 1;
    const bool back = item & 1;
    const uint64_t s1 = scr_off(seg, s + 1, n_t);
    const uint64_t s0 = scr_off(seg, s, s1);
    if (s1 - s0 <= HMM_CHUNK) continue;                  // one chunk: hmm_chunk_kernel needs nothing from here
    if (back && !backward) continue;                     // a pass that forms no backward values
    const uint64_t K = (s1 - s0 + HMM_CHUNK - 1) / HMM_CHUNK;
    // forward: chunks 0 .. K - 1, the product with chunk k's matrix gives what enters chunk k + 1 (lane g holds column g);
    // backward: chunks K - 1 .. 0, the product with chunk k's matrix gives what leaves chunk k - 1 (lane g holds row g)
    double v = back ? (held ? 0.0 : HMM_NEG_INF) : start;
    for (uint64_t n = 0; n < K; n += 4) {
      double w[4][LW];
      uint64_t slot[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint64_t k = back ? K - 1 - (n + j) : n + j;                     // (n + j < K is tested below)
        slot[j] = n + j < K ? scr_chunk_slot<HMM_CHUNK>(s0, s0 + k * HMM_CHUNK) : 0;
        const bool more = n + j + 1 < K;                                       // a chunk behind this one in the pass
#pragma unroll
        for (int h = 0; h < LW; ++h)
          w[j][h] = more && held && h < S ? mats[(slot[j] * S + (back ? lane : h)) * S + (back ? h : lane)] : HMM_NEG_INF;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (n + j < K) {
          if (held) carry[(slot[j] * 2 + (back ? 1 : 0)) * S + lane] = v;
          if (n + j + 1 < K) v = hmm_mix<SR, LW>(v, w[j], S);
        }
      }
    }
  }
}

// The steps [a, b) of segment s: `in` the forward vector in front of step a (the start where `first`), `out` the backward vector
// at step b - 1.  By one lane group.  log_post of a segment of one chunk is written whole, alpha + beta less the evidence; of a
// longer one as alpha + beta, for hmm_normalise_kernel to take the segment's evidence off (no chunk but the last knows it).
template <class SR, int LW>
__device__ __forceinline__ void hmm_chunk(const double *__restrict__ emit, uint64_t a, uint64_t b, uint64_t s, bool first, bool last,
                                          double in, double out, const double (&col)[LW], const double (&row)[LW], int S, int lane,
                                          double *fwd, double *log_post, uint8_t *__restrict__ path, double *__restrict__ scalar) {   // (fwd may BE log_post)
  const bool held = lane < S;
  if (!fwd && !last) return;                             // forward only: the last chunk alone has something to write
  double v = in;
  double e = held && a < b ? emit[a * S + lane] : HMM_NEG_INF;
  for (uint64_t t = a; t < b; ++t) {
    const double next = held && t + 1 < b ? emit[(t + 1) * S + lane] : HMM_NEG_INF;       // in flight during the step
    v = hmm_forward_step<SR, LW>(v, e, first && t == a, col, S);
    if (fwd && held) fwd[t * S + lane] = v;
    e = next;
  }
  if (!fwd || a == b) {                                  // forward only, or a segment without a step: the reduced vector
    const double r = hmm_all<SR, LW>(v, S);              // (the whole lane group takes every shuffle)
    if (last && lane == 0) scalar[s] = r;
    return;
  }
  // the forward values of a segment's last step, reduced: the evidence (the best path's value)
  const double norm = hmm_all<SR, LW>(v, S);
  if (last && lane == 0) scalar[s] = norm;
  const double off = first && last ? norm : 0.0;         // one chunk: normalised here
  double bt = out;
  // what step b - 2 needs, then one step ahead of the loop: e_(t+1) and this lane's own forward value of t (written above)
  double e1 = held && b - a > 1 ? emit[(b - 1) * S + lane] : HMM_NEG_INF;
  double fw = held && b - a > 1 ? fwd[(b - 2) * S + lane] : HMM_NEG_INF;
  for (uint64_t t = b; t-- > a;) {
    if (t + 1 < b) {
      const double e1_next = held && t > a ? emit[t * S + lane] : HMM_NEG_INF;
      const double fw_next = held && t > a ? fwd[(t - 1) * S + lane] : HMM_NEG_INF;
      bt = hmm_mix<SR, LW>(e1 + bt, row, S);             // reduce_h(log_trans[g, h] + e_(t+1)(h) + beta_(t+1)(h))
      v = fw;
      e1 = e1_next;
      fw = fw_next;
    }
    const double z = v + bt;
    if (log_post && held) log_post[t * S + lane] = z - off;
    if (path) {                                          // the lowest state of the largest forward + backward value
      double x[LW];
      hmm_gather<LW>(z, x);
      const double m = hmm_max::reduce<LW>(x, S);
      uint32_t best = HMM_NO_STATE;
#pragma unroll
      for (int h = LW - 1; h >= 0; --h)
        if (h < S) best = x[h] == m ? (uint32_t)h : best;
      if (lane == 0) path[t] = (uint8_t)(m == HMM_NEG_INF ? HMM_NO_STATE : best);
    }
  }
}

// Items [0, n_seg): the segments of at most one chunk, each its own (and only) chunk; items [n_seg, n_seg + n_blocks): the blocks
// of the text, for the chunks of the longer segments that start there.  n_blocks = 0: no text beyond one chunk, carry is not read.
template <class SR, int LW>
__global__ __launch_bounds__(HMM_THREADS) void hmm_chunk_kernel(const double *__restrict__ emit, uint64_t n_t,
                                                                const uint64_t *__restrict__ seg, uint64_t n_seg, uint64_t n_blocks,
                                                                hmm_chain P, const double *__restrict__ carry, double *fwd,
                                                                double *log_post, uint8_t *__restrict__ path,
                                                                double *__restrict__ scalar) {
  __shared__ double lt[HMM_MAX_STATES * HMM_MAX_STATES];
  hmm_stage(P, lt);
  constexpr int GROUPS = HMM_THREADS / LW;
  const int S = P.S, lane = threadIdx.x % LW, grp = threadIdx.x / LW;
  const bool held = lane < S;
  double col[LW], row[LW];
#pragma unroll
  for (int h = 0; h < LW; ++h) {
    col[h] = held && h < S ? lt[h * S + lane] : HMM_NEG_INF;
    row[h] = held && h < S ? lt[lane * S + h] : HMM_NEG_INF;
  }
  const double start = held ? P.start[lane] : HMM_NEG_INF;
  const double zero = held ? 0.0 : HMM_NEG_INF;
  for (uint64_t item = (uint64_t)blockIdx.x * GROUPS + grp; item < n_seg + n_blocks; item += (uint64_t)gridDim.x * GROUPS) {
    if (item < n_seg) {
      const uint64_t s1 = scr_off(seg, item + 1, n_t);
      const uint64_t s0 = scr_off(seg, item, s1);
      if (s1 - s0 <= HMM_CHUNK) hmm_chunk<SR, LW>(emit, s0, s1, item, true, true, start, zero, col, row, S, lane, fwd, log_post, path, scalar);
    } else {
      scr_chunks_of_block<HMM_CHUNK>(seg, n_seg, n_t, item - n_seg, [&](uint64_t slot, uint64_t a, uint64_t b) {
        const hmm_seg of = hmm_segment_of(seg, n_seg, n_t, a);
        const double in = held ? carry[(slot * 2 + 0) * S + lane] : HMM_NEG_INF;
        const double out = held ? carry[(slot * 2 + 1) * S + lane] : HMM_NEG_INF;
        hmm_chunk<SR, LW>(emit, a, b, of.s, of.s0 == a, of.s1 == b, in, out, col, row, S, lane, fwd, log_post, path, scalar);
      });
    }
  }
}

// log_post of the segments of more than one chunk, which hmm_chunk_kernel left as alpha + beta: less the segment's log_evidence
// (written by that kernel at the segment's last chunk).  One thread per step.
#define HMM_NORM_THREADS 256
__global__ __launch_bounds__(HMM_NORM_THREADS) void hmm_normalise_kernel(const uint64_t *__restrict__ seg, uint64_t n_seg, uint64_t n_t,
                                                                         uint32_t S, const double *__restrict__ log_evidence,
                                                                         double *__restrict__ log_post) {
  const uint64_t first = scr_off(seg, 0, n_t), end = scr_off(seg, n_seg, n_t);
  for (uint64_t t = (uint64_t)blockIdx.x * HMM_NORM_THREADS + threadIdx.x; t < n_t; t += (uint64_t)gridDim.x * HMM_NORM_THREADS) {
    if (t < first || t >= end) continue;
    const uint64_t s = scr_last_le(seg, n_seg, t);
    const uint64_t s0 = scr_off(seg, s, n_t), s1 = scr_off(seg, s + 1, n_t);
    if (!(s0 <= t && t < s1 && s1 - s0 > HMM_CHUNK)) continue;
    const double ev = log_evidence[s];
    for (uint32_t g = 0; g < S; ++g) log_post[t * S + g] -= ev;
  }
}
