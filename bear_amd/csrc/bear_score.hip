// bear_score.hip -- scoring on the device: the entries between the device count tables and the samplers' tables
// (include/bear_hip.h, "Variant and sequence scoring"): symbols -> look-up keys, keys -> rows of a sorted key table, and the sums
// of a sampled table's rows over the transitions of every segment; the exact marginal of every segment (under one column, or under
// every column of a table with a leave-one-out column per segment) and the exact posterior
// mean and variance of every segment's score, which need no table -- and
// sequence generation over the same key tables ("Sequence generation": flanks of given lengths, and whole sequences from start to
// stop) -- and, for bear_ref models, the reference-mixed prior rows of queried k-mers and whole sequences under such a model.
// The only unit that includes -- and so emits --
// kernels_score.h, kernels_marg.h, kernels_groups.h, kernels_segment.h (every position's letter under every group, and the chain over
// the groups that segments a sequence), kernels_moments.h, kernels_refscore.h and kernels_generate.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "bear_dev.h"
#include "bear_release_guard.h"
#include "kernels_generate.h"
#include "kernels_groups.h"
#include "kernels_marg.h"
#include "kernels_moments.h"
#include "kernels_refscore.h"
#include "kernels_score.h"
#include "kernels_segment.h"

namespace {
bool misaligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }
bool misaligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

// blocks of a grid-stride launch over `work` items, `per_block` to a block
unsigned scr_grid(uint64_t work, uint64_t per_block) {
  const uint64_t g = (work + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > (1u << 20) ? (1u << 20) : g));
}

// the width-5 or the width-21 instantiation of a kernel (the entries have refused every other width)
#define LAUNCH_BY_WIDTH(width, k5, k21, grid, block, lds, stream, ...)              \
  do {                                                                              \
    if ((width) == 5)                                                               \
      hipLaunchKernelGGL(k5, grid, block, lds, stream, __VA_ARGS__);                \
    else                                                                            \
      hipLaunchKernelGGL(k21, grid, block, lds, stream, __VA_ARGS__);               \
  } while (0)

// What the generation entries check before any device call, and their argument block.  has_f: rows of the AR function are at
// hand (prior rows, or mat for the kernel to form them); per_step: they are prior rows, those of the CURRENT end k-mers.
bool gen_prepare(int lag, int width, const uint8_t *rank, int mode, int map, double h, double van, bool has_f, bool per_step,
                 uint64_t n_table, uint64_t seed, uint64_t step0, uint64_t n_steps, uint64_t letters_stride, gen_args &A) {
  if (width != 5 && width != 21) return false;
  if (lag < 1 || lag > (width == 5 ? 21 : 12) || !rank) return false;
  if (mode != BEAR_GEN_BMM && mode != BEAR_GEN_BEAR && mode != BEAR_GEN_AR) return false;
  if (mode != BEAR_GEN_BMM && !has_f) return false;
  if (mode == BEAR_GEN_AR && !map) return false;                         // the AR model is a table only at its MAP value
  if (per_step && n_steps > 1) return false;
  if (mode == BEAR_GEN_BEAR && !(h > 0.0)) return false;
  if (mode == BEAR_GEN_BMM && !(van > 0.0)) return false;
  if (n_table >= SCR_ABSENT || n_steps > 0xFFFFFFFFull || step0 > (~0ull) - n_steps || letters_stride < step0 + n_steps) return false;
  const int bits = width == 5 ? 3 : 5;
  memset(&A, 0, sizeof(A));
  for (int c = 0; c <= width; ++c) {
    if (c == width - 1) continue;                                        // the stop: no letter of a context
    if (rank[c] >= (1u << bits)) return false;
    if (c < width - 1) A.rank[c >> 3] |= (uint64_t)rank[c] << ((c & 7) * 8);
    A.code[rank[c] >> 3] |= (uint64_t)(c < width - 1 ? c : width - 1) << ((rank[c] & 7) * 8);      // core.encode_kmers: '[' = A
  }
  A.lag = lag;
  A.mode = mode;
  A.map = map != 0;
  A.inv_h = mode == BEAR_GEN_BEAR ? 1.0 / h : 0.0;
  A.van = mode == BEAR_GEN_BMM ? van : 0.0;
  A.seed = seed;
  A.step0 = step0;
  A.n_steps = n_steps;
  A.stride = letters_stride;
  return true;
}

// ... and of their pointers, once there are sequences
bool gen_pointers_ok(const uint64_t *table, const uint32_t *counts, uint64_t n_table, const double *prior, const uint64_t *keys,
                     const uint64_t *sample, const uint32_t *left, uint64_t n_seq, uint64_t n_steps, const uint8_t *letters,
                     uint64_t letters_stride) {
  if (!keys || !sample || !left || (n_steps && !letters) || misaligned8(keys) || misaligned8(sample) || misaligned4(left) ||
      (prior && misaligned8(prior)) || (n_table && (!table || !counts || misaligned8(table) || misaligned4(counts))))
    return false;
  return !(letters_stride && n_seq > (~0ull) / letters_stride);
}

// The one launch of both entries: generate_whole_kernel (STOP) or generate_steps_kernel of the width, a block per GEN_THREADS /
// GEN_GROUP(letter lanes) sequences.  With mat (width 21, STOP) every block stages mat: few blocks, a stride, and the dynamic LDS image.
template <bool STOP>
int gen_launch(int width, const uint64_t *table, const uint32_t *counts, uint64_t n_table, const double *prior, const double *mat,
               uint64_t *keys, const uint64_t *sample, uint32_t *left, uint32_t *length, uint8_t *stopped, uint64_t n_seq,
               const gen_args &A, uint8_t *letters, int8_t *codes, void *stream) {
  if (A.n_steps == 0 && !codes) return BEAR_OK;
  const int nl = STOP ? width : width - 1;
  unsigned grid = scr_grid(n_seq, GEN_THREADS / GEN_GROUP(nl));
  if (mat && grid > GEN_WHOLE_MAT_BLOCKS) grid = GEN_WHOLE_MAT_BLOCKS;
  const dim3 blocks(grid), block(GEN_THREADS);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if constexpr (STOP)
    LAUNCH_BY_WIDTH(width, (generate_whole_kernel<3, 5>), (generate_whole_kernel<5, 21>), blocks, block, mat ? GEN_WHOLE_MAT_LDS(A.lag) : 0,
                    s, table, counts, n_table, prior, mat, keys, sample, left, length, stopped, n_seq, A, letters, codes);
  else
    LAUNCH_BY_WIDTH(width, (generate_steps_kernel<3, 5>), (generate_steps_kernel<5, 21>), blocks, block, 0, s, table, counts, n_table,
                    prior, keys, sample, left, n_seq, A, letters, codes);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

}  // namespace

extern "C" {

int bear_score_transitions_u64(const uint8_t *text, const uint64_t *seg, uint64_t n_sym, uint64_t n_seg, int lag, int width,
                               const uint8_t *rank, uint64_t *keys, uint8_t *letters, void *stream) {
  if (width != 5 && width != 21) return BEAR_ERR_INVALID_ARG;
  if (lag < 1 || lag > (width == 5 ? 21 : 12) || !rank) return BEAR_ERR_INVALID_ARG;
  const int bits = width == 5 ? 3 : 5;
  scr_ranks R;
  memset(R.rank, 0xFF, sizeof(R.rank));
  for (int c = 0; c <= width; ++c) {
    if (rank[c] != 0xFF && rank[c] >= (1u << bits)) return BEAR_ERR_INVALID_ARG;
    R.rank[c] = rank[c];
  }
  if (n_sym == 0) return BEAR_OK;
  if (!text || !keys || !letters || misaligned8(keys) || (n_seg && (!seg || misaligned8(seg)))) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(scr_grid(n_sym, SCR_THREADS)), block(SCR_THREADS);
  LAUNCH_BY_WIDTH(width, score_transitions_kernel<3>, score_transitions_kernel<5>, grid, block, 0, s, text, seg, n_sym, n_seg, lag,
                  (uint32_t)width, R, keys, letters);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_kmer_find_u64(const uint64_t *table, uint64_t n_table, const uint64_t *query, uint64_t n_query, uint32_t *rows,
                       void *stream) {
  if (n_table >= SCR_ABSENT) return BEAR_ERR_INVALID_ARG;      // a row is a uint32, and the last one says "absent"
  if (n_query == 0) return BEAR_OK;
  if (!query || !rows || misaligned8(query) || misaligned4(rows) || (n_table && (!table || misaligned8(table))))
    return BEAR_ERR_INVALID_ARG;
  hipLaunchKernelGGL(kmer_find_kernel, dim3(scr_grid(n_query, SCR_THREADS)), dim3(SCR_THREADS), 0, static_cast<hipStream_t>(stream),
                     table, n_table, query, n_query, rows);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_score_sum_f64(const double *lp, uint64_t n_rows, int width, uint64_t n_values, const uint32_t *rows, const uint8_t *letters,
                       uint64_t n_t, const uint64_t *seg, uint64_t n_seg, double *scores, void *stream) {
  if (width != 5 && width != 21) return BEAR_ERR_INVALID_ARG;
  if (n_rows >= SCR_ABSENT || n_values > 65535ull * SCR_WAVE) return BEAR_ERR_INVALID_ARG;
  if (n_seg == 0 || n_values == 0) return BEAR_OK;
  if (!seg || !scores || misaligned8(seg) || misaligned8(scores)) return BEAR_ERR_INVALID_ARG;
  if (n_t && (!rows || !letters || misaligned4(rows))) return BEAR_ERR_INVALID_ARG;
  if (n_t && n_rows && (!lp || misaligned8(lp))) return BEAR_ERR_INVALID_ARG;
  if (n_seg > (~0ull) / n_values / sizeof(double)) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned tiles = (unsigned)((n_values + SCR_WAVE - 1) / SCR_WAVE);
  // only a text of more than SCR_CHUNK transitions can hold a long segment: two partial rows per SCR_CHUNK positions of the text
  dev_buf<double> partials;
  if (n_t > SCR_CHUNK) {
    const uint64_t n_blocks = (n_t + SCR_CHUNK - 1) / SCR_CHUNK;
    if (n_blocks > (~0ull) / (2 * sizeof(double)) / n_values) return BEAR_ERR_INVALID_ARG;
    HIP_TRY(partials.alloc(2 * n_blocks * n_values));
    hipLaunchKernelGGL(score_chunk_kernel, dim3(scr_grid(n_blocks, 1), tiles), dim3(SCR_WAVE), 0, s, lp, n_rows, (uint32_t)width,
                       n_values, rows, letters, seg, n_seg, n_t, n_blocks, partials.get());
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(score_sum_kernel, dim3(scr_grid(n_seg, 1), tiles), dim3(SCR_WAVE), 0, s, lp, n_rows, (uint32_t)width, n_values,
                     rows, letters, seg, n_seg, n_t, partials.get(), scores);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;      // (partials goes with this frame: hipFree waits for the two launches)
}

}  // extern "C"

namespace {
// What bear_score_marg_f64 and bear_score_moments_f64 check alike before any device call, and their models: BEAR_OK with
// P filled, or the status to return.  out: the scores / the moments; planes: values per segment and model (1 / 2).
int mrg_prepare(const int32_t *rows, const uint8_t *letters, uint64_t n_t, const uint64_t *seg, uint64_t n_seg, int width,
                const uint32_t *train, const double *prior, uint64_t n_rows, const double *h, int n_h, const double *van, int n_van,
                const double *out, uint64_t planes, mrg_models &P) {
  if (width != 5 && width != 21) return BEAR_ERR_INVALID_ARG;
  if (n_h < 0 || n_van < 0 || n_h > MRG_MAX_MODELS || n_van > MRG_MAX_MODELS || n_h + n_van < 1 || n_h + n_van > MRG_MAX_MODELS)
    return BEAR_ERR_INVALID_ARG;
  if ((n_h > 0 && (!h || !prior)) || (n_van > 0 && !van)) return BEAR_ERR_INVALID_ARG;
  memset(&P, 0, sizeof(P));
  P.n_h = n_h;
  P.n_m = n_h + n_van;
  for (int m = 0; m < n_h; ++m) {
    if (!(h[m] > 0.0)) return BEAR_ERR_INVALID_ARG;
    P.w[m] = 1.0 / h[m];
  }
  for (int m = 0; m < n_van; ++m) {
    if (!(van[m] > 0.0)) return BEAR_ERR_INVALID_ARG;
    P.w[n_h + m] = van[m];
  }
  if (n_rows >= SCR_ABSENT) return BEAR_ERR_INVALID_ARG;
  if (n_seg == 0) return BEAR_OK;
  if (!seg || !out || misaligned8(seg) || misaligned8(out)) return BEAR_ERR_INVALID_ARG;
  if (n_t && (!rows || !letters || misaligned4(rows))) return BEAR_ERR_INVALID_ARG;
  if (n_t && n_rows && (!train || misaligned4(train))) return BEAR_ERR_INVALID_ARG;
  if (n_h > 0 && misaligned8(prior)) return BEAR_ERR_INVALID_ARG;
  const uint64_t M = (uint64_t)P.n_m * planes;
  if (n_seg > (~0ull) / M / sizeof(double) || n_t > (~0ull) / M / sizeof(double)) return BEAR_ERR_INVALID_ARG;
  return BEAR_OK;
}

// ... and the sums behind their terms [M, n_t]: scores [n_seg, M].  partials: two rows per MRG_CHUNK positions of a text of
// n_blocks > 0 chunks (only a text beyond one chunk can hold a long segment); not read otherwise.
int mrg_sum_launches(const double *terms, uint64_t M, const uint64_t *seg, uint64_t n_seg, uint64_t n_t, uint64_t n_blocks,
                     double *partials, double *scores, hipStream_t s) {
  if (n_blocks) {
    hipLaunchKernelGGL(marg_chunk_kernel, dim3(scr_grid(n_blocks, 1), (unsigned)M), dim3(MRG_WAVE), 0, s, terms, (uint32_t)M, seg, n_seg,
                       n_t, n_blocks, partials);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(marg_sum_kernel, dim3(scr_grid(n_seg, 1), (unsigned)M), dim3(MRG_WAVE), 0, s, terms, (uint32_t)M, seg, n_seg, n_t,
                     partials, scores);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

// the chunks of a text: 0 up to MRG_CHUNK positions
uint64_t mrg_chunk_blocks(uint64_t n_t) { return n_t > MRG_CHUNK ? (n_t + MRG_CHUNK - 1) / MRG_CHUNK : 0; }

// the sums of bear_score_marg_f64 and bear_score_moments_f64, which hold their partial rows in a dev_buf
int mrg_sums(const dev_buf<double> &terms, uint64_t M, const uint64_t *seg, uint64_t n_seg, uint64_t n_t, double *scores,
             hipStream_t s) {
  dev_buf<double> partials;
  const uint64_t n_blocks = mrg_chunk_blocks(n_t);
  if (n_blocks) HIP_TRY(partials.alloc(2 * n_blocks * M));
  return mrg_sum_launches(terms.get(), M, seg, n_seg, n_t, n_blocks, partials.get(), scores, s);
  // (partials goes with this frame: hipFree waits for the launches)
}

// Scratch of bear_score_groups_f64: taken from and given back to the device's memory pool IN STREAM ORDER (hipMallocAsync /
// hipFreeAsync), so the entry neither waits for its stream nor for the device.  Given back with the owner, behind whatever the
// entry has launched on the stream by then.
class stream_buf {
 public:
  explicit stream_buf(hipStream_t s) : s_(s) {}
  stream_buf(const stream_buf &) = delete;
  stream_buf &operator=(const stream_buf &) = delete;
  ~stream_buf() {
    if (p_) (void)hipFreeAsync(p_, s_);
  }
  double *get() const { return p_; }
  hipError_t alloc(size_t n) { return hipMallocAsync(reinterpret_cast<void **>(&p_), n * sizeof(double), s_); }

 private:
  hipStream_t s_;
  double *p_ = nullptr;
};
}  // namespace

extern "C" {

int bear_score_marg_f64(const int32_t *rows, const uint8_t *letters, uint64_t n_t, const uint64_t *seg, uint64_t n_seg, int width,
                        const uint32_t *train, const double *prior, uint64_t n_rows, const double *h, int n_h, const double *van,
                        int n_van, double *scores, void *stream) {
  mrg_models P;
  const int st = mrg_prepare(rows, letters, n_t, seg, n_seg, width, train, prior, n_rows, h, n_h, van, n_van, scores, 1, P);
  if (st != BEAR_OK || n_seg == 0) return st;
  const uint64_t M = (uint64_t)P.n_m;
  hipStream_t s = static_cast<hipStream_t>(stream);
  dev_buf<double> terms;                 // one term per position and model
  if (n_t) {
    HIP_TRY(terms.alloc(n_t * M));
    const dim3 grid(scr_grid(n_t, MRG_THREADS)), block(MRG_THREADS);
    LAUNCH_BY_WIDTH(width, marg_terms_kernel<5>, marg_terms_kernel<21>, grid, block, 0, s, rows, letters, n_t, seg, n_seg, train,
                    n_h > 0 ? prior : nullptr, n_rows, P, terms.get());
    HIP_TRY(hipGetLastError());
  }
  return mrg_sums(terms, M, seg, n_seg, n_t, scores, s);      // (terms goes with this frame: hipFree waits for the launches)
}

int bear_score_moments_f64(const int32_t *rows, const uint8_t *letters, const int64_t *weight_prefix, uint64_t n_t, const uint64_t *seg,
                           uint64_t n_seg, int width, const uint32_t *train, const double *prior, uint64_t n_rows, const double *h,
                           int n_h, const double *van, int n_van, double *moments, void *stream) {
  mrg_models P;
  const int st = mrg_prepare(rows, letters, n_t, seg, n_seg, width, train, prior, n_rows, h, n_h, van, n_van, moments, 2, P);
  if (st != BEAR_OK) return st;
  if (weight_prefix && misaligned8(weight_prefix)) return BEAR_ERR_INVALID_ARG;
  if (n_seg == 0) return BEAR_OK;
  const uint64_t M = 2 * (uint64_t)P.n_m;                     // planes: the mean and the variance of every model
  hipStream_t s = static_cast<hipStream_t>(stream);
  dev_buf<double> terms;
  if (n_t) {
    HIP_TRY(terms.alloc(n_t * M));
    const dim3 grid(scr_grid(n_t, MRG_THREADS)), block(MRG_THREADS);
    LAUNCH_BY_WIDTH(width, moments_terms_kernel<5>, moments_terms_kernel<21>, grid, block, 0, s, rows, letters, weight_prefix, n_t, seg,
                    n_seg, train, n_h > 0 ? prior : nullptr, n_rows, P, terms.get());
    HIP_TRY(hipGetLastError());
  }
  return mrg_sums(terms, M, seg, n_seg, n_t, moments, s);     // plane 2 m + k of segment i lands at moments[i, m, k]
}

int bear_score_groups_f64(const int32_t *rows, const uint8_t *letters, uint64_t n_t, const uint64_t *seg, uint64_t n_seg, int width,
                          const uint32_t *train, int n_groups, const double *prior, uint64_t n_rows, const int32_t *own,
                          const double *h, int n_h, const double *van, int n_van, void *stream, double *scores, uint8_t *short_of) {
  if (n_groups < 1 || n_groups > BEAR_GROUPS_MAX) return BEAR_ERR_INVALID_ARG;
  mrg_models P;
  const int st = mrg_prepare(rows, letters, n_t, seg, n_seg, width, train, prior, n_rows, h, n_h, van, n_van, scores, (uint64_t)n_groups, P);
  if (st != BEAR_OK) return st;
  if (own && misaligned4(own)) return BEAR_ERR_INVALID_ARG;
  if (n_seg == 0) return BEAR_OK;
  if (!short_of) return BEAR_ERR_INVALID_ARG;
  const uint64_t M = (uint64_t)n_groups * (uint64_t)P.n_m;    // planes: group-major, a group's models as bear_score_marg_f64 orders them
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipMemsetAsync(short_of, 0, n_seg, s));
  stream_buf terms(s), partials(s);
  const uint64_t n_blocks = mrg_chunk_blocks(n_t);
  if (n_t) {
    HIP_TRY(terms.alloc(n_t * M));
    if (n_blocks) HIP_TRY(partials.alloc(2 * n_blocks * M));
    const dim3 grid(scr_grid(n_t, MRG_THREADS)), block(MRG_THREADS);
    LAUNCH_BY_WIDTH(width, groups_terms_kernel<5>, groups_terms_kernel<21>, grid, block, 0, s, rows, letters, n_t, seg, n_seg, train,
                    (uint32_t)n_groups, n_h > 0 ? prior : nullptr, n_rows, own, P, terms.get(), short_of);
    HIP_TRY(hipGetLastError());
  }
  return mrg_sum_launches(terms.get(), M, seg, n_seg, n_t, n_blocks, partials.get(), scores, s);   // scores [n_seg, n_groups, n_m]
}

int bear_score_emit_groups_f64(const int32_t *rows, const uint8_t *letters, uint64_t n_t, int width, const uint32_t *train, int n_groups,
                               const double *prior, uint64_t n_rows, const double *h, int n_h, const double *van, int n_van, void *stream,
                               double *emit) {
  if (n_groups < 1 || n_groups > BEAR_GROUPS_MAX) return BEAR_ERR_INVALID_ARG;
  mrg_models P;      // (no segments here: the width, the models and n_rows as bear_score_groups_f64 checks them, the pointers below)
  const int st = mrg_prepare(nullptr, nullptr, 0, nullptr, 0, width, train, prior, n_rows, h, n_h, van, n_van, nullptr, 1, P);
  if (st != BEAR_OK) return st;
  if (n_h > 0 && misaligned8(prior)) return BEAR_ERR_INVALID_ARG;
  if (n_t == 0) return BEAR_OK;
  if (!rows || !letters || !emit || misaligned4(rows) || misaligned8(emit)) return BEAR_ERR_INVALID_ARG;
  if (n_rows && (!train || misaligned4(train))) return BEAR_ERR_INVALID_ARG;
  if (n_t > (~0ull) / ((uint64_t)n_groups * (uint64_t)P.n_m) / sizeof(double)) return BEAR_ERR_INVALID_ARG;
  const dim3 grid(scr_grid(n_t, EMT_THREADS)), block(EMT_THREADS);
  LAUNCH_BY_WIDTH(width, emit_groups_kernel<5>, emit_groups_kernel<21>, grid, block, 0, static_cast<hipStream_t>(stream), rows, letters, n_t,
                  train, (uint32_t)n_groups, n_h > 0 ? prior : nullptr, n_rows, P, emit);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

}  // extern "C"

namespace {
// The chain of bear_hmm_groups_f64 as the kernels take it.  False: NaN or +inf anywhere, a row of log_trans or a log_start without
// a finite entry.
bool hmm_chain_of(const double *log_trans, const double *log_start, int S, hmm_chain &P) {
  memset(&P, 0, sizeof(P));
  P.S = S;
  for (int g = 0; g <= S; ++g) {                         // the rows of log_trans, then log_start
    const double *src = g < S ? log_trans + g * S : log_start;
    double *dst = g < S ? P.lt + g * S : P.start;
    bool any = false;
    for (int k = 0; k < S; ++k) {
      if (isnan(src[k]) || src[k] == HUGE_VAL) return false;
      any = any || isfinite(src[k]);
      dst[k] = src[k];
    }
    if (!any) return false;
  }
  return true;
}

// One pass of the chain in the semiring SR: the chunks' matrices and the carried vectors where the text goes beyond one chunk
// (n_blocks > 0), then every chunk.
template <class SR, int LW>
int hmm_pass(const double *emit, uint64_t n_t, const uint64_t *seg, uint64_t n_seg, uint64_t n_blocks, const hmm_chain &P, double *mats,
             double *carry, double *fwd, double *log_post, uint8_t *path, double *scalar, hipStream_t s) {
  constexpr uint64_t groups = HMM_THREADS / LW;
  if (n_blocks) {
    hipLaunchKernelGGL((hmm_matrix_kernel<SR, LW>), dim3(scr_grid(n_blocks * (uint64_t)P.S, groups)), dim3(HMM_THREADS), 0, s, emit, n_t, seg,
                       n_seg, n_blocks, P, mats);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((hmm_carry_kernel<SR, LW>), dim3(scr_grid(2 * n_seg, groups)), dim3(HMM_THREADS), 0, s, seg, n_seg, n_t, P, mats,
                       fwd != nullptr, carry);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL((hmm_chunk_kernel<SR, LW>), dim3(scr_grid(n_seg + n_blocks, groups)), dim3(HMM_THREADS), 0, s, emit, n_t, seg, n_seg,
                     n_blocks, P, carry, fwd, log_post, path, scalar);
  HIP_TRY(hipGetLastError());
  if (n_blocks && log_post) {                            // the chunks of the longer segments wrote alpha + beta: less the evidence
    hipLaunchKernelGGL(hmm_normalise_kernel, dim3(scr_grid(n_t, HMM_NORM_THREADS)), dim3(HMM_NORM_THREADS), 0, s, seg, n_seg, n_t,
                       (uint32_t)P.S, scalar, log_post);
    HIP_TRY(hipGetLastError());
  }
  return BEAR_OK;
}
}  // namespace

extern "C" {

int bear_hmm_groups_f64(const double *emit, uint64_t n_t, const uint64_t *seg, uint64_t n_seg, int n_states, const double *log_trans,
                        const double *log_start, void *stream, double *log_evidence, double *log_best, uint8_t *path, double *log_post) {
  if (n_states < 1 || n_states > BEAR_HMM_MAX_STATES || !log_trans || !log_start) return BEAR_ERR_INVALID_ARG;
  hmm_chain P;
  if (!hmm_chain_of(log_trans, log_start, n_states, P)) return BEAR_ERR_INVALID_ARG;
  if (log_post && misaligned8(log_post)) return BEAR_ERR_INVALID_ARG;
  if (n_seg == 0) return BEAR_OK;
  if (!seg || !log_evidence || !log_best || misaligned8(seg) || misaligned8(log_evidence) || misaligned8(log_best))
    return BEAR_ERR_INVALID_ARG;
  if (n_t && (!emit || !path || misaligned8(emit))) return BEAR_ERR_INVALID_ARG;
  const uint64_t S = (uint64_t)n_states;
  if (n_t > (~0ull) / S / sizeof(double) / 4 || n_seg > (~0ull) / sizeof(double) / 4) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // only a text of more than BEAR_HMM_CHUNK steps can hold a segment of more than one chunk: two slots per chunk of the text
  const uint64_t n_blocks = n_t > HMM_CHUNK ? (n_t + HMM_CHUNK - 1) / HMM_CHUNK : 0;
  stream_buf mats(s), carry(s), delta(s);                // both passes use them in turn, in stream order
  if (n_blocks) {
    HIP_TRY(mats.alloc(2 * n_blocks * S * S));
    HIP_TRY(carry.alloc(2 * n_blocks * 2 * S));
  }
  if (n_t) HIP_TRY(delta.alloc(n_t * S));                // the forward values of the max pass (the sum pass keeps its own in log_post)
  int st;
  if (n_states <= 4) {
    st = hmm_pass<hmm_lse, 4>(emit, n_t, seg, n_seg, n_blocks, P, mats.get(), carry.get(), log_post, log_post, nullptr, log_evidence, s);
    if (st == BEAR_OK)
      st = hmm_pass<hmm_max, 4>(emit, n_t, seg, n_seg, n_blocks, P, mats.get(), carry.get(), delta.get(), nullptr, path, log_best, s);
  } else {
    st = hmm_pass<hmm_lse, 16>(emit, n_t, seg, n_seg, n_blocks, P, mats.get(), carry.get(), log_post, log_post, nullptr, log_evidence, s);
    if (st == BEAR_OK)
      st = hmm_pass<hmm_max, 16>(emit, n_t, seg, n_seg, n_blocks, P, mats.get(), carry.get(), delta.get(), nullptr, path, log_best, s);
  }
  return st;
}

int bear_generate_steps_f64(const uint64_t *table, const uint32_t *counts, uint64_t n_table, int lag, int width, const uint8_t *rank,
                            int mode, int map, double h, double van, const double *prior, uint64_t seed, uint64_t *keys,
                            const uint64_t *sample, uint32_t *left, uint64_t n_seq, uint64_t step0, uint64_t n_steps,
                            uint8_t *letters, uint64_t letters_stride, int8_t *codes, void *stream) {
  gen_args A;
  if (!gen_prepare(lag, width, rank, mode, map, h, van, prior != nullptr, prior != nullptr, n_table, seed, step0, n_steps, letters_stride, A))
    return BEAR_ERR_INVALID_ARG;
  if (n_seq == 0) return BEAR_OK;
  if (!gen_pointers_ok(table, counts, n_table, prior, keys, sample, left, n_seq, n_steps, letters, letters_stride))
    return BEAR_ERR_INVALID_ARG;
  return gen_launch<false>(width, table, counts, n_table, prior, nullptr, keys, sample, left, nullptr, nullptr, n_seq, A, letters, codes,
                           stream);
}

int bear_generate_whole_f64(const uint64_t *table, const uint32_t *counts, uint64_t n_table, int lag, int width, const uint8_t *rank,
                            int mode, int map, double h, double van, const double *prior, const double *mat, uint64_t seed,
                            uint64_t *keys, const uint64_t *sample, uint32_t *left, uint32_t *length, uint8_t *stopped, uint64_t n_seq,
                            uint64_t step0, uint64_t n_steps, uint8_t *letters, uint64_t letters_stride, int8_t *codes, void *stream) {
  if ((prior && mat) || (mat && width != 21)) return BEAR_ERR_INVALID_ARG;      // one source of rows; the function in the kernel: width 21
  gen_args A;
  if (!gen_prepare(lag, width, rank, mode, map, h, van, prior || mat, prior != nullptr, n_table, seed, step0, n_steps, letters_stride, A))
    return BEAR_ERR_INVALID_ARG;
  if (n_seq == 0) return BEAR_OK;
  if (!gen_pointers_ok(table, counts, n_table, prior, keys, sample, left, n_seq, n_steps, letters, letters_stride) || !length ||
      !stopped || misaligned4(length) || (mat && misaligned8(mat)))
    return BEAR_ERR_INVALID_ARG;
  return gen_launch<true>(width, table, counts, n_table, prior, mat, keys, sample, left, length, stopped, n_seq, A, letters, codes, stream);
}

}  // extern "C"

// ------------------------------------------------------------------ bear_ref models downstream of training
namespace {
// The mixing constants of a bear_ref model from its two scalars, on the host: E = exp(-tau), V = 1 / (nw + 1).  False: tau or nw not
// finite and > 0, or eps not finite and >= 0.
bool ref_params(double tau, double net_weight, double eps, bear_params &prm) {
  if (!(isfinite(tau) && tau > 0.0 && isfinite(net_weight) && net_weight > 0.0 && isfinite(eps) && eps >= 0.0)) return false;
  memset(&prm, 0, sizeof(prm));
  prm.eps = eps;
  prm.tau = tau;
  prm.E = exp(-tau);
  prm.tauE = tau * prm.E;
  prm.nw = net_weight;
  prm.V = 1.0 / (net_weight + 1.0);
  return true;
}

// ... and generate_whole_kernel's launch for generate_whole_ref_kernel
int gen_launch_ref(int width, const uint64_t *table, const uint32_t *counts, uint64_t n_table, const double *prior, const double *mat,
                   uint64_t *keys, const uint64_t *sample, uint32_t *left, uint32_t *length, uint8_t *stopped, uint64_t n_seq,
                   const gen_args &A, uint8_t *letters, int8_t *codes, const gen_ref_args &ref, void *stream) {
  if (A.n_steps == 0 && !codes) return BEAR_OK;
  unsigned grid = scr_grid(n_seq, GEN_THREADS / GEN_GROUP(width));
  if (mat && grid > GEN_WHOLE_MAT_BLOCKS) grid = GEN_WHOLE_MAT_BLOCKS;
  LAUNCH_BY_WIDTH(width, (generate_whole_ref_kernel<3, 5>), (generate_whole_ref_kernel<5, 21>), dim3(grid), dim3(GEN_THREADS),
                  mat ? GEN_WHOLE_MAT_LDS(A.lag) : 0, static_cast<hipStream_t>(stream), table, counts, n_table, prior, mat, keys, sample, left,
                  length, stopped, n_seq, A, letters, codes, ref);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}
}  // namespace

extern "C" {

int bear_ref_prior_rows_f64(const uint64_t *ref_table, const uint32_t *ref_counts, uint64_t n_ref, int width, const uint64_t *query,
                            uint64_t n_query, const double *net_rows, double tau, double net_weight, double eps, double *prior,
                            void *stream) {
  if (width != 5 && width != 21) return BEAR_ERR_INVALID_ARG;
  bear_params prm;
  if (!ref_params(tau, net_weight, eps, prm)) return BEAR_ERR_INVALID_ARG;
  if (n_ref >= SCR_ABSENT || n_query > (~0ull) / sizeof(double) / (uint64_t)width) return BEAR_ERR_INVALID_ARG;
  if (n_ref && (!ref_table || !ref_counts || misaligned8(ref_table) || misaligned4(ref_counts))) return BEAR_ERR_INVALID_ARG;
  if (n_query == 0) return BEAR_OK;
  if (!query || !prior || misaligned8(query) || misaligned8(prior) || (net_rows && misaligned8(net_rows))) return BEAR_ERR_INVALID_ARG;
  const dim3 grid(scr_grid(n_query, SCR_THREADS)), block(SCR_THREADS);
  LAUNCH_BY_WIDTH(width, ref_prior_rows_kernel<5>, ref_prior_rows_kernel<21>, grid, block, 0, static_cast<hipStream_t>(stream), ref_table,
                  ref_counts, n_ref, query, n_query, net_rows, prm, prior);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_generate_whole_ref_f64(const uint64_t *table, const uint32_t *counts, uint64_t n_table, int lag, int width, const uint8_t *rank,
                                int mode, int map, double h, double van, const double *prior, const double *mat, uint64_t seed,
                                uint64_t *keys, const uint64_t *sample, uint32_t *left, uint32_t *length, uint8_t *stopped, uint64_t n_seq,
                                uint64_t step0, uint64_t n_steps, uint8_t *letters, uint64_t letters_stride, int8_t *codes,
                                const uint64_t *ref_table, const uint32_t *ref_counts, uint64_t n_ref, double tau, double net_weight,
                                double eps, int net, void *stream) {
  if (mode != BEAR_GEN_BEAR && mode != BEAR_GEN_AR) return BEAR_ERR_INVALID_ARG;       // a BMM has no AR function to mix
  // the one source of the net function's rows that `net` names, and no other
  if (net != BEAR_GEN_NET_STOP && net != BEAR_GEN_NET_ROWS && net != BEAR_GEN_NET_MAT) return BEAR_ERR_INVALID_ARG;
  if ((prior != nullptr) != (net == BEAR_GEN_NET_ROWS) || (mat != nullptr) != (net == BEAR_GEN_NET_MAT)) return BEAR_ERR_INVALID_ARG;
  if (mat && width != 21) return BEAR_ERR_INVALID_ARG;
  gen_ref_args ref;
  memset(&ref, 0, sizeof(ref));
  if (!ref_params(tau, net_weight, eps, ref.prm) || n_ref >= SCR_ABSENT) return BEAR_ERR_INVALID_ARG;
  gen_args A;
  if (!gen_prepare(lag, width, rank, mode, map, h, van, true, prior != nullptr, n_table, seed, step0, n_steps, letters_stride, A))
    return BEAR_ERR_INVALID_ARG;
  if (n_seq == 0) return BEAR_OK;
  if (!gen_pointers_ok(table, counts, n_table, prior, keys, sample, left, n_seq, n_steps, letters, letters_stride) || !length ||
      !stopped || misaligned4(length) || (mat && misaligned8(mat)) ||
      (n_ref && (!ref_table || !ref_counts || misaligned8(ref_table) || misaligned4(ref_counts))))
    return BEAR_ERR_INVALID_ARG;
  ref.table = ref_table;
  ref.counts = ref_counts;
  ref.n_table = n_ref;
  ref.net = net;
  return gen_launch_ref(width, table, counts, n_table, prior, mat, keys, sample, left, length, stopped, n_seq, A, letters, codes, ref,
                        stream);
}

}  // extern "C"
