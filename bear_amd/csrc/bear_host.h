// bear_host.h -- internal: the host side that the units of libbear_hip share.
//
// One unit per kernel family, each the only one to include -- and so to emit -- the kernels it launches:
//   bear_hip.hip     status strings, the workspace, synthetic tables, samplers; the DM steps (rows, sorted,
//                    planned, reference-aware, ref-mix) and the plan itself
//   bear_linear.hip  k-mer packing, the paired lists, the linear AR head (fused step and rows, both also at rows of 21), the Adam launch
//   bear_cnn.hip     the convolutional AR head and its prefix levels / window tables; the head as rows of 21 and bear_net's step with it
//   bear_eval.hip    held-out evaluation (5- and 21-wide), the wide DM step and bear_ref's wide steps, the evaluation plan, the BMM marginal,
//                    the two-sample and the k-sample Bayes factors
//   (bear_score.hip, scoring under a sampled table, bear_shuffle.hip, the row shuffle, and bear_count.hip, counting, need nothing of
//   this file: bear_dev.h alone)
// What a unit needs of another goes through the declarations at the end of this file.
//
// Device memory and HIP errors, in every unit (bear_dev.h): a temporary sits in a dev_buf, which frees it when the function returns
// (or where the function says reset(): hipFree waits for the device); a long-lived struct keeps raw pointers, which kernels and
// views read, and is built either into dev_bufs that release() into it on success (bear_eval_plan, the pairing of a plan, levels,
// window tables, bear_kmer_sort) or under a guard over its free function (bear_plan, bear_ws).  A failed HIP call leaves through
// HIP_TRY: the error in bear_last_hip_error(), out of device memory as BEAR_ERR_NOMEM, anything else as BEAR_ERR_HIP.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <memory>
#include <new>
#include <vector>

#include "bear_common.h"
#include "bear_dev.h"
#include "bear_levels.h"
#include "plan_common.h"

#define BEAR_INTERNAL __attribute__((visibility("hidden")))

// ------------------------------------------------------------------ arguments
static inline int check_ws(const bear_ws *ws) {
  if (!ws) return BEAR_ERR_INVALID_ARG;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return BEAR_ERR_NO_DEVICE;
  if (dev != ws->device) return BEAR_ERR_WRONG_DEVICE;
  return BEAR_OK;
}

static inline bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }
static inline bool misaligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }
static inline bool wide_width_ok(int width) { return width == 5 || width == 21; }   // rows of the nucleotide / protein alphabet

// F(A, B) with two run-time flags as compile-time booleans: the template parameters of a kernel (AR mode, gradient rows)
#define BEAR_DISPATCH_2(a, b, F) \
  do {                           \
    if (a) {                     \
      if (b) F(true, true);      \
      else F(true, false);       \
    } else {                     \
      if (b) F(false, true);     \
      else F(false, false);      \
    }                            \
  } while (0)

// F(A) with one run-time flag as a compile-time boolean
#define BEAR_DISPATCH_1(a, F) \
  do {                        \
    if (a) F(true);           \
    else F(false);            \
  } while (0)

// `launch` with the row width of an entry that takes one (wide_width_ok: 5 or 21) as the compile-time integer W: the first template
// parameter of the width-generic kernels.  Around a BEAR_DISPATCH_1 / _2 the flags come behind it.
#define BEAR_DISPATCH_W(width, launch) \
  do {                                 \
    if ((width) == 21) {               \
      constexpr int W = 21;            \
      launch;                          \
    } else {                           \
      constexpr int W = 5;             \
      launch;                          \
    }                                  \
  } while (0)

// ------------------------------------------------------------------ kernel parameters by value (bear_common.h, bear_params)
// every field a kernel does not read is zero.  params_eps: the constants come from device-resident parameters (bear_params_of)
static inline bear_params params_eps(double eps) {
  bear_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.eps = eps;
  return prm;
}
static inline bear_params params_net(double h_signed, double eps) {
  bear_params prm = params_eps(eps);
  prm.inv_h = 1.0 / exp(h_signed);
  return prm;
}
static inline bear_params params_ref(double h_signed, double tau_signed, double nu_signed, double eps) {
  bear_params prm = params_net(h_signed, eps);
  const double tau = exp(tau_signed), nw = exp(nu_signed);
  prm.E = exp(-tau);
  prm.tauE = tau * prm.E;
  prm.tau = tau;
  prm.V = 1.0 / (nw + 1.0);
  prm.nw = nw;
  return prm;
}

// ------------------------------------------------------------------ grids
// Every grid-stride launch takes min(work, cap) blocks, and at least one.  The block partials are summed in a fixed order PER GRID:
// a different grid is different bits, so a cap is part of a kernel's results, not a tuning detail of its call site.
static inline int grid_capped(uint64_t work, uint64_t cap) {
  const uint64_t g = work < cap ? work : cap;
  return g < 1 ? 1 : (int)g;
}
// ... the cap of a launch whose blocks each leave a row of ws->partials: per_cu resident blocks, within the buffer
static inline uint64_t ws_blocks(const bear_ws *ws, int per_cu) {
  const uint64_t g = (uint64_t)ws->num_cu * per_cu;
  return g > (uint64_t)ws->max_blocks ? (uint64_t)ws->max_blocks : g;
}
// ... the grid of a wide row kernel: tiles of `tile` contexts, per_cu resident blocks
static inline int wide_grid(const bear_ws *ws, uint64_t n_rows, uint64_t tile, int per_cu) {
  return grid_capped((n_rows + tile - 1) / tile, ws_blocks(ws, per_cu));
}

// the planned step kernels: one resident 1024-thread block per CU (LDS ring; the half-tile build: two of 512)
static inline int grid_plan(const bear_ws *ws, uint64_t n_tiles) { return grid_capped(n_tiles, ws_blocks(ws, PLN_BLOCKS_PER_CU)); }

// Lets each of `kernels` take `bytes` of dynamic LDS (beyond the 64 KiB a launch gets unasked): once per workspace, *_ws_setup.
#define BEAR_KFN(...) reinterpret_cast<const void *>(__VA_ARGS__)
static inline int allow_dynamic_lds(std::initializer_list<const void *> kernels, size_t bytes) {
  for (const void *fn : kernels) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return BEAR_OK;
}

// ------------------------------------------------------------------ one launch per reduce (bear_common.h)
// a fresh stamp for the launch that is about to use ws->arrive (bear_arrival, bear_common.h); 0 is the word's idle value
static inline bear_arrival ws_arrival(bear_ws *ws) {
  if (++ws->epoch == 0u) ws->epoch = 1u;
  return bear_arrival{ws->arrive, ws->epoch};
}

static inline bear_step_io ws_io(bear_ws *ws, const double *theta, int kind, double *out) {
  const bear_arrival a = ws_arrival(ws);
  bear_step_io io;
  io.theta = theta;
  io.kind = kind;
  io.epoch = a.epoch;
  io.out = out;
  io.arrive_word = a.word;
  return io;
}

// BEAR_AMD_DETERMINISTIC=1: parameter gradients that are bit-identical from run to run (kernels_linear.h: fixed-point gradient
// tables; cnn_backward_grid: one wave per block).  Read per call: a process may switch it between steps (tests).
static inline bool bear_deterministic() {
#ifdef BEAR_DET_BUILD      // libbear_hip_det.so: everything deterministic, always (plan_common.h, PLN_FOR_UNITS)
  return true;
#else
  const char *e = getenv("BEAR_AMD_DETERMINISTIC");
  return e && e[0] && e[0] != '0';
#endif
}

// ---- optimizer step in two halves: the shard's reduce (constants from theta -> planned kernel -> finalize into `packed`) and the
// apply (tf.keras Adam on theta from packed).  One rank runs them back to back (bear_*_train_step_f64, graph-capturable);
// several ranks put ONE all-reduce of `packed` between them (bear_net.py:278-290) -- no host round trip either way.
static const bear_apply_io NO_APPLY = {};      // theta == NULL: the launch only reduces

static inline bear_apply_io make_apply(double *theta, int n_theta, double *adam_m, double *adam_v, double *adam_t, double learning_rate,
                                       double scale, int train_ar, double *loss_buf, uint64_t loss_cap) {
  bear_apply_io A;
  A.theta = theta;
  A.m = adam_m;
  A.v = adam_v;
  A.t_state = adam_t;
  A.loss_buf = loss_buf;
  A.loss_cap = (unsigned long long)loss_cap;
  A.lr = learning_rate;
  A.scale = scale;
  A.n_theta = n_theta;
  A.train_ar = train_ar;
  return A;
}

// BEAR_AMD_TWO_LAUNCH_STEP=1: bear_*_train_step_f64 as reduce + bear_train_apply_f64 again (two launches; tests compare the two forms)
static inline bool two_launch_step() {
  const char *e = getenv("BEAR_AMD_TWO_LAUNCH_STEP");
  return e && e[0] && e[0] != '0';
}

// ------------------------------------------------------------------ plans
// Created, freed and walked by bear_hip.hip; the other families attach what their step needs and own those fields.
struct rpl_item;
struct bear_plan {
  // ---- bear_hip.hip (bear_plan_create): the sorted encoding of the count table
  int device;
  int ncol;
  uint64_t n_rows;
  const uint32_t *counts;  // the buffer the plan was built from (identity check only)
  pln_tile *tiles;
  unsigned char *stream;
  pln_heavy_col *heavy_col;
  pln_heavy_row *heavy_row;
  uint64_t *heavy_stop;
  unsigned long long *hist;  // [64]
  uint16_t *live;            // five-column plans: per-tile lists of the contexts that hold counts (plan_live_kernel)
  uint64_t n_tiles;
  uint64_t n_heavy[3];
  int rows_ref;              // bear_plan_create_ref: the DENSE form (a table of large counts: nothing kept per item, dm_ref_rows_kernel)
  uint64_t n_live_rows;      // five-column plans: contexts that hold any count (the kernels that walk `live` skip the lists when all do)
  double count_total[3];     // of the table (all five columns): sum of all counts, cells that hold one, largest count
  double count_bound[3];     // the same of everything that is added into one gradient (bear_plan_set_count_bound; default: count_total)
  uint64_t bytes;            // of everything the plan holds: whoever attaches or drops something accounts for it here
  // ---- bear_cnn.hip (bear_plan_attach_cnn_levels): prefix levels of the (k-mer-sorted) contexts at cnn_codes for the convolutional
  // step (kernels_cnn.h, cnn_level_io); levels[k - 1] = level k, k = 1 .. n_cnn_levels
  bear_level_dev cnn_levels[CNN_MAX_LAG];
  int n_cnn_levels, cnn_lag, cnn_fw;
  // ... and window tables (bear_window_dev) per level k = 0 (the contexts) .. n_cnn_levels: cnn_win[k][q], q < n_cnn_win[k], are the
  // tables of the LAST n_cnn_win[k] positions of the level's range, ascending
  bear_window_dev cnn_win[CNN_MAX_LAG + 1][CNN_MAX_WIN];
  int n_cnn_win[CNN_MAX_LAG + 1];
  int n_cnn_windows;         // all of them
  const uint64_t *cnn_codes;
  // ---- bear_linear.hip (bear_plan_pair_contexts): the paired form of `live` for the index words at pair_codes (kernels_linear.h),
  // and the plan's tiles sorted into those that took it (tiles_p) and those that keep their plain list (tiles_u), each followed by
  // PLN_DESC_PAD zeroed descriptors; spare word of a descriptor = tile number << 32 | entries of the paired list
  uint16_t *live2;
  pln_tile *tiles_p, *tiles_u;
  uint64_t n_tiles_p, n_tiles_u;
  const uint64_t *pair_codes;
  int pair_lag;
  // ---- bear_hip.hip (bear_plan_create_ref): the reference-aware extension (kernels_refplan.h)
  const uint32_t *ref;
  rpl_item *ref_items;
  uint64_t n_ref_items, n_heavy0;
  unsigned long long *hist0;   // [RPL_NKEY], inside the allocation hist0_base
  unsigned long long *hist0_base;
  uint32_t *heavy0;
  double *sum0;
};

static inline pln_view plan_view(const bear_plan *p) {
  pln_view v;
  v.tiles = p->tiles;
  v.stream = p->stream;
  v.heavy_col = p->heavy_col;
  v.heavy_row = p->heavy_row;
  v.heavy_stop = p->heavy_stop;
  v.hist = p->hist;
  v.hist_big = p->hist + 2 * SRT_NKEY;
  v.big_in_hist = 1;
  v.live = p->live;
  v.live2 = p->live2;
  v.subset = 0;
  v.n_tiles = p->n_tiles;
  v.n_heavy_col = p->n_heavy[0];
  v.n_heavy_row = p->n_heavy[1];
  v.n_heavy_stop = p->n_heavy[2];
  return v;
}

// A step on a plan takes the table the plan was built from, on the workspace's device.  ncol: 5 (mode N) or 4 (mode R);
// or_rows: the entry also takes the dense form of a five-column plan (bear_plan_create_auto).
#define PLAN_ROWS 15      // ncol of that form: every entry that walks a plan's tiles and lists asks for 5 and so turns it away
static inline bool plan_is_rows(const bear_plan *p) { return p->ncol == PLAN_ROWS; }
static inline int check_plan_step(const bear_ws *ws, const bear_plan *plan, const uint32_t *counts, uint64_t n_rows, int ncol,
                                  bool or_rows = false) {
  if (plan->ncol != ncol && !(or_rows && plan_is_rows(plan))) return BEAR_ERR_INVALID_ARG;
  if (plan->counts != counts || plan->n_rows != n_rows || plan->device != ws->device) return BEAR_ERR_INVALID_ARG;
  return BEAR_OK;
}

// ------------------------------------------------------------------ across units
// bear_ws_create: each family sets the dynamic-LDS limit of its own kernels and allocates the buffers of the workspace that only it
// uses; a status (bear_last_hip_error).  What they allocated goes with the workspace (ws_release, bear_hip.hip).
BEAR_INTERNAL int linear_ws_setup(bear_ws *ws);      // lin_partials, lin_accum, linw_partials, linw_packed
BEAR_INTERNAL int cnn_ws_setup(bear_ws *ws);         // cnnw_partials (cnn_partials grows on demand: cnn_backward_grid)
BEAR_INTERNAL int eval_ws_setup(bear_ws *ws);        // eval_partials, eval_out
// plan_free (bear_hip.hip): each family drops the fields of a plan that it owns, and takes them off plan->bytes
BEAR_INTERNAL void plan_unpair(bear_plan *plan);            // bear_linear.hip: live2, tiles_p, tiles_u
BEAR_INTERNAL void plan_drop_cnn_levels(bear_plan *plan);   // bear_cnn.hip: cnn_levels, cnn_win

extern "C" {   // (bear_hip.hip defines everything inside one such block)
// bear_hip.hip: the planned mode-N step with gradient rows (the convolutional step runs it between its forward and backward passes)
BEAR_INTERNAL int launch_prior_plan_grad(bear_ws *ws, const bear_plan *plan, const double *prior, const bear_params &prm,
                                         const double *theta, int train_ar, int prior_normalized, double *out, double *grad_prior,
                                         hipStream_t s);
// bear_linear.hip: adam_vec_kernel, the apply half of a step as a launch of its own
BEAR_INTERNAL int launch_train_apply(double *theta, int n_theta, const double *packed, double *adam_m, double *adam_v, double *adam_t,
                                     double learning_rate, double scale, int train_ar, double *loss_buf, uint64_t loss_cap, hipStream_t s);
}  // extern "C"
