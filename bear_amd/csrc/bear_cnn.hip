// bear_cnn.hip -- the convolutional AR head (kernels_cnn.h): forward and backward passes, the prefix levels and window tables a
// plan keeps for it (bear_levels.h), and its training step around the planned DM step of bear_hip.hip; the head as rows at the
// protein alphabet's width and bear_net's step with it there in two launches (kernels_cnn_wide.h).  The other units: bear_host.h.
#include "bear_host.h"
#include "kernels_cnn.h"
#include "kernels_cnn_wide.h"

static const size_t CU_LDS_BYTES = 160u * 1024u;      // the LDS of a CU: what one block may take

int cnn_ws_setup(bear_ws *ws) {
  int st = allow_dynamic_lds({BEAR_KFN(cnn_backward_head_kernel)}, cnh_lds_bytes());
  if (st != BEAR_OK) return st;
  // (linear in the filter width at a given lag: the ends are the extremes)
  st = allow_dynamic_lds({BEAR_KFN(cnn_wide_forward_kernel)},
                         std::max(cnw_fwd_lds(CNN_WIDE_MAX_LAG, CNN_WIDE_MAX_LAG), cnw_fwd_lds(CNN_WIDE_MAX_LAG, 1)));
  if (st != BEAR_OK) return st;
  st = allow_dynamic_lds({BEAR_KFN(cnn_wide_backward_kernel<false>), BEAR_KFN(cnn_wide_backward_kernel<true>)},
                         std::max(cnw_bwd_lds(CNN_WIDE_MAX_LAG, CNN_WIDE_MAX_LAG), cnw_bwd_lds(CNN_WIDE_MAX_LAG, 1)));
  if (st != BEAR_OK) return st;
  // (the head kernel's block partials are two sums per block: ws->partials, as dm_wide_kernel's)
  st = allow_dynamic_lds({BEAR_KFN(cnn_wide_head_dm_kernel<false>), BEAR_KFN(cnn_wide_head_dm_kernel<true>)},
                         std::max(cnw_head_lds(CNN_WIDE_MAX_LAG, CNN_WIDE_MAX_LAG), cnw_head_lds(CNN_WIDE_MAX_LAG, 1)));
  if (st != BEAR_OK) return st;
  HIP_TRY(hipMalloc(&ws->cnnw_partials, sizeof(double) * CNW_MAX_TOTAL * WIDE_PARTIAL_ROWS(ws->num_cu, CNW_BWD_BLOCKS_PER_CU)));
  return BEAR_OK;
}

#ifdef CNN_STAMPS
extern "C" int bear_dbg_cnn_stamps(unsigned long long *host_out, int reset) {   // developer build only
  if (host_out) HIP_TRY(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(cnn_stamp_sums), sizeof(unsigned long long) * 8));
  if (reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(cnn_stamp_sums), z, sizeof(z)));
  }
  return BEAR_OK;
}
#endif

// the forward kernel over `groups` groups of 64 rows (or tiles of a plan, with their lists): a wave per group
static void launch_cnn_forward(const bear_ws *ws, const cnn_dims &D, const unsigned long long *codes, uint64_t n_rows, const double *params,
                               double *prior, double *t1_save, const pln_tile *tiles, const uint16_t *live_lists, uint64_t groups,
                               const cnn_level_io &io, hipStream_t s) {
  const int blocks = grid_capped((groups + CNN_THREADS / 64 - 1) / (CNN_THREADS / 64), (uint64_t)ws->num_cu * 16);
  hipLaunchKernelGGL(cnn_forward_kernel, dim3((unsigned)blocks), dim3(CNN_THREADS), cnn_fwd_lds_bytes(D.fw), s, codes, n_rows, D, params, prior,
                     t1_save, tiles, live_lists, groups, io);
}
// ... over all rows in groups of 64, no plan
static void launch_cnn_forward_rows(const bear_ws *ws, const cnn_dims &D, const unsigned long long *codes, uint64_t n_rows, const double *params,
                                    double *prior, double *t1_save, const cnn_level_io &io, hipStream_t s) {
  launch_cnn_forward(ws, D, codes, n_rows, params, prior, t1_save, nullptr, nullptr, (n_rows + 63) / 64, io, s);
}

static bool cnn_shape_ok(int lag, int fw, int nf, int l1) {
  return lag >= 1 && lag <= CNN_MAX_LAG && fw >= 1 && fw <= lag && nf == CNN_NF && l1 == CNN_L1;
}

static int cnn_check(const bear_ws *ws, int lag, int fw, int nf, int l1) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  return cnn_shape_ok(lag, fw, nf, l1) ? BEAR_OK : BEAR_ERR_INVALID_ARG;
}

int bear_cnn_param_count(int lag, int filter_width, int num_filters, int layer1_width) {
  if (!cnn_shape_ok(lag, filter_width, num_filters, layer1_width)) return BEAR_ERR_INVALID_ARG;
  return cnn_make_dims(lag, filter_width).total;
}

int bear_cnn_forward_f64(bear_ws *ws, const uint64_t *kmer_code, uint64_t n_rows, int lag, int filter_width, int num_filters,
                         int layer1_width, const double *params, double *prior, double *t1_save, void *stream) {
  int st = cnn_check(ws, lag, filter_width, num_filters, layer1_width);
  if (st != BEAR_OK) return st;
  if (n_rows == 0) return BEAR_OK;
  if (!kmer_code || !params || !prior || misaligned(t1_save) || misaligned8(prior)) return BEAR_ERR_INVALID_ARG;
  const cnn_dims D = cnn_make_dims(lag, filter_width);
  launch_cnn_forward_rows(ws, D, reinterpret_cast<const unsigned long long *>(kmer_code), n_rows, params, prior, t1_save, cnn_all_positions(D),
                          static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

static bool cnn_parts_form_forced_off() {      // BEAR_CNN_BACKWARD=1: the 64-context form of the backward kernel (developer A/B runs, tests)
  const char *force = getenv("BEAR_CNN_BACKWARD");
  return force && force[0] == '1';
}

// The backward pass's launch geometry.  cnn_backward_parts_kernel<2>: two lanes per context, eight waves of 32-context tiles (two
// per SIMD), when the staging fits next to the filter, parameter and gradient images (every reference config); otherwise
// cnn_backward_kernel: 64-context tiles, one wave per SIMD (as many of four as fit), and no position range.
struct cnn_backward_geom {
  bool parts;         // the form
  int waves;          // per block
  size_t lds;
  uint64_t blocks;    // rows of the partial buffer the finalize reads
  uint64_t rows_per_block() const { return (uint64_t)(parts ? cnnq<2>::TILE : 64) * (uint64_t)waves; }
  int allow_lds() const {      // (not inside a stream capture)
    return allow_dynamic_lds({parts ? BEAR_KFN(cnn_backward_parts_kernel<2>) : BEAR_KFN(cnn_backward_kernel)}, lds);
  }
};
// sizes the block-partial buffer of the CNN backward pass; *g is the geometry.  With may_alloc == 0 (inside a stream capture) a
// buffer that is too small is an error: call bear_cnn_reserve first.
static int cnn_backward_grid(bear_ws *ws, const cnn_dims &D, uint64_t n_rows, cnn_backward_geom *g, hipStream_t s, int may_alloc) {
  // BEAR_AMD_DETERMINISTIC: ONE wave per block.  The block's gradient image takes LDS floating-point atomics from all its waves,
  // in whatever order they get there; with one wave the adds happen in program order, the blocks' images are summed in a fixed
  // order anyway (cnn_finalize_kernel) -- two runs of a step are bit-identical, at an eighth of the waves per CU.
  const bool det = bear_deterministic();
  g->parts = cnnq_lds_bytes(D, cnnq<2>::WAVES) <= CU_LDS_BYTES && !cnn_parts_form_forced_off();
  if (g->parts) {
    g->waves = det ? 1 : cnnq<2>::WAVES;
    g->lds = cnnq_lds_bytes(D, g->waves);
  } else {
    g->waves = det ? 1 : 4;
    while (g->waves > 1 && cnn_bwd_lds_bytes(D, g->waves) > CU_LDS_BYTES) g->waves >>= 1;
    g->lds = cnn_bwd_lds_bytes(D, g->waves);
  }
  if (g->lds > CU_LDS_BYTES) return BEAR_ERR_INVALID_ARG;
  g->blocks = (uint64_t)grid_capped((n_rows + g->rows_per_block() - 1) / g->rows_per_block(), (uint64_t)ws->num_cu);
  const size_t need = (size_t)g->blocks * D.total;
  if (ws->cnn_partials_cap < need) {
    if (!may_alloc) return BEAR_ERR_INVALID_ARG;
    HIP_TRY(hipStreamSynchronize(s));
    (void)hipFree(ws->cnn_partials);        // the smaller buffer goes first: the two never stand side by side
    ws->cnn_partials = nullptr;
    ws->cnn_partials_cap = 0;
    HIP_TRY(hipMalloc(&ws->cnn_partials, sizeof(double) * need));
    ws->cnn_partials_cap = need;
  }
  return BEAR_OK;
}

// live_plan [nullable]: a five-column plan of the table -- the part kernel then walks its lists of contexts that hold counts
static int launch_cnn_backward(bear_ws *ws, const cnn_dims &D, const uint64_t *kmer_code, uint64_t n_rows, const double *params,
                               const double *t1_save, const double *prior, const double *grad_prior, double *grad_params, hipStream_t s,
                               int may_alloc, const bear_plan *live_plan = nullptr) {
  cnn_backward_geom g;
  int st = cnn_backward_grid(ws, D, n_rows, &g, s, may_alloc);
  if (st != BEAR_OK) return st;
  if (may_alloc && (st = g.allow_lds()) != BEAR_OK) return st;
  const unsigned long long *kc = reinterpret_cast<const unsigned long long *>(kmer_code);
  if (g.parts) {
    const bool lists = live_plan && live_plan->live && live_plan->n_live_rows < n_rows;   // all rows live: plain groups of rows
    const uint64_t groups = lists ? live_plan->n_tiles : (n_rows + cnnq<2>::TILE - 1) / cnnq<2>::TILE;
    hipLaunchKernelGGL(cnn_backward_parts_kernel<2>, dim3((unsigned)g.blocks), dim3(64 * g.waves), g.lds, s, kc, n_rows, D, params, t1_save, prior,
                       grad_prior, ws->cnn_partials, lists ? live_plan->tiles : nullptr, lists ? live_plan->live : nullptr, groups,
                       cnn_all_positions(D));
  }
  else
    hipLaunchKernelGGL(cnn_backward_kernel, dim3((unsigned)g.blocks), dim3(64 * g.waves), g.lds, s, kc, n_rows, D, params, t1_save, prior,
                       grad_prior, ws->cnn_partials);
  hipLaunchKernelGGL(cnn_finalize_kernel, dim3((D.total + 3) / 4), dim3(256), 0, s, ws->cnn_partials, (int)g.blocks, D.total, grad_params);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_cnn_backward_f64(bear_ws *ws, const uint64_t *kmer_code, uint64_t n_rows, int lag, int filter_width, int num_filters,
                          int layer1_width, const double *params, const double *t1_save, const double *prior,
                          const double *grad_prior, double *grad_params, void *stream) {
  int st = cnn_check(ws, lag, filter_width, num_filters, layer1_width);
  if (st != BEAR_OK) return st;
  if (!params || !grad_params) return BEAR_ERR_INVALID_ARG;
  if (n_rows && (!kmer_code || !t1_save || !prior || !grad_prior || misaligned(t1_save))) return BEAR_ERR_INVALID_ARG;
  const cnn_dims D = cnn_make_dims(lag, filter_width);
  return launch_cnn_backward(ws, D, kmer_code, n_rows, params, t1_save, prior, grad_prior, grad_params, static_cast<hipStream_t>(stream), 1);
}

int bear_cnn_reserve(bear_ws *ws, uint64_t n_rows, int lag, int filter_width, int num_filters, int layer1_width) {
  int st = cnn_check(ws, lag, filter_width, num_filters, layer1_width);
  if (st != BEAR_OK) return st;
  cnn_backward_geom g;
  st = cnn_backward_grid(ws, cnn_make_dims(lag, filter_width), n_rows, &g, nullptr, 1);
  if (st != BEAR_OK) return st;
  return g.allow_lds();
}

// ---- prefix levels and window tables of a plan (kernels_cnn.h, cnn_level_io; bear_plan_attach_cnn_levels)
// "the plan's levels and tables were built from these codes at this lag and filter width"
static bool cnn_plan_has_levels_for(const bear_plan *plan, const uint64_t *kmer_code, int lag, int fw) {
  return (plan->n_cnn_levels > 0 || plan->n_cnn_windows > 0) && plan->cnn_codes == kmer_code && plan->cnn_lag == lag && plan->cnn_fw == fw;
}
// level k as the walks see it; k = 0: the contexts, whose codes and rows buffer come from the caller
struct cnn_level_view {
  const unsigned long long *codes;
  uint64_t n;
  double *rows;         // [n][16] layer-1 sums (forward) / dT1 rows (backward)
  int letters;          // prefix length
};
static cnn_level_view cnn_contexts(const uint64_t *kmer_code, uint64_t n_rows, double *t1_buf, int lag) {
  return {reinterpret_cast<const unsigned long long *>(kmer_code), n_rows, t1_buf, lag};
}
static cnn_level_view cnn_level(const bear_plan *plan, int k, const cnn_level_view &contexts) {
  if (k == 0) return contexts;
  const bear_level_dev &lv = plan->cnn_levels[k - 1];
  return {lv.codes, lv.n, lv.rows, lv.letters};
}
// Level k's rows are prefixes of L_k letters (L_0 = lag: the contexts): it evaluates the positions whose window [p, p + fw) lies
// inside its prefix but not inside the next level's shorter one -- p + fw in (L_{k+1}, L_k]; the last level takes what is left.
static cnn_level_io cnn_level_positions(const bear_plan *plan, const cnn_dims &D, int k) {
  const cnn_level_view ctx = cnn_contexts(nullptr, 0, nullptr, D.lag);
  cnn_level_io io = cnn_all_positions(D);
  io.p_hi = cnn_level(plan, k, ctx).letters - D.fw + 1;
  io.p_lo = k == plan->n_cnn_levels ? 0 : cnn_level(plan, k + 1, ctx).letters - D.fw + 1;
  io.head = k == 0;
  io.p_hi -= plan->n_cnn_win[k];          // the level's last positions come from its window tables
  return io;
}
// the launch over the rows of a window table: its one position, no head, no parent
static cnn_level_io cnn_window_positions(const cnn_dims &D, const bear_window_dev &wt) {
  cnn_level_io io = cnn_all_positions(D);
  io.p_lo = wt.pos;
  io.p_hi = io.p_lo + 1;
  io.head = 0;
  return io;
}
// what level k's rows put their layer-1 sums together from besides their own positions: the parent level's rows and the window tables
static void cnn_level_sources(const bear_plan *plan, int k, cnn_level_io &io) {
  if (k < plan->n_cnn_levels) {
    io.t1_parent = plan->cnn_levels[k].rows;                 // level k + 1
    io.parent = plan->cnn_levels[k].parent_of_below;
  }
  io.n_win = plan->n_cnn_win[k];
  for (int q = 0; q < plan->n_cnn_win[k]; ++q) {
    io.win_rows[q] = plan->cnn_win[k][q].rows;
    io.win_row_of[q] = plan->cnn_win[k][q].row_of_context;
  }
}
// a launch with no position of its own (all of them come from the parent level and the window tables)
static bool cnn_no_own_positions(const cnn_level_io &io) { return io.p_lo >= io.p_hi; }
// the contexts evaluate no position themselves: the head-only kernels (kernels_cnn.h) take level 0, forward and backward
static bool cnn_level0_head_only(const cnn_level_io &io0) { return cnn_no_own_positions(io0) && !getenv("BEAR_AMD_CNN_NO_HEAD_KERNEL"); }

static int cnn_forward_levels(bear_ws *ws, const bear_plan *plan, const cnn_dims &D, const uint64_t *kmer_code, uint64_t n_rows,
                              const double *params, double *prior, double *t1_buf, hipStream_t s);
// ---- the convolutional step over prefix levels: the forward kernel once per level from the shortest
// prefixes down to the contexts, the planned DM kernel with gradient rows, the backward kernel once per level the other way with a
// row-sum launch in between; block partials accumulate in the workspace's buffer (stream order), one finalize at the end.
// Level k < K evaluates position P - 1 - k, the last level K the positions [0, P - K).
static int cnn_train_reduce_levels(bear_ws *ws, const bear_plan *plan, const cnn_dims &D, const uint64_t *kmer_code, uint64_t n_rows,
                                   const double *theta, double *prior_buf, double *t1_buf, double *grad_rows_buf, double eps, int train_ar,
                                   double *packed, hipStream_t s) {
  const int K = plan->n_cnn_levels;
  const double *params = theta + 1;
  cnn_backward_geom bw;
  int st = cnn_backward_grid(ws, D, n_rows, &bw, s, 0);
  if (st != BEAR_OK) return st;
  if (!bw.parts) return BEAR_ERR_INVALID_ARG;      // (attach refuses shapes whose staging does not fit: not reached)
  const cnn_level_view ctx = cnn_contexts(kmer_code, n_rows, t1_buf, D.lag);
  // Level 0 evaluates no position itself: the forward pass then keeps no layer-1 sums of the contexts -- the backward pass puts
  // them together again from the same rows (cnn_gather_t1)
  const cnn_level_io io0 = cnn_level_positions(plan, D, 0);
  const bool recompute_t1 = cnn_no_own_positions(io0) && !getenv("BEAR_AMD_CNN_KEEP_T1");
  const double *t1_of_contexts = recompute_t1 ? nullptr : t1_buf;
  st = cnn_forward_levels(ws, plan, D, kmer_code, n_rows, params, prior_buf, recompute_t1 ? nullptr : t1_buf, s);
  if (st != BEAR_OK) return st;
  st = launch_prior_plan_grad(ws, plan, prior_buf, params_eps(eps), theta, train_ar, 1, packed, grad_rows_buf, s);   // softmax rows: normalised
  if (st != BEAR_OK) return st;
  bool first_launch = true;      // the first backward launch writes every row of the partial buffer the finalize reads, the others add
  auto next_launch = [&](cnn_level_io &io) {
    io.accumulate = first_launch ? 0 : 1;
    first_launch = false;
  };
  auto backward = [&](const unsigned long long *codes, uint64_t n, const double *t1_in, cnn_level_io io) {
    const uint64_t blocks = first_launch ? bw.blocks : (uint64_t)grid_capped((n + bw.rows_per_block() - 1) / bw.rows_per_block(), bw.blocks);
    next_launch(io);
    hipLaunchKernelGGL(cnn_backward_parts_kernel<2>, dim3((unsigned)blocks), dim3(64 * bw.waves), bw.lds, s, codes, n, D, params, t1_in, prior_buf,
                       grad_rows_buf, ws->cnn_partials, static_cast<const pln_tile *>(nullptr), static_cast<const uint16_t *>(nullptr),
                       (n + cnnq<2>::TILE - 1) / cnnq<2>::TILE, io);
  };
  for (int k = 0; k <= K; ++k) {
    cnn_level_io io = cnn_level_positions(plan, D, k);
    const cnn_level_view lv = cnn_level(plan, k, ctx);
    const int W = plan->n_cnn_win[k];
    if (k > 0) {        // this level's dT1 rows = the sums of its children's
      const int sb = grid_capped((lv.n * (CNN_L1 / 2) + 255) / 256, (uint64_t)ws->num_cu * 32);
      hipLaunchKernelGGL(cnn_level_sum_kernel, dim3((unsigned)sb), dim3(256), 0, s, cnn_level(plan, k - 1, ctx).rows,
                         plan->cnn_levels[k - 1].child_start, lv.n, lv.rows);
    }
    io.dT1 = (k == 0 && (K > 0 || W > 0)) ? t1_buf : (k > 0 ? lv.rows : nullptr);   // level 0 leaves its dT1 rows where its t1 rows were
    if (k == 0 && recompute_t1) cnn_level_sources(plan, 0, io);
    // (a level of prefixes whose positions all come from window tables has nothing to do itself: its dT1 rows feed the tables below)
    if (k == 0 && cnn_level0_head_only(io)) {      // always the step's first backward launch
      next_launch(io);
      hipLaunchKernelGGL(cnn_backward_head_kernel, dim3((unsigned)bw.blocks), dim3(CNH_WAVES * 64), cnh_lds_bytes(), s, lv.n, D, params,
                         t1_of_contexts, prior_buf, grad_rows_buf, ws->cnn_partials, io);
    } else if (k == 0 || !cnn_no_own_positions(io)) {
      backward(lv.codes, lv.n, k == 0 ? t1_of_contexts : t1_buf, io);
    }
    for (int q = 0; q < W; ++q) {      // the level's window tables: a window's dT1 row = the sum of its rows' (anywhere in the level)
      const bear_window_dev &wt = plan->cnn_win[k][q];
      const int sb = grid_capped((wt.n + 3) / 4, (uint64_t)ws->num_cu * 8);
      hipLaunchKernelGGL(cnn_window_sum_kernel, dim3((unsigned)sb), dim3(256), 0, s, lv.rows, wt.perm, wt.child_start, wt.n, wt.rows);
      cnn_level_io wio = cnn_window_positions(D, wt);
      wio.dT1 = wt.rows;
      backward(wt.codes, wt.n, t1_buf, wio);
    }
  }
  hipLaunchKernelGGL(cnn_finalize_kernel, dim3((D.total + 3) / 4), dim3(256), 0, s, ws->cnn_partials, (int)bw.blocks, D.total, packed + 2);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

// Prefix levels of the plan's (k-mer-sorted) contexts for the convolutional step: see include/bear_hip.h.
void plan_drop_cnn_levels(bear_plan *plan) {
  for (int k = 0; k < plan->n_cnn_levels; ++k) {
    plan->bytes -= plan->cnn_levels[k].bytes;
    bear_level_free(&plan->cnn_levels[k]);
  }
  for (int k = 0; k <= CNN_MAX_LAG; ++k) {
    for (int q = 0; q < plan->n_cnn_win[k]; ++q) {
      plan->bytes -= plan->cnn_win[k][q].bytes;
      bear_window_free(&plan->cnn_win[k][q]);
    }
    plan->n_cnn_win[k] = 0;
  }
  plan->n_cnn_levels = 0;
  plan->n_cnn_windows = 0;
  plan->cnn_codes = nullptr;
}

int bear_plan_attach_cnn_levels(bear_plan *plan, const uint64_t *kmer_code, int lag, int filter_width, int *n_levels, void *stream) {
  if (n_levels) *n_levels = 0;
  if (!plan || plan->ncol != 5 || !cnn_shape_ok(lag, filter_width, CNN_NF, CNN_L1)) return BEAR_ERR_INVALID_ARG;
  if (plan->n_rows && (!kmer_code || misaligned(kmer_code))) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipStreamSynchronize(s));
  plan_drop_cnn_levels(plan);                          // a plan holds one set of levels: the new one replaces it
  const cnn_dims D = cnn_make_dims(lag, filter_width);
  // (the part form of the backward kernel is the one with a position range: shapes whose staging does not fit keep the plain step)
  if (cnnq_lds_bytes(D, cnnq<2>::WAVES) > CU_LDS_BYTES) return BEAR_OK;
  if (plan->n_rows < 2 || plan->n_live_rows != plan->n_rows) return BEAR_OK;   // (the step walks the plan's lists instead: no levels)
  const unsigned long long *below = reinterpret_cast<const unsigned long long *>(kmer_code);
  uint64_t n_below = plan->n_rows;
  int misses = 0;
  const double keep_ratio = 0.6;
  for (int k = 1; k <= D.P - 1 && misses < 3; ++k) {
    bear_level_dev lv;
    const int st = bear_level_build(below, n_below, lag - k, &lv, s);
    if (st != BEAR_OK) {
      plan_drop_cnn_levels(plan);                      // the levels built so far go with it: the plan is as it was without levels
      return st;
    }
    // a level pays when it is clearly smaller than the last one kept (a position per row either way, plus the row traffic); a
    // prefix length that does not (a sparser table: its prefixes of lag - 1 letters hardly repeat) is skipped -- the level below
    // then evaluates that position too -- and the next shorter one is tried against the same rows
    if ((double)lv.n > keep_ratio * (double)n_below) {
      bear_level_free(&lv);
      ++misses;
      continue;
    }
    misses = 0;
    lv.bytes = lv.n * (8 + 4 + 16 * 8) + 4 * n_below;
    plan->cnn_levels[plan->n_cnn_levels++] = lv;
    plan->bytes += lv.bytes;
    below = lv.codes;
    n_below = lv.n;
  }
  // Window tables, level by level (level 0 = the contexts): for the level's own positions, from the last one up, CNN_MAX_WIN at most,
  // each only while the level holds at least eight rows per distinct window (a table costs one position per window plus a 128-byte
  // gather per row and direction; a position evaluated per row costs ~25 times that gather).
  if (!getenv("BEAR_AMD_CNN_NO_WINDOWS")) {
    const cnn_level_view ctx = cnn_contexts(kmer_code, plan->n_rows, nullptr, lag);
    for (int k = 0; k <= plan->n_cnn_levels; ++k) {
      const cnn_level_view lv = cnn_level(plan, k, ctx);
      const cnn_level_io own = cnn_level_positions(plan, D, k);      // (no table attached yet: all the level's own positions)
      bear_window_dev built[CNN_MAX_WIN];
      int nb = 0;
      for (int p = own.p_hi - 1; p >= own.p_lo && nb < CNN_MAX_WIN && lv.n >= 64; --p) {
        bear_window_dev wt;
        const int st = bear_window_build(lv.codes, lv.n, p, filter_width, &wt, s);
        if (st != BEAR_OK) {
          for (int q = 0; q < nb; ++q) bear_window_free(&built[q]);
          plan_drop_cnn_levels(plan);
          return st;
        }
        if (wt.n * 8 > lv.n) {
          bear_window_free(&wt);
          break;
        }
        built[nb++] = wt;
      }
      for (int q = 0; q < nb; ++q) {         // ascending positions
        plan->cnn_win[k][q] = built[nb - 1 - q];
        plan->bytes += plan->cnn_win[k][q].bytes;
      }
      plan->n_cnn_win[k] = nb;
      plan->n_cnn_windows += nb;
    }
  }
  if (plan->n_cnn_levels || plan->n_cnn_windows) {
    plan->cnn_codes = kmer_code;
    plan->cnn_lag = lag;
    plan->cnn_fw = filter_width;
  }
  if (n_levels) *n_levels = plan->n_cnn_levels;
  return BEAR_OK;
}

int bear_plan_cnn_window_rows(const bear_plan *plan, uint64_t *rows_out, int *pos_out, int *level_out, int capacity) {
  if (!plan || (capacity > 0 && !rows_out)) return BEAR_ERR_INVALID_ARG;
  int t = 0;
  for (int k = 0; k <= plan->n_cnn_levels; ++k)
    for (int q = 0; q < plan->n_cnn_win[k]; ++q, ++t)
      if (t < capacity) {
        rows_out[t] = plan->cnn_win[k][q].n;
        if (pos_out) pos_out[t] = plan->cnn_win[k][q].pos;
        if (level_out) level_out[t] = k;
      }
  return plan->n_cnn_windows;
}

int bear_plan_cnn_level_rows(const bear_plan *plan, uint64_t *rows_out, int *letters_out, int capacity) {
  if (!plan || (capacity > 0 && !rows_out)) return BEAR_ERR_INVALID_ARG;
  for (int k = 0; k < plan->n_cnn_levels && k < capacity; ++k) {
    rows_out[k] = plan->cnn_levels[k].n;
    if (letters_out) letters_out[k] = plan->cnn_levels[k].letters;
  }
  return plan->n_cnn_levels;
}

// The forward pass alone over a plan's prefix levels (evaluation-style callers, bench.py): prior rows and the contexts' layer-1 sums.
static int cnn_forward_levels(bear_ws *ws, const bear_plan *plan, const cnn_dims &D, const uint64_t *kmer_code, uint64_t n_rows,
                              const double *params, double *prior, double *t1_buf, hipStream_t s) {
  const cnn_level_view ctx = cnn_contexts(kmer_code, n_rows, t1_buf, D.lag);
  for (int k = plan->n_cnn_levels; k >= 0; --k) {
    for (int q = 0; q < plan->n_cnn_win[k]; ++q) {          // the level's window tables first: one position over its distinct windows
      const bear_window_dev &wt = plan->cnn_win[k][q];
      launch_cnn_forward_rows(ws, D, wt.codes, wt.n, params, nullptr, wt.rows, cnn_window_positions(D, wt), s);
    }
    const cnn_level_view lv = cnn_level(plan, k, ctx);
    cnn_level_io io = cnn_level_positions(plan, D, k);
    cnn_level_sources(plan, k, io);
    if (k == 0 && cnn_level0_head_only(io)) {      // the head alone
      const int hb = grid_capped((lv.n + 32 * 16 - 1) / (32 * 16), (uint64_t)ws->num_cu * 2);
      hipLaunchKernelGGL(cnn_forward_head_kernel, dim3((unsigned)hb), dim3(1024), 0, s, lv.n, D, params, prior, t1_buf, io);
      continue;
    }
    launch_cnn_forward_rows(ws, D, lv.codes, lv.n, params, k == 0 ? prior : nullptr, lv.rows, io, s);
  }
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_cnn_forward_plan_f64(bear_ws *ws, const bear_plan *plan, const uint64_t *kmer_code, uint64_t n_rows, int lag, int filter_width,
                              int num_filters, int layer1_width, const double *params, double *prior, double *t1_save, void *stream) {
  int st = cnn_check(ws, lag, filter_width, num_filters, layer1_width);
  if (st != BEAR_OK) return st;
  if (!plan || plan->n_rows != n_rows || plan->device != ws->device) return BEAR_ERR_INVALID_ARG;
  if (n_rows == 0) return BEAR_OK;
  if (!kmer_code || !params || !prior || !t1_save || misaligned(t1_save) || misaligned8(prior)) return BEAR_ERR_INVALID_ARG;
  if (!cnn_plan_has_levels_for(plan, kmer_code, lag, filter_width) || getenv("BEAR_AMD_CNN_NO_LEVELS"))
    return bear_cnn_forward_f64(ws, kmer_code, n_rows, lag, filter_width, num_filters, layer1_width, params, prior, t1_save, stream);
  return cnn_forward_levels(ws, plan, cnn_make_dims(lag, filter_width), kmer_code, n_rows, params, prior, t1_save, static_cast<hipStream_t>(stream));
}

int bear_net_cnn_train_reduce_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const uint64_t *kmer_code, uint64_t n_rows,
                                  int lag, int filter_width, int num_filters, int layer1_width, const double *theta, double *prior_buf,
                                  double *t1_buf, double *grad_rows_buf, double eps, int train_ar, double *packed, void *stream) {
  int st = cnn_check(ws, lag, filter_width, num_filters, layer1_width);
  if (st != BEAR_OK) return st;
  if (!plan || !packed || !theta || !prior_buf || !t1_buf || !grad_rows_buf || !n_rows || !kmer_code) return BEAR_ERR_INVALID_ARG;
  if (check_plan_step(ws, plan, counts, n_rows, 5) != BEAR_OK) return BEAR_ERR_INVALID_ARG;
  if (misaligned(prior_buf) || misaligned(t1_buf) || misaligned(grad_rows_buf) || misaligned8(packed)) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const cnn_dims D = cnn_make_dims(lag, filter_width);
  const double *params = theta + 1;
  if (cnn_plan_has_levels_for(plan, kmer_code, lag, filter_width) && plan->n_live_rows == n_rows && !getenv("BEAR_AMD_CNN_NO_LEVELS") &&
      !cnn_parts_form_forced_off())
    return cnn_train_reduce_levels(ws, plan, D, kmer_code, n_rows, theta, prior_buf, t1_buf, grad_rows_buf, eps, train_ar, packed, s);
  {
    // only the contexts that hold training counts: the DM kernel reads nobody else's prior row (their gradient rows are zero).
    // Only together with the backward kernel that walks the same lists (shapes whose LDS does not fit take all rows in both).
    cnn_backward_geom bw;
    st = cnn_backward_grid(ws, D, n_rows, &bw, s, 0);
    if (st != BEAR_OK) return st;
    const bool lists = plan->live && bw.parts && plan->n_live_rows < n_rows;   // all rows live: plain groups of rows
    launch_cnn_forward(ws, D, reinterpret_cast<const unsigned long long *>(kmer_code), n_rows, params, prior_buf, t1_buf,
                       lists ? plan->tiles : nullptr, lists ? plan->live : nullptr, lists ? plan->n_tiles : (n_rows + 63) / 64,
                       cnn_all_positions(D), s);
  }
  st = launch_prior_plan_grad(ws, plan, prior_buf, params_eps(eps), theta, train_ar, 1, packed, grad_rows_buf, s);   // softmax rows: normalised
  if (st != BEAR_OK) return st;
  return launch_cnn_backward(ws, D, kmer_code, n_rows, params, t1_buf, prior_buf, grad_rows_buf, packed + 2, s, 0, plan);
}

int bear_net_cnn_train_step_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const uint64_t *kmer_code, uint64_t n_rows,
                                int lag, int filter_width, int num_filters, int layer1_width, double *theta, double *adam_m,
                                double *adam_v, double *adam_t, double *prior_buf, double *t1_buf, double *grad_rows_buf,
                                double *packed, double eps, int train_ar, double learning_rate, double scale, double *loss_buf,
                                uint64_t loss_cap, void *stream) {
  if (!adam_m || !adam_v || !adam_t) return BEAR_ERR_INVALID_ARG;
  int st = bear_net_cnn_train_reduce_f64(ws, plan, counts, kmer_code, n_rows, lag, filter_width, num_filters, layer1_width, theta, prior_buf,
                                         t1_buf, grad_rows_buf, eps, train_ar, packed, stream);
  if (st != BEAR_OK) return st;
  const cnn_dims D = cnn_make_dims(lag, filter_width);
  return launch_train_apply(theta, 1 + D.total, packed, adam_m, adam_v, adam_t, learning_rate, scale, train_ar, loss_buf, loss_cap,
                            static_cast<hipStream_t>(stream));
}

// ---- the convolutional AR function as rows at the protein alphabet's width (kernels_cnn_wide.h): int8 code rows, no plan ----------
static bool cnn_wide_shape_ok(int lag, int fw, int nf, int l1, int width) {
  return width == CNW_W && nf == CNN_NF && l1 == CNN_L1 && fw >= 1 && fw <= lag && lag <= CNN_WIDE_MAX_LAG;
}

int bear_cnn_param_count_wide(int lag, int filter_width, int num_filters, int layer1_width, int width) {
  if (!cnn_wide_shape_ok(lag, filter_width, num_filters, layer1_width, width)) return BEAR_ERR_INVALID_ARG;
  return cnw_make_dims(lag, filter_width).total;
}

// the backward grid is part of its result (the block partials are summed in a fixed order per grid); cnnw_partials holds its rows
static int cnnwide_bwd_grid(const bear_ws *ws, uint64_t n_rows) {
  return grid_capped((n_rows + CNW_BWD_TILE - 1) / CNW_BWD_TILE, (uint64_t)ws->num_cu * CNW_BWD_BLOCKS_PER_CU);
}

int bear_cnn_forward_wide_f64(bear_ws *ws, const int8_t *codes, uint64_t n_rows, int lag, int filter_width, int num_filters,
                              int layer1_width, int width, const double *params, double *prior, double *t1_save, void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!cnn_wide_shape_ok(lag, filter_width, num_filters, layer1_width, width) || !params || misaligned8(params)) return BEAR_ERR_INVALID_ARG;
  if (n_rows == 0) return BEAR_OK;
  if (!codes || !prior || misaligned(codes) || misaligned(prior) || misaligned(t1_save)) return BEAR_ERR_INVALID_ARG;
  const cnn_dims D = cnw_make_dims(lag, filter_width);
  // two resident blocks per CU where their LDS lets them in (short filters), else one; the rows do not depend on the grid
  const size_t lds = cnw_fwd_lds(lag, filter_width);
  const uint64_t per_cu = 2 * lds <= CU_LDS_BYTES ? 2 : 1;
  const int grid = grid_capped((n_rows + CNW_FWD_TILE - 1) / CNW_FWD_TILE, (uint64_t)ws->num_cu * per_cu);
  hipLaunchKernelGGL(cnn_wide_forward_kernel, dim3(grid), dim3(CNW_FWD_THREADS), lds, static_cast<hipStream_t>(stream), codes, n_rows, D,
                     params, prior, t1_save);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_cnn_backward_wide_f64(bear_ws *ws, const int8_t *codes, uint64_t n_rows, int lag, int filter_width, int num_filters,
                               int layer1_width, int width, const double *params, const double *t1_save, const double *prior,
                               const double *grad_prior, double *grad_params, void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!cnn_wide_shape_ok(lag, filter_width, num_filters, layer1_width, width) || !params || !grad_params || misaligned8(params) ||
      misaligned8(grad_params))
    return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const cnn_dims D = cnw_make_dims(lag, filter_width);
  if (n_rows == 0) {
    HIP_TRY(hipMemsetAsync(grad_params, 0, sizeof(double) * (size_t)D.total, s));
    return BEAR_OK;
  }
  if (!codes || !t1_save || !prior || !grad_prior) return BEAR_ERR_INVALID_ARG;
  if (misaligned(codes) || misaligned(t1_save) || misaligned(prior) || misaligned(grad_prior)) return BEAR_ERR_INVALID_ARG;
  hipLaunchKernelGGL(cnn_wide_backward_kernel<false>, dim3(cnnwide_bwd_grid(ws, n_rows)), dim3(CNW_BWD_THREADS), cnw_bwd_lds(lag, filter_width),
                     s, codes, n_rows, D, params, t1_save, prior, grad_prior, ws->cnnw_partials, ws_arrival(ws), grad_params, NO_APPLY);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

// ---- bear_net's step with the convolutional AR function at the protein alphabet's width (kernels_cnn_wide.h): head + backward ----
// the head kernel's grid is part of the two sums (block partials in ws->partials, summed in a fixed order per grid)
static int cnnwide_head_grid(const bear_ws *ws, uint64_t n_rows) { return wide_grid(ws, n_rows, CNW_HEAD_TILE, CNW_HEAD_BLOCKS_PER_CU); }

// The checks and the launches of all three entries.  theta != NULL: h_signed from the device-resident parameters (prm: eps only).
// sums [2] and grad [param count] are the two ends of `packed` in the reduce / step forms; `apply`: the backward block that writes
// the gradient's fixed-order sum runs the update on packed = grad - 2 behind it.  n_rows == 0: one block each, zeros (and the update).
static int cnn_wide_reduce(bear_ws *ws, const uint32_t *counts, const int8_t *codes, uint64_t n_rows, int lag, int fw, int nf, int l1,
                           int width, const double *params, const double *theta, const bear_params &prm, int train_ar, double *dz_buf,
                           double *t1_buf, double *sums, double *grad, hipStream_t s, const bear_apply_io &apply) {
  if (!cnn_wide_shape_ok(lag, fw, nf, l1, width)) return BEAR_ERR_INVALID_ARG;
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!params || !sums || !grad || (n_rows && (!counts || !codes || !dz_buf || !t1_buf))) return BEAR_ERR_INVALID_ARG;
  if (misaligned(counts) || misaligned(codes) || misaligned(dz_buf) || misaligned(t1_buf)) return BEAR_ERR_INVALID_ARG;
  if (misaligned8(params) || misaligned8(sums) || misaligned8(grad) || !(prm.eps >= 0.0)) return BEAR_ERR_INVALID_ARG;
  const cnn_dims D = cnw_make_dims(lag, fw);
  const bear_step_io io = ws_io(ws, theta, BEAR_THETA_NET, sums);
  const double2 *lt = reinterpret_cast<const double2 *>(ws->logtab);
#define CNN_WIDE_HEAD(AR)                                                                                                              \
  hipLaunchKernelGGL((cnn_wide_head_dm_kernel<AR>), dim3(cnnwide_head_grid(ws, n_rows)), dim3(CNW_HEAD_THREADS), cnw_head_lds(lag, fw), s, \
                     counts, codes, n_rows, D, params, prm, lt, t1_buf, dz_buf, ws->partials, io)
  BEAR_DISPATCH_1(train_ar, CNN_WIDE_HEAD);
#undef CNN_WIDE_HEAD
  // (a stamp of its own on the arrival words: the head's last block has left them at zero by the time this one starts)
  hipLaunchKernelGGL(cnn_wide_backward_kernel<true>, dim3(cnnwide_bwd_grid(ws, n_rows)), dim3(CNW_BWD_THREADS), cnw_bwd_lds(lag, fw), s, codes,
                     n_rows, D, params, t1_buf, dz_buf, static_cast<const double *>(nullptr), ws->cnnw_partials, ws_arrival(ws), grad, apply);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_dm_cnn_wide_f64(bear_ws *ws, const uint32_t *counts, const int8_t *codes, uint64_t n_rows, int lag, int filter_width,
                         int num_filters, int layer1_width, int width, const double *params, double h_signed, double eps, int train_ar,
                         double *dz_buf, double *t1_buf, double *out, double *grad_params, void *stream) {
  if (!isfinite(h_signed)) return BEAR_ERR_INVALID_ARG;
  return cnn_wide_reduce(ws, counts, codes, n_rows, lag, filter_width, num_filters, layer1_width, width, params, nullptr,
                         params_net(h_signed, eps), train_ar, dz_buf, t1_buf, out, grad_params, static_cast<hipStream_t>(stream), NO_APPLY);
}

int bear_net_cnn_train_reduce_wide_f64(bear_ws *ws, const uint32_t *counts, const int8_t *codes, uint64_t n_rows, int lag, int filter_width,
                                       int num_filters, int layer1_width, int width, const double *theta, double *dz_buf, double *t1_buf,
                                       double eps, int train_ar, double *packed, void *stream) {
  if (!theta || !packed || misaligned8(theta)) return BEAR_ERR_INVALID_ARG;
  return cnn_wide_reduce(ws, counts, codes, n_rows, lag, filter_width, num_filters, layer1_width, width, theta + 1, theta, params_eps(eps),
                         train_ar, dz_buf, t1_buf, packed, packed + 2, static_cast<hipStream_t>(stream), NO_APPLY);
}

int bear_net_cnn_train_step_wide_f64(bear_ws *ws, const uint32_t *counts, const int8_t *codes, uint64_t n_rows, int lag, int filter_width,
                                     int num_filters, int layer1_width, int width, double *theta, double *adam_m, double *adam_v,
                                     double *adam_t, double *dz_buf, double *t1_buf, double eps, int train_ar, double learning_rate,
                                     double scale, double *packed, double *loss_buf, uint64_t loss_cap, void *stream) {
  if (!theta || !packed || !adam_m || !adam_v || !adam_t) return BEAR_ERR_INVALID_ARG;
  if (misaligned8(theta) || misaligned8(adam_m) || misaligned8(adam_v) || misaligned8(adam_t) || misaligned8(loss_buf))
    return BEAR_ERR_INVALID_ARG;
  if (!cnn_wide_shape_ok(lag, filter_width, num_filters, layer1_width, width)) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n_theta = 1 + cnw_make_dims(lag, filter_width).total;
  if (two_launch_step()) {
    int st = cnn_wide_reduce(ws, counts, codes, n_rows, lag, filter_width, num_filters, layer1_width, width, theta + 1, theta,
                             params_eps(eps), train_ar, dz_buf, t1_buf, packed, packed + 2, s, NO_APPLY);
    if (st != BEAR_OK) return st;
    return launch_train_apply(theta, n_theta, packed, adam_m, adam_v, adam_t, learning_rate, scale, train_ar, loss_buf, loss_cap, s);
  }
  // the backward block that sums the gradient's partials runs the update behind them (bear_apply_in_block)
  return cnn_wide_reduce(ws, counts, codes, n_rows, lag, filter_width, num_filters, layer1_width, width, theta + 1, theta, params_eps(eps),
                         train_ar, dz_buf, t1_buf, packed, packed + 2, s,
                         make_apply(theta, n_theta, adam_m, adam_v, adam_t, learning_rate, scale, train_ar, loss_buf, loss_cap));
}
