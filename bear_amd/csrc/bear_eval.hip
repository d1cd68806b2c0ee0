// bear_eval.hip -- held-out evaluation and the BMM marginal (kernels_eval.h), their 21-wide forms and the wide DM step
// (kernels_wide.h), bear_ref's wide steps (kernels_refmix_wide.h), evaluation on a sorted plan of the test column
// (kernels_evalplan.h), the two-sample Bayes factors of two count columns (kernels_twosample.h)
// and those among up to sixteen (kernels_ksample.h).  The other units: bear_host.h.
#include "bear_host.h"
#include "kernels_eval.h"
#include "kernels_wide.h"
#include "kernels_refmix_wide.h"
#include "kernels_evalplan.h"
#include "kernels_twosample.h"
#include "kernels_ksample.h"

#ifdef EVP_STAMPS
#define EVP_DBG_ARG , ws->dbg
#else
#define EVP_DBG_ARG
#endif

int eval_ws_setup(bear_ws *ws) {
  const int st = allow_dynamic_lds({BEAR_KFN(eval_plan_kernel<0, 4>), BEAR_KFN(eval_plan_kernel<1, 0>), BEAR_KFN(eval_plan_kernel<1, 4>),
                                    BEAR_KFN(eval_plan_kernel<4, 0>)},
                                   sizeof(evp_lds));
  if (st != BEAR_OK) return st;
  HIP_TRY(hipMalloc(&ws->eval_partials, sizeof(double) * EVL_MAX_OUT * (size_t)ws->eval_blocks));
  HIP_TRY(hipMalloc(&ws->eval_out, sizeof(double) * EVL_MAX_OUT));
  return BEAR_OK;
}

// Where the compact sums of one launch -- the DM models [m0, m0 + m_cnt), m_cnt <= EVS_CHUNK, and with the first chunk the AR model
// and the total length -- go in the result vector: ll_ear[n_h], ll_arm, ll_van[n_van], cor_ear[n_h], cor_arm, cor_van[n_van], total
static evs_slots eval_chunk_slots(const evl_args &A, int m0, int m_cnt) {
  const int n_models = A.n_h + A.n_van;
  evs_slots S;
  for (int k = 0; k < EVS_NOUT; ++k) S.slot[k] = -1;
  for (int k = 0; k < m_cnt; ++k) {
    const int m = m0 + k;
    const int ll_slot = m < A.n_h ? m : m + 1;                 // ll_arm sits between the BEAR and vanilla blocks
    S.slot[k] = ll_slot;
    S.slot[EVS_CHUNK + k] = n_models + 1 + ll_slot;
  }
  if (m0 == 0) {
    S.slot[2 * EVS_CHUNK] = A.n_h;
    S.slot[2 * EVS_CHUNK + 1] = n_models + 1 + A.n_h;
    S.slot[2 * EVS_CHUNK + 2] = 2 * n_models + 2;
  }
  return S;
}

static int launch_eval(bear_ws *ws, const uint32_t *test, const uint32_t *train, const double *prior, uint64_t n_rows,
                       const evl_args &A, double *out, hipStream_t s) {
  // sorted formulation (kernels_eval.h): at most EVS_CHUNK DM models per launch; the first launch also carries the AR
  // model and the total length (eval_chunk_slots)
  const int n_models = A.n_h + A.n_van;
  const int grid = grid_capped((n_rows + EVS_THREADS - 1) / EVS_THREADS, (uint64_t)ws->eval_blocks);
  static_assert(EVS_NOUT <= EVL_MAX_OUT, "compact partials fit the evaluation partial buffer");
  for (int m0 = 0; m0 == 0 || m0 < n_models; m0 += EVS_CHUNK) {
    const int m_cnt = n_models - m0 < EVS_CHUNK ? n_models - m0 : EVS_CHUNK;
    const int common = m0 == 0;
    const evs_slots S = eval_chunk_slots(A, m0, m_cnt);
    hipLaunchKernelGGL(eval_sorted_kernel, dim3(grid), dim3(EVS_THREADS), 0, s, test, train, prior, n_rows, A, m0, m_cnt, common,
                       reinterpret_cast<const double2 *>(ws->logtab), ws->eval_partials);
    hipLaunchKernelGGL(eval_sorted_finalize_kernel, dim3((EVS_NOUT + 3) / 4), dim3(256), 0, s, ws->eval_partials, grid, S, out);
  }
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}
static int eval_make_args(const uint32_t *test, const uint32_t *train, const double *prior, uint64_t n_rows, const double *h, int n_h,
                          int with_ar, const double *van_reg, int n_van, double eps, uint64_t noise_seed, uint64_t row_base,
                          const double *out, evl_args *Aout) {
  if (!out || n_h < 0 || n_van < 0 || n_h + n_van > EVL_MAX_MODELS || (n_h && !h) || (n_van && !van_reg))
    return BEAR_ERR_INVALID_ARG;
  if ((n_h || with_ar) && !prior && n_rows) return BEAR_ERR_INVALID_ARG;
  if (n_rows && !test) return BEAR_ERR_INVALID_ARG;
  if (misaligned(test) || misaligned(train) || misaligned(prior)) return BEAR_ERR_INVALID_ARG;
  if (!(eps >= 0.0)) return BEAR_ERR_INVALID_ARG;
  evl_args &A = *Aout;
  memset(&A, 0, sizeof(A));
  A.n_h = n_h;
  A.n_van = n_van;
  A.arm = with_ar ? 1 : 0;
  A.has_train = train ? 1 : 0;
  A.has_prior = prior ? 1 : 0;
  A.eps = eps;
  A.seed = noise_seed;
  A.row_base = row_base;
  for (int j = 0; j < n_h; ++j) {
    if (!(h[j] > 0.0)) return BEAR_ERR_INVALID_ARG;
    A.inv_h[j] = 1.0 / h[j];
  }
  for (int k = 0; k < n_van; ++k) A.inv_h[n_h + k] = van_reg[k];
  return BEAR_OK;
}

int bear_eval_f64(bear_ws *ws, const uint32_t *test, const uint32_t *train, const double *prior, uint64_t n_rows,
                  const double *h, int n_h, int with_ar, const double *van_reg, int n_van, double eps,
                  uint64_t noise_seed, uint64_t row_base, double *out, void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  evl_args A;
  st = eval_make_args(test, train, prior, n_rows, h, n_h, with_ar, van_reg, n_van, eps, noise_seed, row_base, out, &A);
  if (st != BEAR_OK) return st;
  return launch_eval(ws, test, train, prior, n_rows, A, out, static_cast<hipStream_t>(stream));
}


int bear_dm_prior_wide_f64(bear_ws *ws, const uint32_t *counts, const double *prior, uint64_t n_rows, int width,
                           const double *h_signed_dev, double eps, int train_ar, double *out, double *grad_prior, void *stream) {
  if (!wide_width_ok(width)) return BEAR_ERR_INVALID_ARG;
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!out || (n_rows && (!counts || !prior)) || (!h_signed_dev && !train_ar)) return BEAR_ERR_INVALID_ARG;
  if (misaligned(counts) || misaligned(prior) || misaligned(grad_prior) || misaligned8(out) || misaligned8(h_signed_dev))
    return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  bear_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.inv_h = 1.0;           // (AR mode without h_signed_dev: never read)
  prm.eps = eps;
  const int grid = wide_grid(ws, n_rows, WIDE_TILE(width), WIDE_BLOCKS_PER_CU);
  const bear_step_io io = ws_io(ws, h_signed_dev, BEAR_THETA_NET, out);
  const double2 *lt = reinterpret_cast<const double2 *>(ws->logtab);
#define WIDE_LAUNCH(AR, GRAD) \
  hipLaunchKernelGGL((dm_wide_kernel<W, AR, GRAD>), dim3(grid), dim3(WIDE_THREADS), 0, s, counts, prior, n_rows, prm, grad_prior, lt, ws->partials, io)
  BEAR_DISPATCH_W(width, BEAR_DISPATCH_2(train_ar, grad_prior, WIDE_LAUNCH));
#undef WIDE_LAUNCH
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_eval_wide_f64(bear_ws *ws, const uint32_t *test, const uint32_t *train, const double *prior, uint64_t n_rows, int width,
                       const double *h, int n_h, int with_ar, const double *van_reg, int n_van, double eps,
                       uint64_t noise_seed, uint64_t row_base, double *out, void *stream) {
  if (!wide_width_ok(width)) return BEAR_ERR_INVALID_ARG;
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  evl_args A;
  st = eval_make_args(test, train, prior, n_rows, h, n_h, with_ar, van_reg, n_van, eps, noise_seed, row_base, out, &A);
  if (st != BEAR_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // launch_eval's chunks of models and slot layout
  const int n_models = A.n_h + A.n_van;
  const int grid = grid_capped((n_rows + EVW_THREADS - 1) / EVW_THREADS, (uint64_t)ws->eval_blocks);
  const double2 *lt = reinterpret_cast<const double2 *>(ws->logtab);
  for (int m0 = 0; m0 == 0 || m0 < n_models; m0 += EVS_CHUNK) {
    const int m_cnt = n_models - m0 < EVS_CHUNK ? n_models - m0 : EVS_CHUNK;
    const int common = m0 == 0;
    const evs_slots S = eval_chunk_slots(A, m0, m_cnt);
    BEAR_DISPATCH_W(width, hipLaunchKernelGGL(eval_wide_kernel<W>, dim3(grid), dim3(EVW_THREADS), 0, s, test, train, prior, n_rows, A, m0,
                                              m_cnt, common, lt, ws->eval_partials));
    hipLaunchKernelGGL(eval_sorted_finalize_kernel, dim3((EVS_NOUT + 3) / 4), dim3(256), 0, s, ws->eval_partials, grid, S, out);
  }
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

// ---- two-sample and goodness-of-fit Bayes factors (kernels_twosample.h) ----------------------------------------------------
// What bear_two_sample_f64 and bear_k_sample_f64 refuse alike about their models, and the models' weights w: [0, n_h) 1 / h,
// [n_h, n_h + n_van) van, every h and van > 0 and finite -> the number of models, or BEAR_ERR_INVALID_ARG.  No device call.
static int bayes_models(const double *h, int n_h, const double *van, int n_van, const double *prior, uint64_t n_rows, bool want_ar,
                        double w[BEAR_TWO_SAMPLE_MAX_MODELS]) {
  if (n_h < 0 || n_van < 0 || n_h + n_van < 1 || n_h + n_van > BEAR_TWO_SAMPLE_MAX_MODELS) return BEAR_ERR_INVALID_ARG;
  if ((n_h && !h) || (n_van && !van) || (n_rows && (n_h || want_ar) && !prior)) return BEAR_ERR_INVALID_ARG;
  for (int m = 0; m < n_h + n_van; ++m) {
    const double v = m < n_h ? h[m] : van[m - n_h];
    if (!(v > 0.0 && v < INFINITY)) return BEAR_ERR_INVALID_ARG;
    w[m] = m < n_h ? 1.0 / v : v;
  }
  return n_h + n_van;
}

// Every refusal comes before the first device call; h and van are read here, before the entry returns (they travel by value).
int bear_two_sample_f64(bear_ws *ws, const uint32_t *a, const uint32_t *b, const double *prior, uint64_t n_rows, int width,
                        const double *h, int n_h, const double *van, int n_van, void *stream, double *out, double *out_ar,
                        double *row_terms) {
  if (!wide_width_ok(width)) return BEAR_ERR_INVALID_ARG;
  if (!ws || !out || (n_rows && (!a || !b))) return BEAR_ERR_INVALID_ARG;
  if (misaligned(a) || misaligned(b) || misaligned(prior) || misaligned8(out) || misaligned8(out_ar) || misaligned8(row_terms))
    return BEAR_ERR_INVALID_ARG;
  ts_args A;
  memset(&A, 0, sizeof(A));
  A.n_h = n_h;
  A.n_models = bayes_models(h, n_h, van, n_van, prior, n_rows, out_ar != nullptr, A.w);
  if (A.n_models < 0) return A.n_models;
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  static_assert(TS_NOUT <= EVL_MAX_OUT, "compact partials fit the evaluation partial buffer");
  uint64_t cap = ws_blocks(ws, TS_BLOCKS_PER_CU);
  if (cap > (uint64_t)ws->eval_blocks) cap = (uint64_t)ws->eval_blocks;
  const int grid = grid_capped((n_rows + TS_TILE(width) - 1) / TS_TILE(width), cap);
  const double2 *lt = reinterpret_cast<const double2 *>(ws->logtab);
  for (int m0 = 0; m0 < A.n_models; m0 += TS_CHUNK) {
    const int m_cnt = A.n_models - m0 < TS_CHUNK ? A.n_models - m0 : TS_CHUNK;
    const int do_ar = m0 == 0 && out_ar;
    const int use_prior = do_ar || m0 < n_h;
    BEAR_DISPATCH_W(width, hipLaunchKernelGGL(two_sample_kernel<W>, dim3(grid), dim3(TS_THREADS), 0, s, a, b, prior, n_rows, A, m0, m_cnt,
                                              use_prior, do_ar, lt, ws->eval_partials, row_terms));
    hipLaunchKernelGGL(two_sample_finalize_kernel, dim3((TS_NOUT + 3) / 4), dim3(256), 0, s, ws->eval_partials, grid, m0, m_cnt, out,
                       do_ar ? out_ar : nullptr);
  }
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

// ---- Bayes factors among G columns (kernels_ksample.h) ----------------------------------------------------------------------
static inline int ks_padded_groups(int g) { return g <= 2 ? 2 : g <= 4 ? 4 : g <= 8 ? 8 : 16; }
static inline uint64_t ks_npart(int gp) { return gp == 2 ? KS_NPART(2) : gp == 4 ? KS_NPART(4) : gp == 8 ? KS_NPART(8) : KS_NPART(16); }
// the blocks any device takes for a table: the tiles, at most KS_MAX_BLOCKS (a launch: and at most KS_BLOCKS_PER_CU a CU)
static inline uint64_t ks_blocks(uint64_t n_rows, int width, int gp) {
  const uint64_t tile = (uint64_t)(KS_TILE(width, gp)), tiles = n_rows / tile + (n_rows % tile ? 1 : 0);
  return tiles < 1 ? 1 : (tiles < KS_MAX_BLOCKS ? tiles : KS_MAX_BLOCKS);
}

uint64_t bear_k_sample_scratch(bear_ws *ws, uint64_t n_rows, int width, int n_groups) {
  (void)ws;
  if (!wide_width_ok(width) || n_groups < 2 || n_groups > BEAR_K_SAMPLE_MAX_GROUPS) return 0;
  const int gp = ks_padded_groups(n_groups);
  return ks_blocks(n_rows, width, gp) * ks_npart(gp);
}

// Every refusal comes before the first device call; col_rows, h and van are read here (they travel by value).
int bear_k_sample_f64(bear_ws *ws, const uint32_t *counts, const uint64_t *col_rows, int n_groups, const double *prior,
                      uint64_t n_rows, int width, const double *h, int n_h, const double *van, int n_van, void *stream,
                      double *scratch, uint64_t n_scratch, double *out_group, double *out_pair, double *out_all,
                      double *out_ar, double *row_terms) {
  if (!wide_width_ok(width)) return BEAR_ERR_INVALID_ARG;
  if (n_groups < 2 || n_groups > BEAR_K_SAMPLE_MAX_GROUPS || !col_rows) return BEAR_ERR_INVALID_ARG;
  if (!ws || !scratch || !out_group || !out_pair || !out_all || (n_rows && !counts)) return BEAR_ERR_INVALID_ARG;
  if (n_scratch < bear_k_sample_scratch(ws, n_rows, width, n_groups)) return BEAR_ERR_INVALID_ARG;
  if (misaligned(prior) || misaligned8(scratch) || misaligned8(out_group) || misaligned8(out_pair) || misaligned8(out_all) ||
      misaligned8(out_ar) || misaligned8(row_terms))
    return BEAR_ERR_INVALID_ARG;
  ks_args A;
  memset(&A, 0, sizeof(A));
  A.n_h = n_h;
  A.n_groups = n_groups;
  for (int g = 0; g < n_groups; ++g) {
    if (counts && misaligned(counts + col_rows[g] * (uint64_t)width)) return BEAR_ERR_INVALID_ARG;
    A.col[g] = col_rows[g];
  }
  A.n_models = bayes_models(h, n_h, van, n_van, prior, n_rows, out_ar != nullptr, A.w);
  if (A.n_models < 0) return A.n_models;
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int gp = ks_padded_groups(n_groups), n_part = (int)ks_npart(gp);
  const int sl = gp == 2 ? KS_SLOTS(2) : gp == 4 ? KS_SLOTS(4) : gp == 8 ? KS_SLOTS(8) : KS_SLOTS(16);
  const int grid = grid_capped(ks_blocks(n_rows, width, gp), ws_blocks(ws, KS_BLOCKS_PER_CU));
  const double2 *lt = reinterpret_cast<const double2 *>(ws->logtab);
  for (int m0 = 0; m0 < A.n_models; m0 += KS_CHUNK) {
    const int m_cnt = A.n_models - m0 < KS_CHUNK ? A.n_models - m0 : KS_CHUNK;
    const int do_ar = m0 == 0 && out_ar;
    const int use_prior = do_ar || m0 < n_h;
#define KS_LAUNCH(GP_)                                                                                                              \
  hipLaunchKernelGGL((k_sample_kernel<W, GP_>), dim3(grid), dim3(KS_THREADS), 0, s, counts, prior, n_rows, A, m0, m_cnt, use_prior, \
                     do_ar, lt, scratch, row_terms)
    BEAR_DISPATCH_W(width, do {
      if (gp == 2) KS_LAUNCH(2);
      else if (gp == 4) KS_LAUNCH(4);
      else if (gp == 8) KS_LAUNCH(8);
      else KS_LAUNCH(16);
    } while (0));
#undef KS_LAUNCH
    hipLaunchKernelGGL(k_sample_finalize_kernel, dim3((n_part + 3) / 4), dim3(256), 0, s, scratch, grid, gp, sl, n_groups, m0, m_cnt,
                       out_group, out_pair, out_all, do_ar ? out_ar : nullptr);
  }
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

// ---- bear_ref's step at width W (kernels_refmix_wide.h) ------------------------------------------------------------------
// the stop net function: the checks and the launch of bear_dm_ref_wide_f64 and of bear_ref_train_{reduce,step}_wide_f64 (theta != NULL:
// the constants from the device-resident parameters; `apply`: the last block runs the update behind its sums)
static int launch_ref_wide(bear_ws *ws, const uint32_t *train, const uint32_t *ref, uint64_t n_rows, int width, const bear_params &prm,
                           const double *theta, int train_ar, double *out, hipStream_t s, const bear_apply_io &apply) {
  if (!wide_width_ok(width)) return BEAR_ERR_INVALID_ARG;
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!out || (n_rows && (!train || !ref))) return BEAR_ERR_INVALID_ARG;
  if (misaligned(train) || misaligned(ref) || misaligned8(out) || misaligned8(theta) || !(prm.eps >= 0.0)) return BEAR_ERR_INVALID_ARG;
  const int grid = wide_grid(ws, n_rows, RFW_TILE(width), RFW_BLOCKS_PER_CU);
  const bear_step_io io = ws_io(ws, theta, BEAR_THETA_REF, out);
  const double2 *lt = reinterpret_cast<const double2 *>(ws->logtab);
#define REF_WIDE(AR) \
  hipLaunchKernelGGL((dm_ref_wide_kernel<W, AR>), dim3(grid), dim3(RFW_THREADS), 0, s, train, ref, n_rows, prm, lt, ws->partials, io, apply)
  BEAR_DISPATCH_W(width, BEAR_DISPATCH_1(train_ar, REF_WIDE));
#undef REF_WIDE
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_dm_ref_wide_f64(bear_ws *ws, const uint32_t *train, const uint32_t *ref, uint64_t n_rows, int width, double h_signed,
                         double tau_signed, double nu_signed, double eps, int train_ar, double *out, void *stream) {
  return launch_ref_wide(ws, train, ref, n_rows, width, params_ref(h_signed, tau_signed, nu_signed, eps), nullptr, train_ar, out,
                         static_cast<hipStream_t>(stream), NO_APPLY);
}

int bear_ref_train_reduce_wide_f64(bear_ws *ws, const uint32_t *train, const uint32_t *ref, uint64_t n_rows, int width,
                                   const double *theta, double eps, int train_ar, double *packed, void *stream) {
  if (!theta) return BEAR_ERR_INVALID_ARG;
  return launch_ref_wide(ws, train, ref, n_rows, width, params_eps(eps), theta, train_ar, packed, static_cast<hipStream_t>(stream), NO_APPLY);
}

int bear_ref_train_step_wide_f64(bear_ws *ws, const uint32_t *train, const uint32_t *ref, uint64_t n_rows, int width, double *theta,
                                 double *adam_m, double *adam_v, double *adam_t, double eps, int train_ar, double learning_rate,
                                 double scale, double *out, double *loss_buf, uint64_t loss_cap, void *stream) {
  if (!theta || !adam_m || !adam_v || !adam_t) return BEAR_ERR_INVALID_ARG;
  if (misaligned8(adam_m) || misaligned8(adam_v) || misaligned8(adam_t) || misaligned8(loss_buf)) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (two_launch_step()) {
    int st = launch_ref_wide(ws, train, ref, n_rows, width, params_eps(eps), theta, train_ar, out, s, NO_APPLY);
    if (st != BEAR_OK) return st;
    return launch_train_apply(theta, 3, out, adam_m, adam_v, adam_t, learning_rate, scale, train_ar, loss_buf, loss_cap, s);
  }
  // ONE launch: the last block of the reduce kernel runs the update behind its sums (bear_apply_in_block)
  return launch_ref_wide(ws, train, ref, n_rows, width, params_eps(eps), theta, train_ar, out, s,
                         make_apply(theta, 3, adam_m, adam_v, adam_t, learning_rate, scale, train_ar, loss_buf, loss_cap));
}

// a net function with parameters: the mixing inside the DM step, gradient rows over the net rows
int bear_dm_refmix_wide_grad_f64(bear_ws *ws, const uint32_t *counts, const double *net_rows, const uint32_t *ref, uint64_t n_rows,
                                 int width, const double *h_signed_dev, const double *tau_signed_dev, const double *net_weight_signed_dev,
                                 double eps, int train_ar, double *out, double *grad_net_rows, void *stream) {
  if (!wide_width_ok(width)) return BEAR_ERR_INVALID_ARG;
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!out || !h_signed_dev || !tau_signed_dev || !net_weight_signed_dev) return BEAR_ERR_INVALID_ARG;
  if (n_rows && (!counts || !net_rows || !ref || !grad_net_rows)) return BEAR_ERR_INVALID_ARG;
  if (misaligned(counts) || misaligned(net_rows) || misaligned(ref) || misaligned(grad_net_rows) || misaligned8(out) ||
      misaligned8(h_signed_dev) || misaligned8(tau_signed_dev) || misaligned8(net_weight_signed_dev) || !(eps >= 0.0))
    return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int grid = wide_grid(ws, n_rows, RMW_TILE(width), RMW_BLOCKS_PER_CU);
  const bear_step_io io = ws_io(ws, nullptr, BEAR_THETA_REF, out);
  const double2 *lt = reinterpret_cast<const double2 *>(ws->logtab);
#define MIX_WIDE(AR)                                                                                                                \
  hipLaunchKernelGGL((dm_refmix_wide_kernel<W, AR>), dim3(grid), dim3(RFW_THREADS), 0, s, counts, net_rows, ref, n_rows, h_signed_dev, \
                     tau_signed_dev, net_weight_signed_dev, eps, lt, grad_net_rows, ws->partials, io)
  BEAR_DISPATCH_W(width, BEAR_DISPATCH_1(train_ar, MIX_WIDE));
#undef MIX_WIDE
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

// ---- evaluation on a sorted plan of the test column (kernels_evalplan.h) ------------------------------------------------
struct bear_eval_plan {
  int device;
  uint64_t n_rows, n_tiles;
  const uint32_t *test, *train;  // the buffers the plan was built from (identity check only; train may be NULL)
  uint16_t *items;       // [n_tiles][EVP_ITEMS_CAP]
  uint2 *tile_info;      // [n_tiles]
  unsigned long long *consts;   // [EVP_NCONST]: what the vanilla models, the total length need of the table as a whole (kernels_evalplan.h, EVP_C_*)
  uint64_t bytes;
};

int bear_eval_plan_create(bear_ws *ws, const uint32_t *test, const uint32_t *train, uint64_t n_rows, bear_eval_plan **out, void *stream) {
  if (!out) return BEAR_ERR_INVALID_ARG;
  *out = nullptr;
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if ((n_rows && !test) || misaligned(test) || misaligned(train)) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint64_t n_tiles = (n_rows + EVP_ROWS - 1) / EVP_ROWS;
  // + 1 KiB: the last DMA piece of a tile's lists may be issued for a partial KiB
  const size_t n_items = EVP_ITEMS_CAP * (size_t)n_tiles + 1024 / sizeof(uint16_t), n_info = (size_t)n_tiles + 2;
  dev_buf<uint16_t> items;
  dev_buf<uint2> tile_info;
  dev_buf<unsigned long long> consts;
  if (n_tiles) {
    HIP_TRY(items.alloc(n_items));
    HIP_TRY(tile_info.alloc(n_info));
    HIP_TRY(consts.alloc(EVP_NCONST));
    HIP_TRY(hipMemsetAsync(tile_info.get(), 0, sizeof(uint2) * n_info, s));
    HIP_TRY(hipMemsetAsync(consts.get(), 0, sizeof(unsigned long long) * EVP_NCONST, s));
    const int grid = grid_capped(n_tiles, (uint64_t)ws->num_cu * 16);
    hipLaunchKernelGGL(evp_build_kernel, dim3(grid), dim3(256), 0, s, test, train, n_rows, n_tiles, items.get(),
                       tile_info.get(), consts.get());
    HIP_TRY(hipGetLastError());
  }
  const uint64_t bytes = n_tiles ? sizeof(uint16_t) * n_items + sizeof(uint2) * n_info + sizeof(unsigned long long) * EVP_NCONST : 0;
  *out = new (std::nothrow) bear_eval_plan{ws->device, n_rows, n_tiles, test, train, items.release(), tile_info.release(), consts.release(), bytes};
  return *out ? BEAR_OK : BEAR_ERR_NOMEM;
}

int bear_eval_plan_destroy(bear_eval_plan *plan) {
  if (!plan) return BEAR_OK;
  int prev = 0;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(plan->device);
  (void)hipFree(plan->items);
  (void)hipFree(plan->tile_info);
  (void)hipFree(plan->consts);
  (void)hipSetDevice(prev);
  delete plan;
  return BEAR_OK;
}

uint64_t bear_eval_plan_bytes(const bear_eval_plan *plan) { return plan ? plan->bytes : 0; }

int bear_eval_plan_f64(bear_ws *ws, const bear_eval_plan *plan, const uint32_t *test, const uint32_t *train, const double *prior,
                       uint64_t n_rows, const double *h, int n_h, int with_ar, const double *van_reg, int n_van, double eps,
                       uint64_t noise_seed, uint64_t row_base, const uint32_t *row_ids, double *out, void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!plan || plan->test != test || plan->train != train || plan->n_rows != n_rows || plan->device != ws->device)
    return BEAR_ERR_INVALID_ARG;
  if (misaligned(row_ids)) return BEAR_ERR_INVALID_ARG;
  evl_args A;
  st = eval_make_args(test, train, prior, n_rows, h, n_h, with_ar, van_reg, n_van, eps, noise_seed, row_base, out, &A);
  if (st != BEAR_OK) return st;
  A.has_rid = row_ids ? 1 : 0;
  // The plan decides the vanilla models' arg-max on the INTEGER training counts (a letter a whole count below the top cannot win):
  // that is the arg-max of count + van_reg + eps + noise only while 17.5 sigma = 1750 eps stays below a count and the sum keeps
  // the counts apart (bear_eval_f64 takes any values).
  if (A.n_van && !(1750.0 * eps < 0.5)) return BEAR_ERR_INVALID_ARG;
  for (int k = 0; k < A.n_van; ++k)
    if (!(van_reg[k] >= 0.0 && van_reg[k] <= 0x1p30)) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n_models = A.n_h + A.n_van;
  const uint64_t nt = plan->n_tiles;
  const int grid = grid_capped(nt, (uint64_t)ws->num_cu);   // one resident 768-thread block per CU
  const double2 *lt = reinterpret_cast<const double2 *>(ws->logtab);
  // launches: BEAR models (product path) four at a time, vanilla models (lgamma tables) four at a time -- a BEAR group and a
  // vanilla group share a launch; the first launch also carries the AR model and the total length.
  int h0 = 0, v0 = 0;
  bool first = true;
  while (first || h0 < A.n_h || v0 < A.n_van) {
    const int nh = A.n_h - h0 < EVP_MAXH ? A.n_h - h0 : EVP_MAXH;
    int nv = A.n_van - v0 < EVP_MAXV ? A.n_van - v0 : EVP_MAXV;
    if (nh > 1) nv = 0;   // four BEAR models fill the register file (168 per lane at three waves per SIMD): the vanilla group follows
    int common = first ? 1 : 0;
    evs_slots S;
    for (int k = 0; k < EVS_NOUT; ++k) S.slot[k] = -1;
    for (int k = 0; k < nh; ++k) {            // output: ll_ear[n_h], ll_arm, ll_van[n_van], cor_ear[n_h], cor_arm, cor_van[n_van], total
      S.slot[k] = h0 + k;
      S.slot[EVS_CHUNK + k] = n_models + 1 + h0 + k;
    }
    for (int k = 0; k < nv; ++k) {
      S.slot[EVP_SLOT_VAN + k] = A.n_h + 1 + v0 + k;
      S.slot[EVS_CHUNK + EVP_SLOT_VAN + k] = n_models + 1 + A.n_h + 1 + v0 + k;
    }
    if (common) {
      S.slot[2 * EVS_CHUNK] = A.n_h;
      S.slot[2 * EVS_CHUNK + 1] = n_models + 1 + A.n_h;
      S.slot[2 * EVS_CHUNK + 2] = 2 * n_models + 2;
    }
#define EVP_LAUNCH(NH_, NV_)                                                                                                        \
  hipLaunchKernelGGL((eval_plan_kernel<NH_, NV_>), dim3(grid), dim3(EVP_THREADS), sizeof(evp_lds), s, test, train, prior, row_ids, n_rows, A, \
                     h0, nh, v0, nv, common, plan->items, plan->tile_info, plan->consts, nt, lt, ws->eval_partials EVP_DBG_ARG)
    if (nh == 0) EVP_LAUNCH(0, 4);
    else if (nh == 1 && nv == 0) EVP_LAUNCH(1, 0);
    else if (nh == 1) EVP_LAUNCH(1, 4);
    else EVP_LAUNCH(4, 0);
#undef EVP_LAUNCH
    hipLaunchKernelGGL(eval_sorted_finalize_kernel, dim3((EVS_NOUT + 3) / 4), dim3(256), 0, s, ws->eval_partials, grid, S, out);
    h0 += nh;
    v0 += nv;
    first = false;
  }
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_bmm_f64(bear_ws *ws, const uint32_t *counts, uint64_t n_rows, const double *alpha, int n_alpha, double *out,
                 void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!out || !alpha || n_alpha <= 0 || n_alpha > EVL_MAX_MODELS || (n_rows && !counts) || misaligned(counts))
    return BEAR_ERR_INVALID_ARG;
  evl_args A;
  memset(&A, 0, sizeof(A));
  A.n_van = n_alpha;
  for (int k = 0; k < n_alpha; ++k) {
    if (!(alpha[k] > 0.0)) return BEAR_ERR_INVALID_ARG;
    A.inv_h[k] = alpha[k];
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  st = launch_eval(ws, counts, nullptr, nullptr, n_rows, A, ws->eval_out, s);
  if (st != BEAR_OK) return st;
  // result vector layout: [ll_arm (unused), ll_van[n_alpha], ...]
  HIP_TRY(hipMemcpyAsync(out, ws->eval_out + 1, sizeof(double) * (size_t)n_alpha, hipMemcpyDeviceToDevice, s));
  return BEAR_OK;
}
