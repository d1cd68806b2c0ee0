// bear_linear.hip -- the linear AR head: k-mer packing and index words, the paired context lists of a plan, the fused DM step
// (kernels_linear.h; kernels_linear_wide.h at the protein alphabet's width), the head as rows (kernels_linrows.h;
// kernels_linrows_wide.h at that width), and the optimizer update as a launch of its own (adam_vec_kernel).
// The other units: bear_host.h.
#include "bear_host.h"
#include "kernels_linear.h"
#include "kernels_linrows.h"
#include "kernels_linrows_wide.h"
#include "kernels_linear_wide.h"

// ---- the fused step's kernel (kernels_linear.h), every instantiation: [AR][PAIRED][DET][slot].  A slot is a number of letter groups
// as a compile-time constant: the lags 4 / 5 (2 groups: the bundled table), 12 / 13 (6: BASELINE's k = 13) and 14 / 15 (7); slot 0
// takes the kernel that finds the number at run time (distinct13: 0.847 -> 0.833 ms, 128 -> 97 registers).  A count added to
// LIN_NGK gets its kernels, their LDS attribute (linear_ws_setup) and its launches (launch_linear) from this one list.
static constexpr int LIN_NGK[] = {0, 2, 6, 7};
constexpr int LIN_SLOTS = (int)(sizeof(LIN_NGK) / sizeof(LIN_NGK[0]));
using lin_kernel_fn = decltype(&dm_linear_plan_kernel<false, false, false, 0>);
#define LIN_FORMS(AR, PAIRED, DET)                                                                                     \
  {dm_linear_plan_kernel<AR, PAIRED, DET, LIN_NGK[0]>, dm_linear_plan_kernel<AR, PAIRED, DET, LIN_NGK[1]>, \
   dm_linear_plan_kernel<AR, PAIRED, DET, LIN_NGK[2]>, dm_linear_plan_kernel<AR, PAIRED, DET, LIN_NGK[3]>}
static_assert(LIN_SLOTS == 4, "LIN_FORMS names the slots");
static const lin_kernel_fn LIN_KERNELS[2][2][2][LIN_SLOTS] = {
    {{LIN_FORMS(false, false, false), LIN_FORMS(false, false, true)}, {LIN_FORMS(false, true, false), LIN_FORMS(false, true, true)}},
    {{LIN_FORMS(true, false, false), LIN_FORMS(true, false, true)}, {LIN_FORMS(true, true, false), LIN_FORMS(true, true, true)}}};
#undef LIN_FORMS
// the slot of a number of groups (0: none of the specialised ones)
static int lin_slot(int n_groups) {
  for (int k = 1; k < LIN_SLOTS; ++k)
    if (LIN_NGK[k] == n_groups) return k;
  return 0;
}

int linear_ws_setup(bear_ws *ws) {
  int st = BEAR_OK;
  const lin_kernel_fn *all = &LIN_KERNELS[0][0][0][0];
  for (size_t k = 0; st == BEAR_OK && k < sizeof(LIN_KERNELS) / sizeof(lin_kernel_fn); ++k)
    st = allow_dynamic_lds({BEAR_KFN(all[k])}, sizeof(pln_lds_lin));
  if (st != BEAR_OK) return st;
  st = allow_dynamic_lds({BEAR_KFN(linear_wide_forward_kernel)}, LNW_FWD_LDS(LINEAR_WIDE_MAX_LAG));
  if (st != BEAR_OK) return st;
  st = allow_dynamic_lds({BEAR_KFN(dm_linear_wide_kernel<false>), BEAR_KFN(dm_linear_wide_kernel<true>)}, LSW_LDS(LINEAR_WIDE_MAX_LAG));
  if (st != BEAR_OK) return st;
  // one buffer for the backward rows and the fused step: the same grid cap, the longer row
  HIP_TRY(hipMalloc(&ws->linw_partials, sizeof(double) * LSW_MAX_PACKED * WIDE_PARTIAL_ROWS(ws->num_cu, LNW_BWD_BLOCKS_PER_CU)));
  HIP_TRY(hipMalloc(&ws->linw_packed, sizeof(double) * LSW_MAX_PACKED));
  HIP_TRY(hipMalloc(&ws->lin_partials, sizeof(double) * LIN_MAX_GRAD * (size_t)ws->num_cu * PLN_BLOCKS_PER_CU));
  HIP_TRY(hipMalloc(&ws->lin_accum, sizeof(double) * LIN_MAX_GRAD));
  HIP_TRY(hipMemset(ws->lin_accum, 0, sizeof(double) * LIN_MAX_GRAD));
  return BEAR_OK;
}

#ifdef LIN_STAMPS
extern "C" int bear_dbg_lin_stamps(unsigned long long *host_out, int reset) {   // developer build only
  if (host_out) HIP_TRY(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(lin_stamp_sums), sizeof(unsigned long long) * 8));
  if (reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(lin_stamp_sums), z, sizeof(z)));
  }
  return BEAR_OK;
}
extern "C" int bear_dbg_lin_pe_stamps(unsigned long long *host_out) {   // prologue / epilogue sections of the last launch (12 words)
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(lin_pe_stamps), sizeof(unsigned long long) * 12));
  return BEAR_OK;
}
#endif

// ---- fused linear AR head (kernels_linear.h) -----------------------------------------------------------
int bear_pack_kmers_u64(const int8_t *codes, uint64_t n_rows, int lag, uint64_t *packed, void *stream) {
  if (lag < 1 || lag > LIN_MAX_LAG) return BEAR_ERR_INVALID_ARG;
  if (n_rows == 0) return BEAR_OK;
  if (!codes || !packed) return BEAR_ERR_INVALID_ARG;
  const uint64_t blocks = (n_rows + 255) / 256;
  if (blocks > 0x7fffffffull) return BEAR_ERR_INVALID_ARG;
  hipLaunchKernelGGL(pack_kmers_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), codes, n_rows, lag,
                     reinterpret_cast<unsigned long long *>(packed));
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_linear_index_u64(const uint64_t *kmer_code, uint64_t n_rows, int lag, uint64_t *kmer_index, void *stream) {
  if (lag < 1 || lag > LIN_MAX_LAG) return BEAR_ERR_INVALID_ARG;
  if (n_rows == 0) return BEAR_OK;
  if (!kmer_code || !kmer_index) return BEAR_ERR_INVALID_ARG;
  uint64_t blocks = (n_rows + 255) / 256;
  if (blocks > 1u << 20) blocks = 1u << 20;
  hipLaunchKernelGGL(linear_index_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const unsigned long long *>(kmer_code), n_rows, lag, reinterpret_cast<unsigned long long *>(kmer_index));
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_encode_kmers_i8(const uint8_t *ascii, uint64_t n_rows, int lag, int rna, int8_t *codes, void *stream) {
  if (lag < 1) return BEAR_ERR_INVALID_ARG;
  if (n_rows == 0) return BEAR_OK;
  if (!ascii || !codes) return BEAR_ERR_INVALID_ARG;
  const uint64_t n_bytes = n_rows * (uint64_t)lag;
  uint64_t blocks = (n_bytes + 255) / 256;
  if (blocks > 1u << 20) blocks = 1u << 20;
  hipLaunchKernelGGL(encode_kmers_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), ascii, n_bytes, rna,
                     codes);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

// The fused step's launch.  A plan paired for exactly these index words (bear_plan_pair_contexts): the PAIRED form of the kernel
// over the paired tiles and, when some tiles kept their plain list, a second launch of the plain form over those, which adds
// its sums to the first one's (same stream: the workspace is free again when it starts).
static void launch_linear(bear_ws *ws, const bear_plan *plan, const uint64_t *kmer_code, const double *mat, int lag, const bear_params &prm,
                          int train_ar, const bear_step_io &io, double *grad_mat, hipStream_t s, const bear_apply_io &apply = NO_APPLY) {
  const double2 *lt = reinterpret_cast<const double2 *>(ws->logtab);
  const unsigned long long *kc = reinterpret_cast<const unsigned long long *>(kmer_code);
  const bool paired = plan->live2 && plan->pair_codes == kmer_code && plan->pair_lag == lag && !getenv("BEAR_AMD_LINEAR_UNPAIRED");
  // BEAR_AMD_DETERMINISTIC: fixed-point gradient tables (kernels_linear.h, lin_fx); the kernel derives their scale from these bounds
  const bool det = bear_deterministic() && plan->count_bound[0] >= 1.0 && plan->count_bound[0] < 0x1p50;
  const lin_fx_bound gt_bound = {plan->count_bound[0], plan->count_bound[1], log(plan->count_bound[2] > 1.0 ? plan->count_bound[2] : 1.0)};
  bear_step_io io2 = io;      // the second launch of a step: its own stamp on the arrival word
  io2.epoch = ws_arrival(ws).epoch;
  const pln_view pv = plan_view(plan);
  const bool two_launches = paired && plan->n_tiles_u != 0;
  // (BEAR_AMD_LINEAR_GENERIC=1: always the kernel that takes the group count at run time; tests compare the two)
  const int slot = getenv("BEAR_AMD_LINEAR_GENERIC") ? 0 : lin_slot(lin_make_geom(lag).ng);
  // one launch over `view`; acc 0: the step's only launch, 2: the first of two, 1: the second (its own stamp; it adds to the
  // first one's sums).  The update, if any, goes with the step's LAST launch: the one that completes the sums.
  auto launch = [&](bool paired_form, const pln_view &view, int acc) {
    hipLaunchKernelGGL(LIN_KERNELS[train_ar != 0][paired_form][det][slot], dim3(grid_plan(ws, view.n_tiles)), dim3(PLN_THREADS),
                       sizeof(pln_lds_lin), s, kc, mat, lag, prm, view, lt, ws->partials, ws->lin_accum, acc == 1 ? io2 : io, grad_mat, acc,
                       gt_bound, (acc == 1 || !two_launches) ? apply : NO_APPLY);
  };
  // a launch over some of the plan's tiles (their descriptors carry the tile's number in the plan: pln_view::subset)
  auto subset_view = [&](const pln_tile *tiles, uint64_t n_tiles) {
    pln_view v = pv;
    v.tiles = tiles;
    v.n_tiles = n_tiles;
    v.subset = 1;
    return v;
  };
  if (!paired) {
    launch(false, pv, 0);
    return;
  }
  // the paired tiles; the plan's global lists and histogram go with this launch
  launch(true, subset_view(plan->tiles_p, plan->n_tiles_p), two_launches ? 2 : 0);
  if (!two_launches) return;
  pln_view pu = subset_view(plan->tiles_u, plan->n_tiles_u);           // the rest: tiles only
  pu.n_heavy_col = pu.n_heavy_row = pu.n_heavy_stop = 0;
  pu.hist = nullptr;
  pu.hist_big = nullptr;
  launch(false, pu, 1);
}

void plan_unpair(bear_plan *plan) {
  if (!plan->live2) return;
  plan->bytes -= plan->n_tiles * LIN_LIVE2_STRIDE * sizeof(uint16_t) + (plan->n_tiles + 2 * PLN_DESC_PAD) * sizeof(pln_tile);
  (void)hipFree(plan->live2);
  (void)hipFree(plan->tiles_p);
  (void)hipFree(plan->tiles_u);
  plan->live2 = nullptr;
  plan->tiles_p = plan->tiles_u = nullptr;
  plan->n_tiles_p = plan->n_tiles_u = 0;
  plan->pair_codes = nullptr;
}

// Pairs the contexts of every tile's list for the fused linear step (kernels_linear.h, LIN_PAIR_CAP): kmer_index are the index
// words the step will be called with (bear_linear_index_u64 for `lag`), in the row order of the plan's count slab.
int bear_plan_pair_contexts(bear_plan *plan, const uint64_t *kmer_index, int lag, int *paired, void *stream) {
  if (paired) *paired = 0;
  if (!plan || plan->ncol != 5 || lag < 1 || lag > LIN_MAX_LAG) return BEAR_ERR_INVALID_ARG;
  if (plan->n_rows && (!kmer_index || misaligned(kmer_index))) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (plan->live2) {           // a plan holds one pairing: the new one replaces it
    HIP_TRY(hipStreamSynchronize(s));
    plan_unpair(plan);
  }
  const uint64_t nt = plan->n_tiles;
  if (nt == 0 || !plan->live) return BEAR_OK;
  dev_buf<uint16_t> live2, n_ent_dev;
  dev_buf<pln_tile> tp, tu;
  std::vector<uint16_t> n_ent;
  std::vector<pln_tile> host, hp, hu;
  try {
    n_ent.resize(nt);
    host.resize(nt);
  } catch (const std::bad_alloc &) {
    return BEAR_ERR_NOMEM;
  }
  HIP_TRY(live2.alloc(nt * LIN_LIVE2_STRIDE));
  HIP_TRY(n_ent_dev.alloc(nt));
  uint64_t blocks = nt;                   // one wave per tile
  if (blocks > (1u << 18)) blocks = 1u << 18;
  hipLaunchKernelGGL(plan_pair_kernel, dim3((unsigned)blocks), dim3(64), 0, s, plan->tiles, nt, plan->live,
                     reinterpret_cast<const unsigned long long *>(kmer_index), lag, live2.get(), n_ent_dev.get(),
                     getenv("BEAR_AMD_PAIR_NO_EMPTY") ? 0 : 1);     // (developer switch: the dealt order without the extra empty slots)
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(n_ent.data(), n_ent_dev.get(), nt * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(host.data(), plan->tiles, nt * sizeof(pln_tile), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  n_ent_dev.reset();
  uint64_t n_p = 0;
  try {
    for (uint64_t t = 0; t < nt; ++t) {
      pln_tile d = host[t];
      const bool fits = n_ent[t] != 0xffffu;         // (a tile without live contexts fits with 0 entries)
      d.pad = (t << 32) | (fits ? n_ent[t] : 0u);
      (fits ? hp : hu).push_back(d);
    }
    n_p = hp.size();
    // fewer than half of the tiles paired (a sparse table: runs of one context): nothing to gain, the plan stays as it was
    if (2 * n_p < nt) return BEAR_OK;
    const pln_tile zero = {};
    hp.insert(hp.end(), PLN_DESC_PAD, zero);
    hu.insert(hu.end(), PLN_DESC_PAD, zero);
  } catch (const std::bad_alloc &) {
    return BEAR_ERR_NOMEM;
  }
  HIP_TRY(tp.alloc(hp.size()));
  HIP_TRY(tu.alloc(hu.size()));
  HIP_TRY(hipMemcpy(tp.get(), hp.data(), hp.size() * sizeof(pln_tile), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(tu.get(), hu.data(), hu.size() * sizeof(pln_tile), hipMemcpyHostToDevice));
  plan->live2 = live2.release();
  plan->tiles_p = tp.release();
  plan->tiles_u = tu.release();
  plan->n_tiles_p = n_p;
  plan->n_tiles_u = nt - n_p;
  plan->pair_codes = kmer_index;
  plan->pair_lag = lag;
  plan->bytes += nt * LIN_LIVE2_STRIDE * sizeof(uint16_t) + (nt + 2 * PLN_DESC_PAD) * sizeof(pln_tile);
  if (paired) *paired = 1;
  return BEAR_OK;
}

int bear_plan_pair_info(const bear_plan *plan, uint64_t *paired_tiles, uint64_t *plain_tiles) {
  if (!plan) return BEAR_ERR_INVALID_ARG;
  if (paired_tiles) *paired_tiles = plan->live2 ? plan->n_tiles_p : 0;
  if (plain_tiles) *plain_tiles = plan->live2 ? plan->n_tiles_u : plan->n_tiles;
  return plan->live2 ? 1 : 0;
}

int bear_dm_linear_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const uint64_t *kmer_code,
                       const double *mat, int lag, uint64_t n_rows, double h_signed, double eps, int train_ar,
                       double *out, double *grad_mat, void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!plan || !out || !grad_mat || !mat || lag < 1 || lag > LIN_MAX_LAG) return BEAR_ERR_INVALID_ARG;
  if (check_plan_step(ws, plan, counts, n_rows, 5) != BEAR_OK) return BEAR_ERR_INVALID_ARG;
  if ((n_rows && !kmer_code) || misaligned(kmer_code) || misaligned8(out)) return BEAR_ERR_INVALID_ARG;
  if (!(eps >= 0.0) || !isfinite(h_signed)) return BEAR_ERR_INVALID_ARG;
  const bear_step_io io = ws_io(ws, nullptr, BEAR_THETA_NET, out);   // one launch: the last block sums the partials
  launch_linear(ws, plan, kmer_code, mat, lag, params_net(h_signed, eps), train_ar, io, grad_mat, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

// ---- the linear AR function as rows (kernels_linrows.h): evaluation, bear_ref with the linear net function ------------
static int linrows_grid(const bear_ws *ws, uint64_t n_rows) {
  return grid_capped((n_rows + LNR_THREADS - 1) / LNR_THREADS, (uint64_t)ws->num_cu);   // lin_partials holds num_cu blocks
}

int bear_linear_forward_f64(bear_ws *ws, const uint64_t *kmer_code, uint64_t n_rows, int lag, const double *mat, double *prior,
                            void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (lag < 1 || lag > LIN_MAX_LAG || !mat) return BEAR_ERR_INVALID_ARG;
  if (n_rows == 0) return BEAR_OK;
  if (!kmer_code || !prior || misaligned(prior) || misaligned8(kmer_code) || misaligned8(mat))
    return BEAR_ERR_INVALID_ARG;
  hipLaunchKernelGGL(linear_rows_forward_kernel, dim3(linrows_grid(ws, n_rows)), dim3(LNR_THREADS), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const unsigned long long *>(kmer_code), n_rows, mat, lag, prior);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_linear_backward_f64(bear_ws *ws, const uint64_t *kmer_code, uint64_t n_rows, int lag, const double *prior,
                             const double *grad_prior, double *grad_mat, void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (lag < 1 || lag > LIN_MAX_LAG || !grad_mat || misaligned8(grad_mat)) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_rows == 0) {
    HIP_TRY(hipMemsetAsync(grad_mat, 0, sizeof(double) * (size_t)lag * 25, s));
    return BEAR_OK;
  }
  if (!kmer_code || !prior || !grad_prior) return BEAR_ERR_INVALID_ARG;
  if (misaligned8(kmer_code) || misaligned8(prior) || misaligned8(grad_prior)) return BEAR_ERR_INVALID_ARG;
  hipLaunchKernelGGL(linear_rows_backward_kernel, dim3(linrows_grid(ws, n_rows)), dim3(LNR_THREADS), 0, s,
                     reinterpret_cast<const unsigned long long *>(kmer_code), n_rows, lag, prior, grad_prior, ws->lin_partials,
                     ws_arrival(ws), grad_mat);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

// ---- ... and at the protein alphabet's width (kernels_linrows_wide.h): int8 code rows, mat [lag, 21, 21] in LDS ----------------
// the backward grid is part of its result (the block partials are summed in a fixed order per grid); linw_partials holds its rows
static int linwide_bwd_grid(const bear_ws *ws, uint64_t n_rows) {
  return grid_capped((n_rows + LNW_BWD_TILE - 1) / LNW_BWD_TILE, (uint64_t)ws->num_cu * LNW_BWD_BLOCKS_PER_CU);
}

int bear_linear_forward_wide_f64(bear_ws *ws, const int8_t *codes, uint64_t n_rows, int lag, int width, const double *mat, double *prior,
                                 void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (width != LNW_W || lag < 1 || lag > LINEAR_WIDE_MAX_LAG || !mat || misaligned8(mat)) return BEAR_ERR_INVALID_ARG;
  if (n_rows == 0) return BEAR_OK;
  if (!codes || !prior || misaligned(prior)) return BEAR_ERR_INVALID_ARG;
  // one resident block per CU (its LDS holds mat and a tile of rows); the rows do not depend on the grid
  const int grid = grid_capped((n_rows + LNW_FWD_TILE - 1) / LNW_FWD_TILE, (uint64_t)ws->num_cu);
  hipLaunchKernelGGL(linear_wide_forward_kernel, dim3(grid), dim3(LNW_FWD_THREADS), LNW_FWD_LDS(lag), static_cast<hipStream_t>(stream),
                     codes, n_rows, lag, mat, prior);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_linear_backward_wide_f64(bear_ws *ws, const int8_t *codes, uint64_t n_rows, int lag, int width, const double *prior,
                                  const double *grad_prior, double *grad_mat, void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (width != LNW_W || lag < 1 || lag > LINEAR_WIDE_MAX_LAG || !grad_mat || misaligned8(grad_mat)) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_rows == 0) {
    HIP_TRY(hipMemsetAsync(grad_mat, 0, sizeof(double) * (size_t)lag * LNW_MAT, s));
    return BEAR_OK;
  }
  if (!codes || !prior || !grad_prior) return BEAR_ERR_INVALID_ARG;
  if (misaligned(codes) || misaligned(prior) || misaligned(grad_prior)) return BEAR_ERR_INVALID_ARG;
  hipLaunchKernelGGL(linear_wide_backward_kernel, dim3(linwide_bwd_grid(ws, n_rows)), dim3(LNW_BWD_THREADS), 0, s, codes, n_rows, lag, prior,
                     grad_prior, ws->linw_partials, ws_arrival(ws), grad_mat);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

// ---- bear_net's step with the linear AR function at the protein alphabet's width as one launch (kernels_linear_wide.h) ------------
// the grid is part of the result (block partials summed in a fixed order per grid); linw_partials holds a row per block
static int linstep_wide_grid(const bear_ws *ws, uint64_t n_rows) {
  return grid_capped((n_rows + LNW_BWD_TILE - 1) / LNW_BWD_TILE, (uint64_t)ws->num_cu * LSW_BLOCKS_PER_CU);
}

// the checks and the launch of all three entries: theta != NULL: h_signed and mat from the device-resident parameters (prm: eps only);
// `apply`: the block that sums the partials runs the update behind them.  n_rows == 0: one block, zeros (and the update).
static int launch_linear_wide(bear_ws *ws, const uint32_t *counts, const int8_t *codes, uint64_t n_rows, int lag, int width,
                              const double *mat, const double *theta, const bear_params &prm, int train_ar, double *packed, hipStream_t s,
                              const bear_apply_io &apply) {
  if (width != LNW_W || lag < 1 || lag > LINEAR_WIDE_MAX_LAG) return BEAR_ERR_INVALID_ARG;
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!packed || !mat || (n_rows && (!counts || !codes))) return BEAR_ERR_INVALID_ARG;
  if (misaligned(counts) || misaligned(codes) || misaligned8(mat) || misaligned8(packed) || !(prm.eps >= 0.0)) return BEAR_ERR_INVALID_ARG;
  const bear_step_io io = ws_io(ws, theta, BEAR_THETA_NET, packed);
  const double2 *lt = reinterpret_cast<const double2 *>(ws->logtab);
#define LIN_WIDE(AR)                                                                                                                   \
  hipLaunchKernelGGL((dm_linear_wide_kernel<AR>), dim3(linstep_wide_grid(ws, n_rows)), dim3(LSW_THREADS), LSW_LDS(lag), s, counts, codes, \
                     n_rows, lag, mat, prm, lt, ws->linw_partials, io, apply)
  BEAR_DISPATCH_1(train_ar, LIN_WIDE);
#undef LIN_WIDE
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_dm_linear_wide_f64(bear_ws *ws, const uint32_t *counts, const int8_t *codes, uint64_t n_rows, int lag, int width,
                            const double *mat, double h_signed, double eps, int train_ar, double *out, double *grad_mat, void *stream) {
  if (!out || !grad_mat || misaligned8(out) || misaligned8(grad_mat) || !isfinite(h_signed)) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the kernel leaves its sums as one packed vector: through the workspace, then to the caller's two arrays (same stream)
  int st = launch_linear_wide(ws, counts, codes, n_rows, lag, width, mat, nullptr, params_net(h_signed, eps), train_ar, ws ? ws->linw_packed : out,
                              s, NO_APPLY);
  if (st != BEAR_OK) return st;
  HIP_TRY(hipMemcpyAsync(out, ws->linw_packed, sizeof(double) * 2, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(grad_mat, ws->linw_packed + 2, sizeof(double) * (size_t)lag * LNW_MAT, hipMemcpyDeviceToDevice, s));
  return BEAR_OK;
}

int bear_net_linear_train_reduce_wide_f64(bear_ws *ws, const uint32_t *counts, const int8_t *codes, uint64_t n_rows, int lag, int width,
                                          const double *theta, double eps, int train_ar, double *packed, void *stream) {
  if (!theta || misaligned8(theta)) return BEAR_ERR_INVALID_ARG;
  return launch_linear_wide(ws, counts, codes, n_rows, lag, width, theta + 1, theta, params_eps(eps), train_ar, packed,
                            static_cast<hipStream_t>(stream), NO_APPLY);
}

int bear_net_linear_train_step_wide_f64(bear_ws *ws, const uint32_t *counts, const int8_t *codes, uint64_t n_rows, int lag, int width,
                                        double *theta, double *adam_m, double *adam_v, double *adam_t, double eps, int train_ar,
                                        double learning_rate, double scale, double *packed, double *loss_buf, uint64_t loss_cap,
                                        void *stream) {
  if (!theta || !adam_m || !adam_v || !adam_t) return BEAR_ERR_INVALID_ARG;
  if (misaligned8(theta) || misaligned8(adam_m) || misaligned8(adam_v) || misaligned8(adam_t) || misaligned8(loss_buf))
    return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (two_launch_step()) {
    int st = launch_linear_wide(ws, counts, codes, n_rows, lag, width, theta + 1, theta, params_eps(eps), train_ar, packed, s, NO_APPLY);
    if (st != BEAR_OK) return st;
    return launch_train_apply(theta, 1 + lag * LNW_MAT, packed, adam_m, adam_v, adam_t, learning_rate, scale, train_ar, loss_buf, loss_cap, s);
  }
  // ONE launch: the block that sums the partials runs the update behind them (bear_apply_in_block)
  return launch_linear_wide(ws, counts, codes, n_rows, lag, width, theta + 1, theta, params_eps(eps), train_ar, packed, s,
                            make_apply(theta, 1 + lag * LNW_MAT, adam_m, adam_v, adam_t, learning_rate, scale, train_ar, loss_buf, loss_cap));
}

// the shard's reduce of the linear head's step: constants from theta, sums by the last block (one launch, or two on a partly
// paired plan); with `apply` the last block of the step's last kernel runs the update behind its sums
static int linear_reduce(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const uint64_t *kmer_code, int lag, uint64_t n_rows,
                         const double *theta, double eps, int train_ar, double *packed, hipStream_t s, const bear_apply_io &apply) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!plan || !packed || !theta || lag < 1 || lag > LIN_MAX_LAG || !n_rows) return BEAR_ERR_INVALID_ARG;
  if (check_plan_step(ws, plan, counts, n_rows, 5) != BEAR_OK) return BEAR_ERR_INVALID_ARG;
  if (!kmer_code || misaligned(kmer_code) || misaligned8(packed)) return BEAR_ERR_INVALID_ARG;
  const bear_step_io io = ws_io(ws, theta, BEAR_THETA_NET, packed);
  launch_linear(ws, plan, kmer_code, theta + 1, lag, params_eps(eps), train_ar, io, packed + 2, s, apply);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_net_linear_train_reduce_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const uint64_t *kmer_code, int lag,
                                     uint64_t n_rows, const double *theta, double eps, int train_ar, double *packed, void *stream) {
  return linear_reduce(ws, plan, counts, kmer_code, lag, n_rows, theta, eps, train_ar, packed, static_cast<hipStream_t>(stream), NO_APPLY);
}

int bear_net_linear_train_step_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const uint64_t *kmer_code, int lag,
                                   uint64_t n_rows, double *theta, double *adam_m, double *adam_v, double *adam_t, double *packed,
                                   double eps, int train_ar, double learning_rate, double scale, double *loss_buf,
                                   uint64_t loss_cap, void *stream) {
  if (!adam_m || !adam_v || !adam_t) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (two_launch_step()) {
    int st = linear_reduce(ws, plan, counts, kmer_code, lag, n_rows, theta, eps, train_ar, packed, s, NO_APPLY);
    if (st != BEAR_OK) return st;
    return launch_train_apply(theta, 1 + lag * 25, packed, adam_m, adam_v, adam_t, learning_rate, scale, train_ar, loss_buf, loss_cap, s);
  }
  return linear_reduce(ws, plan, counts, kmer_code, lag, n_rows, theta, eps, train_ar, packed, s,
                       make_apply(theta, 1 + lag * 25, adam_m, adam_v, adam_t, learning_rate, scale, train_ar, loss_buf, loss_cap));
}

int launch_train_apply(double *theta, int n_theta, const double *packed, double *adam_m, double *adam_v, double *adam_t,
                              double learning_rate, double scale, int train_ar, double *loss_buf, uint64_t loss_cap, hipStream_t s) {
  hipLaunchKernelGGL(adam_vec_kernel, dim3(1), dim3(1024), 0, s,
                     make_apply(theta, n_theta, adam_m, adam_v, adam_t, learning_rate, scale, train_ar, loss_buf, loss_cap), packed);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_train_apply_f64(double *theta, int n_theta, const double *packed, double *adam_m, double *adam_v, double *adam_t,
                         double learning_rate, double scale, int train_ar, double *loss_buf, uint64_t loss_cap, void *stream) {
  if (!theta || !packed || !adam_m || !adam_v || !adam_t || n_theta < 1) return BEAR_ERR_INVALID_ARG;
  return launch_train_apply(theta, n_theta, packed, adam_m, adam_v, adam_t, learning_rate, scale, train_ar, loss_buf, loss_cap,
                            static_cast<hipStream_t>(stream));
}

// Developer probe: the paired lists (bear_plan_pair_contexts) of tiles [first, first + n) and their first rows, to the host
// (scripts/dev/pair_conflicts.py counts the bank-pair collisions of the triple adds from them).  A row is LIN_LIVE2_STRIDE uint16:
// [0] = entries m, [1] = 0, m entries, then lin_lev_len(m) level words; a call with lists == NULL returns that stride instead.
extern "C" int bear_debug_pair_lists(const bear_plan *plan, uint64_t first, uint64_t n, uint16_t *lists, uint64_t *row0) {
  if (!lists) return (int)LIN_LIVE2_STRIDE;
  if (!plan || !plan->live2 || !lists || !row0 || first + n > plan->n_tiles) return BEAR_ERR_INVALID_ARG;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(lists, plan->live2 + first * LIN_LIVE2_STRIDE, n * LIN_LIVE2_STRIDE * sizeof(uint16_t), hipMemcpyDeviceToHost));
  std::vector<pln_tile> t(n);
  HIP_TRY(hipMemcpy(t.data(), plan->tiles + first, n * sizeof(pln_tile), hipMemcpyDeviceToHost));
  for (uint64_t k = 0; k < n; ++k) row0[k] = t[k].row0;
  return BEAR_OK;
}
