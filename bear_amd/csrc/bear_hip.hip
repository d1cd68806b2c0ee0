// bear_hip.hip -- the C ABI (include/bear_hip.h) of the workspace and of the Dirichlet-multinomial steps on gfx950: status strings,
// workspace, synthetic tables and samplers; the row and sorted kernels (kernels_rows.h, kernels_sorted.h), plans and
// the planned mode-N / mode-R steps (kernels_plan.h, kernels_refplan.h), bear_ref's mixing (kernels_refmix.h, kernels_mixplan.h).
// The linear head, the convolutional head and evaluation are units of their own (bear_linear.hip, bear_cnn.hip, bear_eval.hip);
// what the units share on the host is in bear_host.h.
#include "bear_host.h"
#include "kernels_finalize.h"
#include "kernels_rows.h"
#include "kernels_sorted.h"
#include "kernels_plan.h"
#include "kernels_synth.h"
#include "kernels_refmix.h"
#include "kernels_mixplan.h"
#include "kernels_sample.h"
#include "kernels_refplan.h"

#ifdef PLN_STAMPS  // developer build: per-wave phase timers of dm_prior_plan_kernel land in ws->dbg
#define PLN_DBG_ARG , ws->dbg
#else
#define PLN_DBG_ARG
#endif

// ------------------------------------------------------------------ C ABI
extern "C" {

int bear_abi_version(void) { return BEAR_ABI_VERSION; }

const char *bear_strerror(int status) {
  switch (status) {
    case BEAR_OK: return "ok";
    case BEAR_ERR_INVALID_ARG: return "invalid argument (null or misaligned pointer, bad flag)";
    case BEAR_ERR_NO_DEVICE: return "no usable HIP device";
    case BEAR_ERR_WRONG_DEVICE: return "current HIP device differs from the workspace device";
    case BEAR_ERR_HIP: return "HIP runtime call failed (see bear_last_hip_error)";
    case BEAR_ERR_NOMEM: return "out of memory";
    case BEAR_ERR_IO: return "file could not be opened or read";
    case BEAR_ERR_PARSE: return "malformed count-table row";
    default: return "unknown bear status";
  }
}

int bear_last_hip_error(void) { return g_last_hip_error; }

// the dynamic-LDS limits of this unit's kernels (the other families: *_ws_setup, bear_host.h)
static int dm_kernels_setup() {
  int st = allow_dynamic_lds({BEAR_KFN(dm_prior_sorted_kernel<0>), BEAR_KFN(dm_prior_sorted_kernel<1>), BEAR_KFN(dm_prior_sorted_kernel<9>)},
                             sizeof(srt_lds_n));
  if (st == BEAR_OK) st = allow_dynamic_lds({BEAR_KFN(dm_ref_sorted_kernel)}, sizeof(srt_lds_r));
  if (st == BEAR_OK)
    st = allow_dynamic_lds({BEAR_KFN(dm_prior_plan_kernel<false, false>), BEAR_KFN(dm_prior_plan_kernel<true, false>),
                            BEAR_KFN(dm_prior_plan_kernel<true, true>)},
                           sizeof(pln_lds_n));
  if (st == BEAR_OK)
    st = allow_dynamic_lds({BEAR_KFN(dm_prior_plan_grad_kernel<false, false>), BEAR_KFN(dm_prior_plan_grad_kernel<true, true>),
                            BEAR_KFN(dm_refmix_plan_grad_kernel<false>), BEAR_KFN(dm_refmix_plan_grad_kernel<true>)},
                           sizeof(pln_lds_g));
  if (st == BEAR_OK) st = allow_dynamic_lds({BEAR_KFN(dm_prior_plan_grad_inplace_kernel)}, sizeof(pln_lds_gi));
  if (st == BEAR_OK) st = allow_dynamic_lds({BEAR_KFN(dm_ref_plan_kernel<false>), BEAR_KFN(dm_ref_plan_kernel<true>)}, sizeof(pln_lds_r));
  return st;
}

// Frees whatever the workspace holds so far (hipFree(NULL) does nothing) and the workspace itself: bear_ws_destroy, and
// bear_ws_create when anything fails half way.  The current device is the workspace's.
static void ws_release(bear_ws *ws) {
  (void)hipFree(ws->partials);
  (void)hipFree(ws->logtab);
  (void)hipFree(ws->dbg);
  (void)hipFree(ws->eval_partials);
  (void)hipFree(ws->eval_out);
  (void)hipFree(ws->lin_partials);
  (void)hipFree(ws->linw_partials);
  (void)hipFree(ws->linw_packed);
  (void)hipFree(ws->lin_accum);
  (void)hipFree(ws->cnn_partials);
  (void)hipFree(ws->cnnw_partials);
  (void)hipFree(ws->arrive);
  delete ws;
}

// the buffers every family uses, then each family's own kernels and buffers (bear_host.h)
static int ws_setup(bear_ws *ws) {
  HIP_TRY(hipMalloc(&ws->partials, sizeof(double) * BEAR_MAX_OUT * (size_t)ws->max_blocks));
  HIP_TRY(hipMalloc(&ws->logtab, sizeof(double) * 2 * BEAR_LOGTAB_N));
  HIP_TRY(hipMalloc(&ws->dbg, sizeof(unsigned long long) * 48 * (size_t)ws->max_blocks));
  HIP_TRY(hipMalloc(&ws->arrive, sizeof(unsigned long long) * BEAR_ARRIVE_WORDS));
  HIP_TRY(hipMemset(ws->arrive, 0, sizeof(unsigned long long) * BEAR_ARRIVE_WORDS));
  // {r_i, -log r_i}: r_i = 1 / midpoint of the i-th mantissa cell of [0.5, 1) (bear_log_tab)
  double tab[2 * BEAR_LOGTAB_N];
  for (int i = 0; i < BEAR_LOGTAB_N; ++i) {
    const double r = 1.0 / ((BEAR_LOGTAB_N + i + 0.5) / (2.0 * BEAR_LOGTAB_N));
    tab[2 * i] = r;
    tab[2 * i + 1] = -log(r);
  }
  HIP_TRY(hipMemcpy(ws->logtab, tab, sizeof(tab), hipMemcpyHostToDevice));
  int st = dm_kernels_setup();
  if (st == BEAR_OK) st = linear_ws_setup(ws);
  if (st == BEAR_OK) st = cnn_ws_setup(ws);
  if (st == BEAR_OK) st = eval_ws_setup(ws);
  return st;
}

struct ws_deleter {
  void operator()(bear_ws *ws) const { ws_release(ws); }
};

// (the workspace's device is current)
static int ws_create_on(int device, bear_ws **out) {
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  std::unique_ptr<bear_ws, ws_deleter> ws(new (std::nothrow) bear_ws());
  if (!ws) return BEAR_ERR_NOMEM;
  ws->device = device;
  ws->num_cu = prop.multiProcessorCount;
  ws->max_blocks = ws->num_cu * 8;
  ws->eval_blocks = ws->num_cu * 8;
  const int st = ws_setup(ws.get());
  if (st == BEAR_OK) *out = ws.release();
  return st;
}

int bear_ws_create(int device, bear_ws **out) {
  if (!out) return BEAR_ERR_INVALID_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return BEAR_ERR_NO_DEVICE;
  if (device < 0 || device >= count) return BEAR_ERR_INVALID_ARG;
  int prev = 0;
  HIP_TRY(hipGetDevice(&prev));
  HIP_TRY(hipSetDevice(device));
  const int st = ws_create_on(device, out);
  (void)hipSetDevice(prev);
  return st;
}

int bear_ws_destroy(bear_ws *ws) {
  if (!ws) return BEAR_OK;
  int prev = 0;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(ws->device);
  ws_release(ws);
  (void)hipSetDevice(prev);
  return BEAR_OK;
}

int bear_deterministic_build(void) {
#ifdef BEAR_DET_BUILD
  return 1;
#else
  return 0;
#endif
}

// the row kernels (a tile of BEAR_TILE_ROWS contexts per block pass) and the sorted ones (SRT_TILE; LDS: two resident blocks per CU)
static int grid_rows(const bear_ws *ws, uint64_t n_rows) { return grid_capped((n_rows + BEAR_TILE_ROWS - 1) / BEAR_TILE_ROWS, ws_blocks(ws, 2)); }
static int grid_sorted(const bear_ws *ws, uint64_t n_rows) { return grid_capped((n_rows + SRT_TILE - 1) / SRT_TILE, ws_blocks(ws, 2)); }
// ... and the streaming kernels of the dense plan form (kernels_rows.h, dm_prior_rows_kernel / dm_ref_rows_kernel)
static int grid_dense(const bear_ws *ws, uint64_t n_rows) {
  return grid_capped((n_rows + DPR_TILE_ROWS - 1) / DPR_TILE_ROWS, ws_blocks(ws, DPR_BLOCKS_PER_CU));
}

int bear_dm_prior_f64(bear_ws *ws, const uint32_t *counts, const double *prior, uint64_t n_rows,
                      double h_signed, double eps, int train_ar, double *out, double *grad_prior,
                      void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!out || (n_rows && (!counts || !prior))) return BEAR_ERR_INVALID_ARG;
  if (misaligned(counts) || misaligned(prior) || misaligned(grad_prior) || misaligned8(out)) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bear_params prm = params_net(h_signed, eps);
  int grid = grid_rows(ws, n_rows);
  if (!train_ar && !grad_prior) {
    grid = grid_sorted(ws, n_rows);
    const char *dbg = getenv("BEAR_DEBUG_STOP");  // developer switch: phase timing (results are then meaningless)
    const int stop = dbg ? atoi(dbg) : 0;
    const double2 *lt = reinterpret_cast<const double2 *>(ws->logtab);
    if (stop == 1)
      hipLaunchKernelGGL(dm_prior_sorted_kernel<1>, dim3(grid), dim3(SRT_THREADS), sizeof(srt_lds_n), s, counts, prior, n_rows, prm, lt, ws->partials, ws->dbg);
    else if (stop == 9)
      hipLaunchKernelGGL(dm_prior_sorted_kernel<9>, dim3(grid), dim3(SRT_THREADS), sizeof(srt_lds_n), s, counts, prior, n_rows, prm, lt, ws->partials, ws->dbg);
    else
      hipLaunchKernelGGL(dm_prior_sorted_kernel<0>, dim3(grid), dim3(SRT_THREADS), sizeof(srt_lds_n), s, counts, prior, n_rows, prm, lt, ws->partials, ws->dbg);
  } else {
#define PRIOR_LAUNCH(AR, GRAD)                                                                                                          \
  hipLaunchKernelGGL((dm_prior_kernel<AR, GRAD>), dim3(grid), dim3(BEAR_THREADS), 0, s, counts, prior, n_rows, prm, grad_prior, \
                     reinterpret_cast<const double2 *>(ws->logtab), ws->partials)
    BEAR_DISPATCH_2(train_ar, grad_prior, PRIOR_LAUNCH);
#undef PRIOR_LAUNCH
  }
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, s, ws->partials, grid, 2, out);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_dm_ref_f64(bear_ws *ws, const uint32_t *train, const uint32_t *ref, uint64_t n_rows,
                    double h_signed, double tau_signed, double nu_signed, double eps, int train_ar,
                    double *out, void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!out || (n_rows && (!train || !ref))) return BEAR_ERR_INVALID_ARG;
  if (misaligned(train) || misaligned(ref) || misaligned8(out)) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bear_params prm = params_ref(h_signed, tau_signed, nu_signed, eps);
  const double2 *lt = reinterpret_cast<const double2 *>(ws->logtab);
  int grid = grid_rows(ws, n_rows);
  if (train_ar || getenv("BEAR_ROWS_KERNEL")) {  // (BEAR mode: developer switch, the v1 row-per-thread kernel for A/B measurements)
#define REF_LAUNCH(AR) hipLaunchKernelGGL((dm_ref_kernel<AR>), dim3(grid), dim3(BEAR_THREADS), 0, s, train, ref, n_rows, prm, lt, ws->partials)
    BEAR_DISPATCH_1(train_ar, REF_LAUNCH);
#undef REF_LAUNCH
  } else {
    grid = grid_sorted(ws, n_rows);
    hipLaunchKernelGGL(dm_ref_sorted_kernel, dim3(grid), dim3(SRT_THREADS), sizeof(srt_lds_r), s, train, ref, n_rows, prm, lt, ws->partials);
  }
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, s, ws->partials, grid, 4, out);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

// ------------------------------------------------------------------ plans (struct bear_plan: bear_host.h)
// The sorted encoding of the table: tiles, their stream, the global lists.  Goes with the plan, or when a builder finds the table
// dense (bear_plan_create_auto, bear_plan_create_ref): the histograms are then all the plan keeps.
#define PLAN_HIST_WORDS (2 * SRT_NKEY + PLN_NBIG + 1)      // (+ the large totals' histogram)
static void plan_drop_sorted(bear_plan *p) {
  (void)hipFree(p->tiles);
  (void)hipFree(p->stream);
  (void)hipFree(p->heavy_col);
  (void)hipFree(p->heavy_row);
  (void)hipFree(p->heavy_stop);
  p->tiles = nullptr;
  p->stream = nullptr;
  p->heavy_col = nullptr;
  p->heavy_row = nullptr;
  p->heavy_stop = nullptr;
  p->n_tiles = 0;
  p->n_heavy[0] = p->n_heavy[1] = p->n_heavy[2] = 0;
  p->bytes = sizeof(unsigned long long) * PLAN_HIST_WORDS;
}
// ... the live lists of a five-column plan
static void plan_drop_live(bear_plan *p) {
  (void)hipFree(p->live);
  p->live = nullptr;
}
// ... the reference-aware extension (bear_plan_create_ref)
static void plan_drop_ref(bear_plan *p) {
  (void)hipFree(p->ref_items);
  (void)hipFree(p->hist0_base);
  (void)hipFree(p->heavy0);
  (void)hipFree(p->sum0);
  p->ref_items = nullptr;
  p->hist0 = p->hist0_base = nullptr;
  p->heavy0 = nullptr;
  p->sum0 = nullptr;
}

// every family drops the fields it owns (bear_host.h)
static void plan_free(bear_plan *p) {
  if (!p) return;
  plan_drop_sorted(p);
  plan_drop_live(p);
  (void)hipFree(p->hist);
  plan_drop_cnn_levels(p);
  plan_unpair(p);
  plan_drop_ref(p);
  delete p;
}
struct plan_deleter {
  void operator()(bear_plan *p) const { plan_free(p); }
};
using plan_guard = std::unique_ptr<bear_plan, plan_deleter>;      // holds a plan while it is built: a failed phase just returns

// ---- bear_plan_create, phase by phase.  Each returns a status; what one hands to the next, beyond the plan's own fields:
struct plan_scan {
  uint64_t n_quads = 0;
  dev_buf<uint8_t> quad;              // [3][n_quads] per group of PLN_QUAD contexts: product-path items, large-count cells, large-total rows
  dev_buf<unsigned long long> cnt;    // [0..2] heavy counts, [3..5] fill cursors, [6..8] sum of all counts, cells that hold one, largest count
  unsigned long long heavy[3] = {0, 0, 0};      // cnt[0..2] on the host: the sizes of the global lists
};
struct plan_cut {
  dev_buf<pln_tile> tiles;
  uint64_t n_tiles = 0, off16 = 0;    // off16: 16-byte units of the tiles' stream
  // + PLN_DESC_PAD zeroed descriptors: the kernels fetch descriptors 32 at a time (1 KiB LDS-DMA pieces)
  hipError_t alloc_tiles(uint64_t n) {
    n_tiles = n;
    return tiles.alloc_zeroed(n + PLN_DESC_PAD);
  }
};

// pass A: product-path items per group of 4 contexts, heavy counts, histograms, the table's totals
static int plan_scan_table(const bear_ws *ws, bear_plan *p, plan_scan &sc) {
  sc.n_quads = (p->n_rows + PLN_QUAD - 1) / PLN_QUAD;
  HIP_TRY(sc.quad.alloc(3 * sc.n_quads));
  HIP_TRY(sc.cnt.alloc_zeroed(9));
  const int grid = grid_capped((sc.n_quads + 255) / 256, (uint64_t)ws->num_cu * 8);
  hipLaunchKernelGGL(plan_scan_kernel, dim3(grid), dim3(256), 0, 0, p->counts, p->n_rows, p->ncol, sc.quad.get(), sc.cnt.get(), p->hist);
  HIP_TRY(hipGetLastError());
  unsigned long long h_total[3] = {0, 0, 0};
  HIP_TRY(hipMemcpy(sc.heavy, sc.cnt.get(), sizeof(sc.heavy), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h_total, sc.cnt.get() + 6, sizeof(h_total), hipMemcpyDeviceToHost));
  for (int k = 0; k < 3; ++k) p->count_total[k] = p->count_bound[k] = (double)h_total[k];
  return BEAR_OK;
}

// The tiles: greedy cut so that a tile holds <= PLN_NI items and <= PLN_RMAX contexts.  Either cut uses up the per-group counters.
// BEAR_PLAN_CUT=host: the sequential host loop over them (the definition; used by the tests to compare)
static int cut_on_host(const bear_plan *p, plan_scan &sc, plan_cut &cut) {
  const uint64_t n_quads = sc.n_quads, n_rows = p->n_rows;
  std::unique_ptr<uint8_t[]> h_quad(new (std::nothrow) uint8_t[3 * n_quads]);
  if (!h_quad) return hip_status(hipErrorOutOfMemory);
  HIP_TRY(hipMemcpy(h_quad.get(), sc.quad.get(), 3 * n_quads, hipMemcpyDeviceToHost));
  std::vector<pln_tile> tiles;
  uint64_t q = 0, off16 = 0;
  while (q < n_quads) {
    uint32_t items = 0, rows = 0, hcol = 0, hrow = 0;
    const uint64_t q0 = q;
    while (q < n_quads && rows + PLN_QUAD <= PLN_RMAX && items + h_quad[q] <= PLN_NI_CUT) {
      items += h_quad[q];
      hcol += h_quad[n_quads + q];
      hrow += h_quad[2 * n_quads + q];
      rows += PLN_QUAD;
      ++q;
    }
    pln_tile ti;
    memset(&ti, 0, sizeof(ti));
    ti.row0 = q0 * PLN_QUAD;
    if (ti.row0 + rows > n_rows) rows = (uint32_t)(n_rows - ti.row0);  // ragged end of the table
    // large-count items evaluated inside the tile (their rows are in LDS anyway); the surplus of very dense
    // tiles goes to the global lists.  Mode R needs no row data for large totals: they stay global.
    const uint32_t hc = hcol < PLN_HCAP ? hcol : PLN_HCAP;
    const uint32_t hr = p->ncol == 5 ? (hrow < PLN_HCAP ? hrow : PLN_HCAP) : 0u;
    ti.rows_items = (rows << 16) | items;
    ti.off16 = (uint32_t)off16;
    ti.hc_hr = (hc << 16) | hr;
    ti.blk16 = pln_block_layout(rows, items, hc, hr).end / 16;
    off16 += ti.blk16;
    if (off16 > 0xffffffffull) return hip_status(hipErrorOutOfMemory);     // plan stream beyond 2^32 16-byte units
    tiles.push_back(ti);
  }
  cut.off16 = off16;
  h_quad.reset();
  sc.quad.reset();
  HIP_TRY(cut.alloc_tiles(tiles.size()));
  HIP_TRY(hipMemcpy(cut.tiles.get(), tiles.data(), sizeof(pln_tile) * tiles.size(), hipMemcpyHostToDevice));
  return BEAR_OK;
}

// ... the same cut on the device (plan_cut_*_kernel): no per-group counters through the host
static int cut_on_device(const bear_plan *p, plan_scan &sc, plan_cut &cut) {
  const uint64_t n_quads = sc.n_quads;
  const uint32_t chunk = plan_cut_chunk(n_quads);
  const uint64_t n_chunks = (n_quads + chunk - 1) / chunk;
  dev_buf<uint32_t> walk;
  dev_buf<uint16_t> step;              // [n_quads] length of the tile that starts at a group
  dev_buf<uint64_t> entry;             // [n_chunks] entry | [n_chunks] base
  dev_buf<unsigned long long> meta;
  unsigned long long h_meta[3] = {0, 0, 0};
  HIP_TRY(walk.alloc(n_chunks * PLN_CUT_SPAN));
  HIP_TRY(step.alloc(n_quads));
  HIP_TRY(entry.alloc(2 * n_chunks));
  HIP_TRY(meta.alloc_zeroed(3));
  const uint64_t wb = (n_chunks * PLN_CUT_SPAN + 255) / 256;
  const unsigned cb = (unsigned)((n_chunks + 255) / 256);
  hipLaunchKernelGGL(plan_cut_step_kernel, dim3(cb), dim3(256), 0, 0, sc.quad.get(), n_quads, n_chunks, chunk, step.get());
  hipLaunchKernelGGL(plan_cut_walk_kernel, dim3((unsigned)wb), dim3(256), 0, 0, step.get(), n_quads, n_chunks, chunk, walk.get());
  hipLaunchKernelGGL(plan_cut_chain_kernel, dim3(1), dim3(1), 0, 0, walk.get(), n_chunks, chunk, entry.get(), entry.get() + n_chunks,
                     meta.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(h_meta, meta.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost));
  HIP_TRY(cut.alloc_tiles(h_meta[0]));
  hipLaunchKernelGGL(plan_cut_write_kernel, dim3(cb), dim3(256), 0, 0, sc.quad.get(), n_quads, p->n_rows, p->ncol, n_chunks, chunk, entry.get(),
                     entry.get() + n_chunks, cut.tiles.get());
  hipLaunchKernelGGL(plan_cut_offsets_kernel, dim3(1), dim3(1024), 0, 0, cut.tiles.get(), cut.n_tiles, meta.get());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(h_meta, meta.get(), sizeof(h_meta), hipMemcpyDeviceToHost));
  if (h_meta[2]) return hip_status(hipErrorOutOfMemory);     // plan stream beyond 2^32 16-byte units
  cut.off16 = h_meta[1];
  sc.quad.reset();
  return BEAR_OK;
}

// pass B: the tiles' stream and the global lists of what a tile could not keep (through the cursors cnt[3..5])
static int plan_fill(const bear_ws *ws, bear_plan *p, const plan_scan &sc, uint64_t stream_bytes) {
  HIP_TRY(hipMalloc(&p->stream, stream_bytes));
  HIP_TRY(hipMemset(p->stream, 0, stream_bytes));
  if (sc.heavy[0]) HIP_TRY(hipMalloc(&p->heavy_col, sizeof(pln_heavy_col) * sc.heavy[0]));
  if (sc.heavy[1]) HIP_TRY(hipMalloc(&p->heavy_row, sizeof(pln_heavy_row) * sc.heavy[1]));
  if (sc.heavy[2]) HIP_TRY(hipMalloc(&p->heavy_stop, sizeof(uint64_t) * sc.heavy[2]));
  const int grid = grid_capped(p->n_tiles, (uint64_t)ws->num_cu * 2);
  hipLaunchKernelGGL(plan_fill_kernel, dim3(grid), dim3(1024), 0, 0, p->counts, p->n_rows, p->ncol, p->tiles, p->n_tiles, p->stream,
                     p->heavy_col, p->heavy_row, p->heavy_stop, sc.cnt.get() + 3);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

// five-column plans: per-tile lists of the contexts that hold counts
static int plan_live_lists(const bear_ws *ws, bear_plan *p, uint64_t live_bytes) {
  HIP_TRY(hipMalloc(&p->live, live_bytes));
  HIP_TRY(hipMemset(p->live, 0, live_bytes));
  const int grid = grid_capped(p->n_tiles, (uint64_t)ws->num_cu * 2);
  hipLaunchKernelGGL(plan_live_kernel, dim3(grid), dim3(1024), 0, 0, p->tiles, p->n_tiles, p->stream, p->live);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

// The global lists were filled through atomic cursors, in whatever order the blocks got there: into row order (bear_levels.h).
// Neighbouring threads of the kernels that walk them then read neighbouring prior cells and -- the gradient fix-up -- update
// neighbouring gradient cells without atomics; and the lists are the same bits in every build of the plan.
// (lists of a few thousand entries -- every sparse k-mer table -- are left as they are: nothing to coalesce, and the sorts' set-up
// would triple the plan's build time; the deterministic build sorts them all)
static int plan_order_lists(bear_plan *p) {
#ifdef BEAR_DET_BUILD
  const uint64_t sort_from = 2;
#else
  const uint64_t sort_from = 1u << 16;
#endif
  int st = p->n_heavy[0] >= sort_from ? bear_canonical_order(p->heavy_col, p->n_heavy[0], 16, 0) : BEAR_OK;
  if (st == BEAR_OK && p->n_heavy[1] >= sort_from) st = bear_canonical_order(p->heavy_row, p->n_heavy[1], 16, 0);
  if (st == BEAR_OK && p->n_heavy[2] >= sort_from) st = bear_canonical_order(p->heavy_stop, p->n_heavy[2], 8, 0);
  return st;
}

// five-column plans: rows with a total of 1..SRT_CL (histogram) + rows with a larger one
static int plan_count_live_rows(bear_plan *p, const plan_scan &sc) {
  unsigned long long h_hist[SRT_NKEY];
  HIP_TRY(hipMemcpy(h_hist, p->hist, sizeof(h_hist), hipMemcpyDeviceToHost));
  unsigned long long live_rows = sc.heavy[1];
  for (int k = 0; k < SRT_NKEY; ++k) live_rows += h_hist[k];
  p->n_live_rows = live_rows;
  return BEAR_OK;
}

static int plan_build(const bear_ws *ws, bear_plan *p) {
  plan_scan sc;
  plan_cut cut;
  int st = plan_scan_table(ws, p, sc);
  if (st != BEAR_OK) return st;
  const char *cut_env = getenv("BEAR_PLAN_CUT");
  st = cut_env && cut_env[0] == 'h' ? cut_on_host(p, sc, cut) : cut_on_device(p, sc, cut);
  if (st != BEAR_OK) return st;
  p->tiles = cut.tiles.release();
  p->n_tiles = cut.n_tiles;
  const uint64_t stream_bytes = cut.off16 * 16 + 1024;  // slack: a DMA piece may be issued for a partial KiB
  const uint64_t live_bytes = p->ncol == 5 ? sizeof(uint16_t) * PLN_LIVE_STRIDE * (p->n_tiles + 1) : 0;   // + 1: DMA pieces are whole KiB
  st = plan_fill(ws, p, sc, stream_bytes);
  if (st == BEAR_OK && live_bytes) st = plan_live_lists(ws, p, live_bytes);
  if (st != BEAR_OK) return st;
  HIP_TRY(hipDeviceSynchronize());
  unsigned long long h_used[3] = {0, 0, 0};  // entries that actually went to the global lists
  HIP_TRY(hipMemcpy(h_used, sc.cnt.get() + 3, sizeof(h_used), hipMemcpyDeviceToHost));
  for (int k = 0; k < 3; ++k) p->n_heavy[k] = h_used[k];
  st = plan_order_lists(p);
  p->n_live_rows = p->n_rows;
  if (st == BEAR_OK && p->ncol == 5) st = plan_count_live_rows(p, sc);
  p->bytes = stream_bytes + live_bytes + sizeof(pln_tile) * p->n_tiles + sizeof(pln_heavy_col) * sc.heavy[0] +
             sizeof(pln_heavy_row) * sc.heavy[1] + sizeof(uint64_t) * sc.heavy[2];
  return st;
}

int bear_plan_create(bear_ws *ws, const uint32_t *counts, uint64_t n_rows, int ncol, bear_plan **out) {
  if (!out) return BEAR_ERR_INVALID_ARG;
  *out = nullptr;
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if ((ncol != 4 && ncol != 5) || (n_rows && !counts) || misaligned(counts)) return BEAR_ERR_INVALID_ARG;
  plan_guard p(new (std::nothrow) bear_plan());
  if (!p) return BEAR_ERR_NOMEM;
  memset(p.get(), 0, sizeof(bear_plan));
  p->device = ws->device;
  p->ncol = ncol;
  p->n_rows = n_rows;
  p->counts = counts;
  HIP_TRY(hipMalloc(&p->hist, sizeof(unsigned long long) * PLAN_HIST_WORDS));
  HIP_TRY(hipMemset(p->hist, 0, sizeof(unsigned long long) * PLAN_HIST_WORDS));
  if (n_rows) st = plan_build(ws, p.get());
  if (st == BEAR_OK) *out = p.release();
  return st;
}

int bear_plan_destroy(bear_plan *plan) {
  if (!plan) return BEAR_OK;
  int prev = 0;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(plan->device);
  plan_free(plan);
  (void)hipSetDevice(prev);
  return BEAR_OK;
}

uint64_t bear_plan_bytes(const bear_plan *plan) { return plan ? plan->bytes : 0; }

// ---- the dense form: a five-column plan that keeps nothing per item (kernels_rows.h, dm_prior_rows_kernel).  Internally ncol =
// PLAN_ROWS (bear_host.h): every entry point that walks a plan's tiles and lists asks for ncol == 5 and so turns such a plan away;
// the mode-N entry points (bear_dm_prior_plan_f64 / _grad_f64 / _dev_f64) take both.
int bear_plan_create_auto(bear_ws *ws, const uint32_t *counts, uint64_t n_rows, int *rowwise, bear_plan **out) {
  if (rowwise) *rowwise = 0;
  int st = bear_plan_create(ws, counts, n_rows, 5, out);
  if (st != BEAR_OK) return st;
  bear_plan *p = *out;
  // cells that hold a count (count_total[1]) against those the sorted encoding could not keep in its tiles (the global list of
  // large-count items): a table of large counts is all list
  const double cells = p->count_total[1], listed = (double)p->n_heavy[0];
  if (!(cells > 0.0) || listed * 2.0 <= cells) return BEAR_OK;
  plan_drop_sorted(p);             // (the histograms stay: nothing else does)
  plan_drop_live(p);
  p->ncol = PLAN_ROWS;
  if (rowwise) *rowwise = 1;
  return BEAR_OK;
}
// mode N on such a plan: one launch (the last block sums), parameters by value or from device memory
static int launch_prior_rows(bear_ws *ws, const bear_plan *plan, const double *prior, const bear_params &prm, const double *theta,
                             int train_ar, double *out, double *grad_prior, hipStream_t s) {
  const int grid = grid_dense(ws, plan->n_rows);
  const double2 *lt = reinterpret_cast<const double2 *>(ws->logtab);
  const bear_step_io io = ws_io(ws, theta, BEAR_THETA_NET, out);
#define ROWS_LAUNCH(AR, GRAD) \
  hipLaunchKernelGGL((dm_prior_rows_kernel<AR, GRAD>), dim3(grid), dim3(BEAR_THREADS), 0, s, plan->counts, prior, plan->n_rows, prm, grad_prior, lt, \
                     ws->partials, io)
  BEAR_DISPATCH_2(train_ar, grad_prior, ROWS_LAUNCH);
#undef ROWS_LAUNCH
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

uint64_t bear_plan_tile_count(const bear_plan *plan) { return plan ? plan->n_tiles : 0; }

int bear_plan_tile_info(const bear_plan *plan, uint64_t first, uint64_t count, uint64_t *row0, uint32_t *rows, uint32_t *items,
                        uint64_t *stream_offset) {
  if (!plan || first + count > plan->n_tiles || (count && (!row0 || !rows || !items || !stream_offset))) return BEAR_ERR_INVALID_ARG;
  if (!count) return BEAR_OK;
  std::vector<pln_tile> h(count);
  int prev = 0;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(plan->device);
  const hipError_t e = hipMemcpy(h.data(), plan->tiles + first, sizeof(pln_tile) * count, hipMemcpyDeviceToHost);
  (void)hipSetDevice(prev);
  HIP_TRY(e);
  for (uint64_t k = 0; k < count; ++k) {
    row0[k] = h[k].row0;
    rows[k] = h[k].rows_items >> 16;
    items[k] = h[k].rows_items & 0xffffu;
    stream_offset[k] = (uint64_t)h[k].off16 * 16;
  }
  return BEAR_OK;
}

int bear_plan_create_ref(bear_ws *ws, const uint32_t *train, const uint32_t *ref, uint64_t n_rows, bear_plan **out) {
  if (!out) return BEAR_ERR_INVALID_ARG;
  *out = nullptr;
  if ((n_rows && !ref) || misaligned(ref)) return BEAR_ERR_INVALID_ARG;
  bear_plan *created = nullptr;
  int st = bear_plan_create(ws, train, n_rows, 4, &created);   // tiles, histograms of totals / stop counts, heavy lists
  if (st != BEAR_OK) return st;
  plan_guard p(created);
  p->ref = ref;
  // a table of large counts (more than half of its cells beyond the sorted encoding's tiles: bear_plan_create_auto's test) keeps
  // nothing per item: the mode-R step then streams the training and reference rows, a context per thread (dm_ref_rows_kernel)
  if (p->count_total[1] > 0.0 && (double)p->n_heavy[0] * 2.0 > p->count_total[1]) {
    plan_drop_sorted(p.get());
    p->rows_ref = 1;
    *out = p.release();
    return BEAR_OK;
  }
  HIP_TRY(hipMalloc(&p->hist0_base, sizeof(unsigned long long) * 72));
  unsigned long long *d_meta = p->hist0_base;   // [0..31] bucket sizes / cursors, [32..63] hist0, [64] n_heavy0
  HIP_TRY(hipMemset(d_meta, 0, sizeof(unsigned long long) * 72));
  HIP_TRY(hipMalloc(&p->sum0, sizeof(double)));
  HIP_TRY(hipMemset(p->sum0, 0, sizeof(double)));
  unsigned long long h_meta[72];
  memset(h_meta, 0, sizeof(h_meta));
  const int grid = grid_capped((n_rows + 1023) / 1024, (uint64_t)ws->num_cu * 8);
  if (n_rows) {
    hipLaunchKernelGGL(rpl_build_kernel, dim3(grid), dim3(256), 0, 0, train, ref, n_rows, 0, d_meta, d_meta + 32, d_meta + 64, p->sum0,
                       static_cast<rpl_item *>(nullptr), static_cast<uint32_t *>(nullptr));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(h_meta, d_meta, sizeof(h_meta), hipMemcpyDeviceToHost));
  }
  unsigned long long run = 0, cur[RPL_NKEY];
  for (int k = 0; k < RPL_NKEY; ++k) {
    cur[k] = run;
    run += h_meta[k];
  }
  p->n_ref_items = run;
  p->n_heavy0 = h_meta[64];
  if (run) HIP_TRY(hipMalloc(&p->ref_items, sizeof(rpl_item) * run));
  if (p->n_heavy0) HIP_TRY(hipMalloc(&p->heavy0, sizeof(uint32_t) * p->n_heavy0));
  HIP_TRY(hipMemcpy(d_meta, cur, sizeof(cur), hipMemcpyHostToDevice));      // sizes -> cursors
  HIP_TRY(hipMemset(d_meta + 64, 0, sizeof(unsigned long long)));
  if (n_rows && (run || p->n_heavy0)) {
    hipLaunchKernelGGL(rpl_build_kernel, dim3(grid), dim3(256), 0, 0, train, ref, n_rows, 1, d_meta, d_meta + 32, d_meta + 64, p->sum0,
                       p->ref_items, p->heavy0);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipDeviceSynchronize());
#ifdef BEAR_DET_BUILD      // the records of a bucket stand in the order of the blocks' cursor bumps: canonical order per bucket
  for (int k = 0; k < RPL_NKEY && st == BEAR_OK; ++k) st = bear_canonical_order(p->ref_items + cur[k], h_meta[k], 16, 0);
  if (st == BEAR_OK) st = bear_canonical_order(p->heavy0, p->n_heavy0, 4, 0);
  if (st != BEAR_OK) return st;
#endif
  p->hist0 = d_meta + 32;
  p->bytes += sizeof(rpl_item) * p->n_ref_items + sizeof(uint32_t) * p->n_heavy0 + sizeof(unsigned long long) * 72;
  *out = p.release();
  return BEAR_OK;
}

// theta != NULL: the kernels derive their constants from the device-resident parameters (kind: BEAR_THETA_NET / _REF; prm.eps is
// still read from `prm`).  Either way ONE launch: the last block to finish writes the fixed-order sums to `out`.
static int launch_prior_plan(bear_ws *ws, const bear_plan *plan, const double *prior, uint64_t n_rows, const bear_params &prm,
                             const double *theta, int train_ar, int prior_normalized, double *out, hipStream_t s) {
  const int grid = grid_plan(ws, plan->n_tiles);
  const double2 *lt = reinterpret_cast<const double2 *>(ws->logtab);
  const bear_step_io io = ws_io(ws, theta, BEAR_THETA_NET, out);
  if (train_ar)
    hipLaunchKernelGGL((dm_prior_plan_kernel<true, true>), dim3(grid), dim3(PLN_THREADS), sizeof(pln_lds_n), s, prior, n_rows, prm,
                       plan_view(plan), lt, ws->partials, io PLN_DBG_ARG);
  else if (prior_normalized)
    hipLaunchKernelGGL((dm_prior_plan_kernel<true, false>), dim3(grid), dim3(PLN_THREADS), sizeof(pln_lds_n), s, prior, n_rows, prm,
                       plan_view(plan), lt, ws->partials, io PLN_DBG_ARG);
  else
    hipLaunchKernelGGL((dm_prior_plan_kernel<false, false>), dim3(grid), dim3(PLN_THREADS), sizeof(pln_lds_n), s, prior, n_rows, prm,
                       plan_view(plan), lt, ws->partials, io PLN_DBG_ARG);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_dm_prior_plan_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const double *prior,
                           uint64_t n_rows, double h_signed, double eps, int train_ar, int prior_normalized,
                           double *out, void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!plan || !out || (n_rows && (!counts || !prior))) return BEAR_ERR_INVALID_ARG;
  if (check_plan_step(ws, plan, counts, n_rows, 5, true) != BEAR_OK || misaligned(prior) || misaligned8(out)) return BEAR_ERR_INVALID_ARG;
  const bear_params prm = params_net(h_signed, eps);
  if (plan_is_rows(plan)) return launch_prior_rows(ws, plan, prior, prm, nullptr, train_ar, out, nullptr, static_cast<hipStream_t>(stream));
  return launch_prior_plan(ws, plan, prior, n_rows, prm, nullptr, train_ar, prior_normalized, out, static_cast<hipStream_t>(stream));
}

int launch_prior_plan_grad(bear_ws *ws, const bear_plan *plan, const double *prior, const bear_params &prm,
                                  const double *theta, int train_ar, int prior_normalized, double *out, double *grad_prior,
                                  hipStream_t s) {
  const int grid = grid_plan(ws, plan->n_tiles);
  const double2 *lt = reinterpret_cast<const double2 *>(ws->logtab);
  const pln_view pv = plan_view(plan);
  const bear_step_io io = ws_io(ws, theta, BEAR_THETA_NET, out);
  if (train_ar)
    hipLaunchKernelGGL((dm_prior_plan_grad_kernel<true, true>), dim3(grid), dim3(PLN_THREADS), sizeof(pln_lds_g), s, prior, prm, pv, lt,
                       grad_prior, ws->partials, io);
  else if (prior_normalized)   // rows asserted normalised: the in-place, double-buffered form
    hipLaunchKernelGGL(dm_prior_plan_grad_inplace_kernel, dim3(grid), dim3(PLN_THREADS), sizeof(pln_lds_gi), s, prior, prm, pv, lt,
                       grad_prior, ws->partials, io);
  else
    hipLaunchKernelGGL((dm_prior_plan_grad_kernel<false, false>), dim3(grid), dim3(PLN_THREADS), sizeof(pln_lds_g), s, prior, prm, pv, lt,
                       grad_prior, ws->partials, io);
  HIP_TRY(hipGetLastError());
  // the plan's global overflow lists (dense tables): the contexts' base, then the column items (kernels_plan.h)
  auto fixup_grid = [&](uint64_t nh) { return grid_capped((nh + 255) / 256, (uint64_t)ws->num_cu * 8); };
#define FIXUP(NORM, AR, ROWS, N) \
  hipLaunchKernelGGL((dm_prior_grad_fixup_kernel<NORM, AR, ROWS>), dim3(fixup_grid(N)), dim3(256), 0, s, prior, prm, pv, lt, grad_prior, io)
  if (pv.n_heavy_row && !train_ar) {
    if (prior_normalized) FIXUP(true, false, true, pv.n_heavy_row);
    else FIXUP(false, false, true, pv.n_heavy_row);
  }
  if (pv.n_heavy_col) {
    if (train_ar) FIXUP(true, true, false, pv.n_heavy_col);
    else if (prior_normalized) FIXUP(true, false, false, pv.n_heavy_col);
    else FIXUP(false, false, false, pv.n_heavy_col);
  }
#undef FIXUP
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_dm_prior_plan_grad_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const double *prior,
                                uint64_t n_rows, double h_signed, double eps, int train_ar, int prior_normalized,
                                double *out, double *grad_prior, void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!plan || !out || !grad_prior || (n_rows && (!counts || !prior))) return BEAR_ERR_INVALID_ARG;
  if (check_plan_step(ws, plan, counts, n_rows, 5, true) != BEAR_OK) return BEAR_ERR_INVALID_ARG;
  if (misaligned(prior) || misaligned(grad_prior) || misaligned8(out)) return BEAR_ERR_INVALID_ARG;
  const bear_params prm = params_net(h_signed, eps);
  if (plan_is_rows(plan)) return launch_prior_rows(ws, plan, prior, prm, nullptr, train_ar, out, grad_prior, static_cast<hipStream_t>(stream));
  return launch_prior_plan_grad(ws, plan, prior, prm, nullptr, train_ar, prior_normalized, out, grad_prior,
                                static_cast<hipStream_t>(stream));
}

// h_signed read from device memory (a parameter the optimizer updates on the device): the step is enqueued without the host
// reading the parameter back.  grad_prior may be NULL (parameter-free ar_func: nothing to feed back).
int bear_dm_prior_plan_dev_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const double *prior, uint64_t n_rows,
                               const double *h_signed_dev, double eps, int train_ar, int prior_normalized, double *out,
                               double *grad_prior, void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!plan || !out || !h_signed_dev || (n_rows && (!counts || !prior))) return BEAR_ERR_INVALID_ARG;
  if (check_plan_step(ws, plan, counts, n_rows, 5, true) != BEAR_OK) return BEAR_ERR_INVALID_ARG;
  if (misaligned(prior) || misaligned(grad_prior) || misaligned8(out)) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bear_params only_eps = params_eps(eps);
  if (plan_is_rows(plan)) return launch_prior_rows(ws, plan, prior, only_eps, h_signed_dev, train_ar, out, grad_prior, s);
  if (grad_prior) return launch_prior_plan_grad(ws, plan, prior, only_eps, h_signed_dev, train_ar, prior_normalized, out, grad_prior, s);
  return launch_prior_plan(ws, plan, prior, n_rows, only_eps, h_signed_dev, train_ar, prior_normalized, out, s);
}

// bear_ref's step for a net function with parameters: the reference mixing inside the DM step (kernels_mixplan.h)
int bear_dm_refmix_plan_grad_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const double *net_rows,
                                 const double *ref_rows, uint64_t n_rows, const double *h_signed_dev, const double *tau_signed_dev,
                                 const double *net_weight_signed_dev, double eps, int train_ar, double *out, double *grad_net_rows,
                                 void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!plan || !out || !h_signed_dev || !tau_signed_dev || !net_weight_signed_dev) return BEAR_ERR_INVALID_ARG;
  if (n_rows && (!counts || !net_rows || !ref_rows || !grad_net_rows)) return BEAR_ERR_INVALID_ARG;
  if (check_plan_step(ws, plan, counts, n_rows, 5) != BEAR_OK) return BEAR_ERR_INVALID_ARG;
  if (misaligned(net_rows) || misaligned(ref_rows) || misaligned(grad_net_rows) || misaligned8(out) || misaligned8(h_signed_dev) ||
      misaligned8(tau_signed_dev) || misaligned8(net_weight_signed_dev) || !(eps >= 0.0))
    return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int grid = grid_plan(ws, plan->n_tiles);
  const double2 *lt = reinterpret_cast<const double2 *>(ws->logtab);
  const pln_view pv = plan_view(plan);
  const bear_step_io io = ws_io(ws, nullptr, BEAR_THETA_REF, out);
#define MIX_LAUNCH(AR)                                                                                                            \
  hipLaunchKernelGGL(dm_refmix_plan_grad_kernel<AR>, dim3(grid), dim3(PLN_THREADS), sizeof(pln_lds_g), s, net_rows, ref_rows, \
                     h_signed_dev, tau_signed_dev, net_weight_signed_dev, eps, pv, lt, grad_net_rows, ws->partials, io)
  BEAR_DISPATCH_1(train_ar, MIX_LAUNCH);
#undef MIX_LAUNCH
  HIP_TRY(hipGetLastError());
  if (pv.n_heavy_col + pv.n_heavy_row) {
    const uint64_t nh = pv.n_heavy_col + pv.n_heavy_row;
    const int g2 = grid_capped((nh + 255) / 256, (uint64_t)ws->num_cu * 4);
#define MIX_FIXUP(AR)                                                                                                      \
  hipLaunchKernelGGL(dm_refmix_fixup_kernel<AR>, dim3(g2), dim3(256), 0, s, net_rows, ref_rows, h_signed_dev, tau_signed_dev, \
                     net_weight_signed_dev, eps, pv, lt, grad_net_rows)
    BEAR_DISPATCH_1(train_ar, MIX_FIXUP);
#undef MIX_FIXUP
    HIP_TRY(hipGetLastError());
  }
  return BEAR_OK;
}

// The mode-R step on a plan: the reference-aware item stream when the plan was built with this reference column
// (bear_plan_create_ref), the streaming kernel otherwise.  theta != NULL: constants from the device-resident parameters.

static int launch_ref_plan(bear_ws *ws, const bear_plan *plan, const uint32_t *ref, uint64_t n_rows, const bear_params &prm,
                           const double *theta, int train_ar, double *out, hipStream_t s, const bear_apply_io &apply = NO_APPLY) {
  const double2 *lt = reinterpret_cast<const double2 *>(ws->logtab);
  const bear_step_io io = ws_io(ws, theta, BEAR_THETA_REF, out);
  int grid;
  if (plan->rows_ref) {       // the dense form: rows streamed (kernels_rows.h)
    if (plan->ref != ref) return BEAR_ERR_INVALID_ARG;
    grid = grid_dense(ws, n_rows);
#define REF_ROWS(AR) \
  hipLaunchKernelGGL(dm_ref_rows_kernel<AR>, dim3(grid), dim3(BEAR_THREADS), 0, s, plan->counts, ref, n_rows, prm, lt, ws->partials, io, apply)
    BEAR_DISPATCH_1(train_ar, REF_ROWS);
#undef REF_ROWS
  } else if (plan->ref) {
    if (plan->ref != ref) return BEAR_ERR_INVALID_ARG;   // the plan is valid for the reference buffer it was built from
    rpl_view rv;
    rv.items = plan->ref_items;
    rv.n_items = plan->n_ref_items;
    rv.hist0 = plan->hist0;
    rv.heavy0 = plan->heavy0;
    rv.n_heavy0 = plan->n_heavy0;
    rv.sum0 = plan->sum0;
    // 4 waves per block; blocks per CU by measurement (scripts/dev/cfg1_grid.py: a block's fixed work -- the log table into LDS, its
    // partials, two arrival atomics, its share of the last block's sum -- against the balance of more blocks): configs[1] (1e7
    // contexts, ~3e4 units) 25.3 / 23.9 / 22.2 / 23.4 / 27.3 us per step on 8 / 6 / 4 / 3 / 2 blocks per CU, configs[3] (1.25e8
    // contexts, ~4e5 units) 160 / 154 / 174 / 196 / 256 us
    const uint64_t units = (plan->n_ref_items + 63) / 64, want = (units + 3) / 4 + 2, cap = (uint64_t)ws->num_cu * (units > 131072 ? 6 : 4);
    grid = grid_capped(want, cap);
#define REF_ITEMS(AR) \
  hipLaunchKernelGGL(dm_ref_items_kernel<AR>, dim3(grid), dim3(256), 0, s, prm, rv, plan_view(plan), lt, ws->partials, io, apply)
    BEAR_DISPATCH_1(train_ar, REF_ITEMS);
#undef REF_ITEMS
  } else {
    grid = grid_plan(ws, plan->n_tiles);
#define REF_PLAN(AR)                                                                                                                     \
  hipLaunchKernelGGL(dm_ref_plan_kernel<AR>, dim3(grid), dim3(PLN_THREADS), sizeof(pln_lds_r), s, ref, n_rows, prm, plan_view(plan), lt, \
                     ws->partials, io, apply)
    BEAR_DISPATCH_1(train_ar, REF_PLAN);
#undef REF_PLAN
  }
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_dm_ref_plan_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *train, const uint32_t *ref,
                         uint64_t n_rows, double h_signed, double tau_signed, double nu_signed, double eps,
                         int train_ar, double *out, void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!plan || !out || (n_rows && (!train || !ref))) return BEAR_ERR_INVALID_ARG;
  if (check_plan_step(ws, plan, train, n_rows, 4) != BEAR_OK || misaligned(ref) || misaligned8(out)) return BEAR_ERR_INVALID_ARG;
  return launch_ref_plan(ws, plan, ref, n_rows, params_ref(h_signed, tau_signed, nu_signed, eps), nullptr, train_ar, out,
                         static_cast<hipStream_t>(stream));
}

// the shard's reduce of bear_ref's own step, constants from theta; with `apply` the last block runs the update behind its sums
static int ref_reduce(bear_ws *ws, const bear_plan *plan, const uint32_t *train, const uint32_t *ref, uint64_t n_rows, const double *theta,
                      double eps, int train_ar, double *packed, hipStream_t s, const bear_apply_io &apply) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!plan || !packed || !theta || !n_rows || !train || !ref) return BEAR_ERR_INVALID_ARG;
  if (check_plan_step(ws, plan, train, n_rows, 4) != BEAR_OK || misaligned(ref) || misaligned8(packed)) return BEAR_ERR_INVALID_ARG;
  return launch_ref_plan(ws, plan, ref, n_rows, params_eps(eps), theta, train_ar, packed, s, apply);
}

int bear_ref_train_reduce_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *train, const uint32_t *ref, uint64_t n_rows,
                              const double *theta, double eps, int train_ar, double *packed, void *stream) {
  return ref_reduce(ws, plan, train, ref, n_rows, theta, eps, train_ar, packed, static_cast<hipStream_t>(stream), NO_APPLY);
}

int bear_ref_train_step_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *train, const uint32_t *ref, uint64_t n_rows,
                            double *theta, double *adam_m, double *adam_v, double *adam_t, double eps, int train_ar,
                            double learning_rate, double scale, double *out, double *loss_buf, uint64_t loss_cap, void *stream) {
  if (!adam_m || !adam_v || !adam_t) return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (two_launch_step()) {
    int st = ref_reduce(ws, plan, train, ref, n_rows, theta, eps, train_ar, out, s, NO_APPLY);
    if (st != BEAR_OK) return st;
    return launch_train_apply(theta, 3, out, adam_m, adam_v, adam_t, learning_rate, scale, train_ar, loss_buf, loss_cap, s);
  }
  // ONE launch: the last block of the reduce kernel runs the update behind its sums (bear_apply_in_block)
  return ref_reduce(ws, plan, train, ref, n_rows, theta, eps, train_ar, out, s,
                    make_apply(theta, 3, adam_m, adam_v, adam_t, learning_rate, scale, train_ar, loss_buf, loss_cap));
}

int bear_dm_items_f64(bear_ws *ws, const double *x, const uint32_t *c, uint64_t n, int path, double *D, double *P,
                      void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (n == 0) return BEAR_OK;
  if (!x || !c || !D || !P || path < 0 || path > 2) return BEAR_ERR_INVALID_ARG;
  uint64_t blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffull) return BEAR_ERR_INVALID_ARG;
  hipLaunchKernelGGL(dm_items_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), x, c, n, path,
                     reinterpret_cast<const double2 *>(ws->logtab), D, P);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_plan_count_total(const bear_plan *plan, double *total, double *bound) {
  if (!plan) return BEAR_ERR_INVALID_ARG;
  for (int k = 0; k < 3; ++k) {
    if (total) total[k] = plan->count_total[k];
    if (bound) bound[k] = plan->count_bound[k];
  }
  return BEAR_OK;
}

int bear_plan_set_count_bound(bear_plan *plan, const double *bound) {
  if (!plan || !bound) return BEAR_ERR_INVALID_ARG;
  for (int k = 0; k < 3; ++k)
    if (!(bound[k] >= plan->count_total[k]) || !(bound[k] < 0x1p50)) return BEAR_ERR_INVALID_ARG;
  for (int k = 0; k < 3; ++k) plan->count_bound[k] = bound[k];
  return BEAR_OK;
}

// ---- bear_ref's prior rows for a parametrised net function (kernels_refmix.h) ---------------------------------------------
static int refmix_grid(const bear_ws *ws, uint64_t n_rows) { return grid_capped((n_rows + RMX_THREADS - 1) / RMX_THREADS, ws_blocks(ws, 2)); }

int bear_ref_mix_forward_f64(bear_ws *ws, const double *net_rows, const double *ref_rows, uint64_t n_rows, const double *tau_signed,
                             const double *net_weight_signed, double *prior, void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!tau_signed || !net_weight_signed || misaligned8(tau_signed) || misaligned8(net_weight_signed)) return BEAR_ERR_INVALID_ARG;
  if (n_rows == 0) return BEAR_OK;
  if (!net_rows || !ref_rows || !prior || misaligned(net_rows) || misaligned(ref_rows) || misaligned(prior)) return BEAR_ERR_INVALID_ARG;
  hipLaunchKernelGGL(ref_mix_forward_kernel, dim3(refmix_grid(ws, n_rows)), dim3(RMX_THREADS), 0, static_cast<hipStream_t>(stream),
                     net_rows, ref_rows, tau_signed, net_weight_signed, n_rows, prior);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_ref_mix_backward_f64(bear_ws *ws, const double *net_rows, const double *ref_rows, const double *grad_prior, uint64_t n_rows,
                              const double *tau_signed, const double *net_weight_signed, double *grad_net_rows, double *grad_scalars,
                              void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!tau_signed || !net_weight_signed || !grad_scalars || misaligned8(tau_signed) || misaligned8(net_weight_signed) ||
      misaligned8(grad_scalars))
    return BEAR_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_rows == 0) {
    HIP_TRY(hipMemsetAsync(grad_scalars, 0, 2 * sizeof(double), s));
    return BEAR_OK;
  }
  if (!net_rows || !ref_rows || !grad_prior || !grad_net_rows || misaligned(net_rows) || misaligned(ref_rows) ||
      misaligned(grad_prior) || misaligned(grad_net_rows))
    return BEAR_ERR_INVALID_ARG;
  hipLaunchKernelGGL(ref_mix_backward_kernel, dim3(refmix_grid(ws, n_rows)), dim3(RMX_THREADS), 0, s, net_rows, ref_rows, grad_prior,
                     tau_signed, net_weight_signed, n_rows, grad_net_rows, ws->partials, ws_arrival(ws), grad_scalars);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

// Developer probe (not part of include/bear_hip.h): resident blocks per CU the runtime reports for
// the two sorted kernels at their dynamic-LDS sizes.
// Developer probe: copies the phase-timing buffer written by BEAR_DEBUG_STOP=9 (n u64 words) to the host.
int bear_debug_read_timing(bear_ws *ws, unsigned long long *host, int n_words) {
  if (!ws || !host) return BEAR_ERR_INVALID_ARG;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(host, ws->dbg, sizeof(unsigned long long) * (size_t)n_words, hipMemcpyDeviceToHost));
  return BEAR_OK;
}

int bear_debug_occupancy(int which) {
  int nb = -1;
  hipError_t e = which == 0
      ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, dm_prior_sorted_kernel<0>, SRT_THREADS, sizeof(srt_lds_n))
      : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, dm_ref_sorted_kernel, SRT_THREADS, sizeof(srt_lds_r));
  return e != hipSuccess ? -1000 - (int)e : nb;
}

int bear_log_gamma_f64(const double *conc, uint64_t n, uint64_t n_samples, uint64_t seed, double *out, void *stream) {
  if (n == 0 || n_samples == 0) return BEAR_OK;
  if (!conc || !out) return BEAR_ERR_INVALID_ARG;
  if (n_samples > (~0ull) / n) return BEAR_ERR_INVALID_ARG;
  const uint64_t total = n * n_samples;
  uint64_t blocks = (total + SMP_THREADS - 1) / SMP_THREADS;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(log_gamma_kernel, dim3((unsigned)blocks), dim3(SMP_THREADS), 0, static_cast<hipStream_t>(stream), conc, n,
                     n_samples, seed, out);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

// bear_logdir_sample_f64 and its width-taking twin: rows of `width` letters (5 or 21)
static int logdir_sample_launch(const uint32_t *counts, const double *prior, uint64_t n_rows, int width, const double *h,
                                int n_h, int with_ar, const double *van, int n_van, int mc_samples, int map, uint64_t seed,
                                uint64_t row_base, double *out, void *stream) {
  if (n_h < 0 || n_van < 0 || n_h + n_van > SMP_MAX_MODELS || (n_h && !h) || (n_van && !van)) return BEAR_ERR_INVALID_ARG;
  if (with_ar && !map) return BEAR_ERR_INVALID_ARG;   // the AR model enters only the MAP table (get_var_probs.py:150-153)
  if (map) mc_samples = 1;                            // get_var_probs.py:131-132
  if (mc_samples <= 0) return BEAR_ERR_INVALID_ARG;
  const int M = (with_ar ? 1 : 0) + n_h + n_van;
  if (n_rows == 0 || M == 0) return BEAR_OK;
  if (!out || ((n_h || with_ar) && !prior)) return BEAR_ERR_INVALID_ARG;
  smp_args A;
  memset(&A, 0, sizeof(A));
  A.n_h = n_h;
  A.n_van = n_van;
  A.arm = with_ar ? 1 : 0;
  A.has_counts = counts ? 1 : 0;
  A.has_prior = prior ? 1 : 0;
  A.map = map ? 1 : 0;
  A.mc = (uint32_t)mc_samples;
  A.seed = seed;
  A.row_base = row_base;
  for (int j = 0; j < n_h; ++j) {
    if (!(h[j] > 0.0)) return BEAR_ERR_INVALID_ARG;
    A.w[j] = 1.0 / h[j];
  }
  for (int k = 0; k < n_van; ++k) A.w[n_h + k] = van[k];
  const uint64_t per_row = (uint64_t)M * (uint64_t)mc_samples;
  if (per_row > 0xffffffffull || n_rows > (~0ull) / ((uint64_t)width * per_row)) return BEAR_ERR_INVALID_ARG;
  uint64_t blocks = (n_rows * per_row + SMP_THREADS - 1) / SMP_THREADS;
  if (blocks > 65536) blocks = 65536;
  hipStream_t s = static_cast<hipStream_t>(stream);
  BEAR_DISPATCH_W(width, hipLaunchKernelGGL(logdir_sample_kernel<W>, dim3((unsigned)blocks), dim3(SMP_THREADS), 0, s, counts, prior, n_rows, A, out));
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_logdir_sample_f64(const uint32_t *counts, const double *prior, uint64_t n_rows, const double *h, int n_h,
                           int with_ar, const double *van, int n_van, int mc_samples, int map, uint64_t seed,
                           uint64_t row_base, double *out, void *stream) {
  return logdir_sample_launch(counts, prior, n_rows, 5, h, n_h, with_ar, van, n_van, mc_samples, map, seed, row_base, out, stream);
}

int bear_logdir_sample_wide_f64(const uint32_t *counts, const double *prior, uint64_t n_rows, int width, const double *h,
                                int n_h, int with_ar, const double *van, int n_van, int mc_samples, int map, uint64_t seed,
                                uint64_t row_base, double *out, void *stream) {
  if (!wide_width_ok(width)) return BEAR_ERR_INVALID_ARG;
  return logdir_sample_launch(counts, prior, n_rows, width, h, n_h, with_ar, van, n_van, mc_samples, map, seed, row_base, out,
                              stream);
}

int bear_stream_read(bear_ws *ws, const void *src, uint64_t n_bytes, void *stream) {
  int st = check_ws(ws);
  if (st != BEAR_OK) return st;
  if (!src || misaligned(src)) return BEAR_ERR_INVALID_ARG;
  hipLaunchKernelGGL(stream_read_kernel, dim3(ws->num_cu * 16), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint4 *>(src), n_bytes / 16, reinterpret_cast<uint32_t *>(ws->dbg));
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_synth_counts_u32(uint64_t seed, uint64_t row0, uint64_t n_rows, int dense, uint32_t *train,
                          uint32_t *test, uint32_t *ref, void *stream) {
  if (n_rows == 0) return BEAR_OK;
  if (!train && !test && !ref) return BEAR_ERR_INVALID_ARG;
  uint64_t blocks = (n_rows + 255) / 256;
  if (blocks > 0x7fffffffull) return BEAR_ERR_INVALID_ARG;
  hipLaunchKernelGGL(synth_counts_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), seed, row0, n_rows, dense, train, test, ref);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

int bear_synth_prior_f64(uint64_t seed, uint64_t row0, uint64_t n_rows, double *prior, void *stream) {
  if (n_rows == 0) return BEAR_OK;
  if (!prior) return BEAR_ERR_INVALID_ARG;
  uint64_t blocks = (n_rows + 255) / 256;
  if (blocks > 0x7fffffffull) return BEAR_ERR_INVALID_ARG;
  hipLaunchKernelGGL(synth_prior_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), seed, row0, n_rows, prior);
  HIP_TRY(hipGetLastError());
  return BEAR_OK;
}

}  // extern "C"