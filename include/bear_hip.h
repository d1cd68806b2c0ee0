/*
 * bear_hip.h -- C ABI of libbear_hip.so: the MI355X (gfx950) implementation of BEAR's
 * empirical-Bayes training hot path.
 *
 * The reference (debbiemarkslab/BEAR) is pure Python on TensorFlow; it has no FFI.  The
 * boundary below is what a reference maintainer binds through ctypes (INTEGRATION.md
 * shows the stub) to replace, per batch, the TensorFlow graph built by
 *   bear_model/bear_net.py:146-197  (_train_step)       -> bear_dm_prior_f64
 *   bear_model/bear_ref.py:207-259  (_train_step)       -> bear_dm_ref_f64
 *   bear_model/core.py:73-74, 138-139 (counts_log_prob) -> both (train_ar selects)
 *   bear_model/dataloader.py:35-46  (TSV -> tensors)    -> bear_parse_counts_tsv
 *
 * Conventions
 *   - every entry point returns an int status: BEAR_OK (0) or a negative bear_status;
 *     bear_strerror() names it.  Nothing throws across the boundary.
 *   - the CALLER owns every buffer.  Pointers marked [dev] are device pointers valid on
 *     the workspace's device (e.g. torch.Tensor.data_ptr()), 16-byte aligned, row-major.
 *     The library owns only the bear_ws handle.
 *   - launches are asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream).  Outputs are valid after the stream is synchronised.
 *   - re-entrant across distinct workspaces / streams; one workspace must not be used
 *     by two streams at once.
 *   - the calling thread's current HIP device must be the workspace's device.
 *   - count rows are 5 wide: A, C, G, T (or U) and the stop symbol, in the order of
 *     bear_model/core.py:146-147; counts are uint32 (KMC's counter limit, summarize.py:66-67).  The *_wide entry points take
 *     the row width as an argument: 21 for the protein alphabet (20 letters + stop, core.py:142-145), or 5.
 *   - there is NO CPU fallback: without a gfx950 device the compute entry points fail
 *     with BEAR_ERR_NO_DEVICE.
 */
#ifndef BEAR_HIP_H
#define BEAR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BEAR_ABI_VERSION 12 /* 7: + bear_dm_prior_wide_f64, bear_eval_wide_f64, bear_parse_counts_tsv[_shard]_wide (rows of 21: protein);
                              8: + bear_logdir_sample_wide_f64;
                              9: + bear_kmer_sort_create_wide, bear_fastx_size_wide, bear_fastx_encode_wide, bear_write_counts_tsv_wide,
                                 bear_encode_kmers_i8 mode 2 (protein count tables from sequence files);
                              10: + bear_linear_forward_wide_f64, bear_linear_backward_wide_f64 (the linear AR function as rows of 21);
                              11: + bear_cnn_param_count_wide, bear_cnn_forward_wide_f64, bear_cnn_backward_wide_f64 (the convolutional AR
                                  function as rows of 21);
                              12: + bear_dm_ref_wide_f64, bear_ref_train_reduce_wide_f64, bear_ref_train_step_wide_f64,
                                  bear_dm_refmix_wide_grad_f64 (bear_ref's training step on rows of 21);
                                  still 12 (symbols added, nothing changed): + bear_dm_linear_wide_f64,
                                  bear_net_linear_train_reduce_wide_f64, bear_net_linear_train_step_wide_f64 (bear_net's step with the
                                  linear AR function on rows of 21 as one launch);
                                  + bear_kmer_sort_bytes, bear_kmer_bin_hist, bear_kmer_sort_create_range (counting in passes over
                                  key ranges);
                                  + bear_dm_cnn_wide_f64, bear_net_cnn_train_reduce_wide_f64, bear_net_cnn_train_step_wide_f64
                                  (bear_net's step with the convolutional AR function on rows of 21 as two launches);
                                  + bear_score_transitions_u64, bear_kmer_find_u64, bear_score_sum_f64 (variant and sequence
                                  scoring on the device);
                                  + bear_shuffle_rows_range, bear_shuffle_gather_host (a range of
                                  the shuffled rows: streamed and multi-rank shuffled epochs);
                                  + bear_math_probe_f64 (the device math routines one at a time: tests and diagnostics);
                                  + bear_ref_prior_rows_f64, bear_generate_whole_ref_f64 (bear_ref models downstream: scoring and
                                  generation under a reference-mixed prior);
                                  + bear_score_moments_f64 (the exact posterior mean and variance of scores; the probe
                                  operations BEAR_PROBE_PSI, BEAR_PROBE_PSI1) */
#define BEAR_ROW_WIDTH 5 /* alphabet_size + 1 for dna/rna */

typedef enum bear_status {
  BEAR_OK = 0,
  BEAR_ERR_INVALID_ARG = -1, /* null / misaligned pointer, bad flag */
  BEAR_ERR_NO_DEVICE = -2,   /* no usable HIP device */
  BEAR_ERR_WRONG_DEVICE = -3,/* current device != workspace device */
  BEAR_ERR_HIP = -4,         /* a HIP runtime call failed; see bear_last_hip_error() */
  BEAR_ERR_NOMEM = -5,
  BEAR_ERR_IO = -6,          /* file could not be opened / read */
  BEAR_ERR_PARSE = -7        /* malformed count-table row */
} bear_status;

typedef struct bear_ws bear_ws; /* opaque workspace: per-block partial sums + launch geometry */

int bear_abi_version(void);
const char *bear_strerror(int status);
/* hipError_t of the most recent failing HIP call on this thread (0 if none). */
int bear_last_hip_error(void);

/* Allocates the workspace on `device` (makes no change to the caller's current device).
 * A workspace serves ONE stream at a time: the block partials and the arrival counter of the kernels whose last block
 * forms the final sums are per-launch state, so launches that may overlap (two streams, two host threads) each take
 * their own workspace; launches ordered on one stream share one freely.  After a launch or synchronisation FAILED, destroy
 * the workspace and create a new one before replaying a captured graph that uses it: an arrival counter left half way by the
 * failed launch is discarded by later EAGER launches only (their stamps are newer), not by replays of an older capture. */
int bear_ws_create(int device, bear_ws **out);
int bear_ws_destroy(bear_ws *ws);

/*
 * bear_net._train_step arithmetic for one batch / shard, unscaled
 * (bear_model/bear_net.py:146-197; alpha = prior / exp(h_signed) + eps, bear_net.py:43;
 *  AR mode probs = prior + eps, bear_net.py:68).
 *   counts  [dev] uint32 [n_rows, 5]   transition counts of the training column
 *   prior   [dev] double [n_rows, 5]   ar_func(kmers) rows
 *   out     [dev] double [2]           out[0] = sum_i LL_i ; out[1] = d out[0] / d h_signed
 *                                      (0 in AR mode, bear_net.py:194-196)
 *   grad_prior [dev, nullable] double [n_rows, 5]  dLL_i / d prior_ib
 * The caller applies the -(num_kmers / batch) scale of bear_net.py:190-191.
 */
int bear_dm_prior_f64(bear_ws *ws, const uint32_t *counts, const double *prior, uint64_t n_rows,
                      double h_signed, double eps, int train_ar, double *out, double *grad_prior,
                      void *stream);

/*
 * bear_ref._train_step arithmetic with the stop net-function (bear_model/bear_ref.py:207-259,
 * prior from bear_ref.py:30-33, 63-68, reference column preprocessed as bear_ref.py:332-337,
 * net function bear_model/ar_funcs.py:121-126), unscaled.
 *   train, ref [dev] uint32 [n_rows, 5]
 *   out        [dev] double [4] = { sum LL, d/d h_signed, d/d tau_signed, d/d net_weight_signed }
 */
int bear_dm_ref_f64(bear_ws *ws, const uint32_t *train, const uint32_t *ref, uint64_t n_rows,
                    double h_signed, double tau_signed, double nu_signed, double eps, int train_ar,
                    double *out, void *stream);

/*
 * Planned variants: the per-step hot path for a count table that stays resident in HBM across
 * optimizer steps (the reference re-reads one cached table every epoch, bear_model/dataloader.py:47-48).
 * A plan holds what depends on the counts only -- per 512-context tile the (context, column) work
 * items sorted by count, as uint16 offsets, plus global lists of the rare large-count items -- so
 * the per-step kernels do no sorting.  Results are identical to the unplanned entry points.
 *   The plan is a lossless sorted sparse encoding of the counts: the planned step kernels read it INSTEAD of the
 *   count rows (the `counts` / `train` arguments of the planned entries only identify the table).
 *   bear_plan_create: synchronous; `ncol` = 5 for bear_dm_prior_plan_f64 (all columns are items),
 *     4 for bear_dm_ref_plan_f64 (the stop column has a context-independent concentration).
 *     The plan is valid for exactly the buffer contents it was built from; rebuild after any change.
 *   bear_plan_bytes: device bytes held by the plan (= extra HBM traffic per step).
 * The library owns the plan's device memory; bear_plan_destroy releases it.
 */
typedef struct bear_plan bear_plan;
int bear_plan_create(bear_ws *ws, const uint32_t *counts, uint64_t n_rows, int ncol, bear_plan **out);
/* The same for a caller that only runs the mode-N entry points (bear_dm_prior_plan_f64 / _grad_f64 / _dev_f64: any torch AR
 * function) on the plan: where more than half of the table's cells are beyond the sorted encoding's product path (counts of
 * 1e3 ... 1e5 -- a k-mer table at small k, bear_model/data/ysd1_lag_5_file_0_preshuf.tsv) the plan comes back in its DENSE form,
 * *rowwise = 1: it keeps nothing per item (a few KB of histograms), and the step streams the caller's count rows and prior rows,
 * a context per thread, every cell through the table-log form of the Stirling difference -- the sorted form of such a table is
 * ~100 B per context of overflow lists whose gathers bound the step (2e7 dense contexts: 1.30 -> 0.9 ms, with gradient rows 2.76 ->
 * 1.18 ms).  Same results to rounding.  Every other entry point that takes a plan (the fused linear / convolutional steps,
 * bear_plan_pair_contexts, ...) returns BEAR_ERR_INVALID_ARG for a dense-form plan: they walk the sorted encoding. */
int bear_plan_create_auto(bear_ws *ws, const uint32_t *counts, uint64_t n_rows, int *rowwise, bear_plan **out);
int bear_plan_destroy(bear_plan *plan);
uint64_t bear_plan_bytes(const bear_plan *plan);
/* Diagnostics: the tiles of a plan -- first context, number of contexts, number of product-path items (1 <= count <= 24) and
 * byte offset of the tile's block in the plan stream; [host] arrays of `count` entries for tiles [first, first + count). */
uint64_t bear_plan_tile_count(const bear_plan *plan);
int bear_plan_tile_info(const bear_plan *plan, uint64_t first, uint64_t count, uint64_t *row0, uint32_t *rows, uint32_t *items,
                        uint64_t *stream_offset);
/* A plan for bear_dm_ref_plan_f64 / bear_ref_train_*_f64 that also knows the REFERENCE column `ref` [dev] uint32 [n_rows, 5]
 * -- as constant as the training column while a table is resident.  Contexts without reference counts (most k-mers of a read
 * set that the reference genome does not contain) share one concentration per letter, so all their items collapse into a
 * 24-bin histogram over the count, built here once; the step then streams only the items of contexts that do have reference
 * counts, as 16-byte records {count, r_b, sum r} sorted by count.  Results are those of the streaming path (same arithmetic
 * per item; the fp64 sums in another order).  The planned entries must be called with the same `train` and `ref` buffers.
 * A table of LARGE counts (more than half of its cells beyond the sorted encoding's product path: bear_plan_create_auto's test; the
 * reference's ysd1 table) gets the plan's dense form here too: nothing kept per item, the planned mode-R entries and
 * bear_ref_train_*_f64 stream the training and reference rows, a context per thread (2e7 such contexts: 1.41 -> ~0.9 ms, 153 -> 0.002 B
 * of plan per context).  Nothing changes for the caller. */
int bear_plan_create_ref(bear_ws *ws, const uint32_t *train, const uint32_t *ref, uint64_t n_rows, bear_plan **out);
/* prior_normalized != 0: the caller asserts that every row of `prior` sums to one -- true for each
 * ar_func of the reference, all of which end in a softmax (bear_model/ar_funcs.py:44,97,121-126).
 * The concentration total A = 1/h + 5 eps is then shared by all contexts and the context terms
 * come from the plan's histogram of totals; with 0 the kernel sums each row and uses the shared A
 * only where the sum is 1 to 2 ulp. */
int bear_dm_prior_plan_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const double *prior,
                           uint64_t n_rows, double h_signed, double eps, int train_ar, int prior_normalized,
                           double *out, void *stream);
/* The same with the gradient rows: grad_prior [dev] double [n_rows, 5] = d sum LL / d prior (BEAR mode), what
 * grad_tape.gradient hands back to ar_func (bear_model/bear_net.py:193).  With prior_normalized != 0 the rows are turned into
 * their gradient in place in LDS (double-buffered tiles: 84 B per context at the streaming rate); as everywhere, prior rows
 * are non-negative (a concentration f / h + eps must be positive). */
int bear_dm_prior_plan_grad_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const double *prior,
                                uint64_t n_rows, double h_signed, double eps, int train_ar, int prior_normalized,
                                double *out, double *grad_prior, void *stream);
int bear_dm_ref_plan_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *train, const uint32_t *ref,
                         uint64_t n_rows, double h_signed, double tau_signed, double nu_signed, double eps,
                         int train_ar, double *out, void *stream);

/* The same with h_signed read from device memory ([dev] double [1], e.g. a parameter tensor the optimizer updates in place): the
 * step is enqueued without the host reading the parameter back (one sync fewer per step; needed for steps that are followed
 * by an all-reduce on the same stream).  grad_prior [dev, nullable]: NULL = no gradient rows (parameter-free ar_func). */
int bear_dm_prior_plan_dev_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const double *prior, uint64_t n_rows,
                               const double *h_signed_dev, double eps, int train_ar, int prior_normalized, double *out,
                               double *grad_prior, void *stream);

/*
 * One optimizer step with every moving quantity in device memory, in two halves:
 *
 *   bear_*_train_reduce_f64  this rank's shard, ONE launch for bear_ref and the linear head (every block derives the kernel
 *                            constants from theta in its prologue, the last block to finish sums the per-block partials in a
 *                            fixed order; the cnn step adds its forward / backward launches) into
 *                            packed [dev] double [1 + n_theta] = { sum LL, d sum LL / d theta[0..n_theta) }  (unscaled)
 *   bear_train_apply_f64     tf.keras Adam (beta 0.9 / 0.999, epsilon 1e-7; bear_ref.py:312-313, 346-350) on theta with the
 *                            gradients scale * packed[1..]; loss_buf[step] = -scale * packed[0] (the "elbo" the reference logs);
 *                            one single-block launch (update, step counter, loss record)
 *
 * Nothing synchronises with the host.  One rank enqueues them back to back (bear_*_train_step_f64 below: capturable in a
 * HIP graph and replayed -- the reference traces its step once with tf.function, bear_model/bear_ref.py:207; the bundled
 * example is 10 000 steps over 1365 contexts, launch-bound).  With the rows sharded over several ranks the caller puts ONE
 * all-reduce(sum) of `packed` between the halves -- what strategy.reduce (bear_net.py:290) and the cross-replica gradient sum
 * inside optimizer.apply_gradients (bear_net.py:278-282) do -- still without a host round trip.
 *
 *   theta    [dev] double [n_theta], updated in place by apply:
 *            bear_ref / stop net function: {h_signed, tau_signed, net_weight_signed}           (n_theta = 3)
 *            bear_net / linear:            {h_signed, mat[lag,5,5]}                            (n_theta = 1 + 25 lag)
 *            bear_net / cnn:               {h_signed, params[bear_cnn_param_count(...)]}       (n_theta = 1 + param count)
 *   adam_m, adam_v [dev] double [n_theta], adam_t [dev] double [1]: optimizer state, zero before the first step
 *   scale    the loss scale -(num_kmers / global batch) (bear_ref.py:252-253); 1 when packed already holds scaled sums
 *            (gradient accumulation: the caller adds scale_k * packed_k over acc_steps batches, bear_net.py:193-196)
 *   train_ar != 0: theta[0] = h_signed gets no gradient (bear_net.py:194-196)
 *   loss_buf [dev, nullable] double [loss_cap], indexed by the step counter adam_t
 *   the cnn step borrows per-context buffers prior_buf [n,5], t1_buf [n,16], grad_rows_buf [n,5]; call bear_cnn_reserve once
 *   before capturing (it sizes the library's block-partial buffer; nothing allocates inside a step).  The step evaluates the
 *   AR function only for the contexts that hold training counts (the plan's lists: nothing else enters the ELBO or a gradient);
 *   the other rows of prior_buf / t1_buf are left as they were -- hand over initialised (e.g. zeroed) buffers.
 */
/*
 * Optional, once per batch, after bear_plan_create (and after the k-mer order, if any): prefix levels for the convolutional step.
 * In a k-mer-sorted batch the window of position p (letters [p, p + filter_width)) is the same for all contexts that share their
 * first p + filter_width letters, and those are neighbours; with levels attached, bear_net_cnn_train_reduce_f64 / _step_f64
 * called with this plan, this kmer_code pointer, lag and filter_width evaluate a position once per DISTINCT prefix, forward and
 * backward (one launch per level; the sums are the same up to rounding) -- about 1.3 instead of 6 positions per context on a
 * dense sorted table of 13-mers; sparser tables keep the prefix lengths that pay (e.g. from lag - 2 letters down).  The levels are tied to the buffer kmer_code (bear_pack_kmers_u64 form; identity and contents,
 * like the plan's count slab).  *n_levels (nullable) = 0: nothing was attached (rows in another order, a table too sparse for its
 * prefixes to repeat, a plan whose lists skip rows, a shape outside the fused kernels): the step runs as before.
 * Holds about 45 bytes per context on a dense table.  Synchronises `stream` (set-up path).
 * A plan with levels attached carries PER-LAUNCH state (the levels' layer-1 / dT1 rows are written by every forward and backward
 * pass over them, also through a `const bear_plan *`): like a workspace it serves one stream at a time.
 */
int bear_plan_attach_cnn_levels(bear_plan *plan, const uint64_t *kmer_code, int lag, int filter_width, int *n_levels, void *stream);
/* Rows and prefix lengths (letters) of the attached levels 1 .. n (rows_out [host, nullable when capacity = 0], letters_out [host,
 * nullable]); returns their number.  A prefix length whose prefixes hardly repeat is skipped: the level below evaluates its position too. */
int bear_plan_cnn_level_rows(const bear_plan *plan, uint64_t *rows_out, int *letters_out, int capacity);
/* bear_plan_attach_cnn_levels also attaches WINDOW TABLES to every level (level 0 = the contexts) for the positions the level's rows
 * would evaluate themselves, from the last one up: what a position adds to a row's layer-1 sums depends on its filter_width-letter
 * window alone, and a batch holds at most 6^filter_width distinct windows (65 536 for eight letters of ACGT) however many rows a
 * level has.  Forward: the position is evaluated once per distinct window, a row gathers its window's row; backward: a window's dT1
 * row is the sum of its rows' dT1 rows (listed by window at attach time: fixed order, no atomics), then the position's backward pass
 * over the windows.  A table is attached while the level holds >= 8 rows per distinct window (at most 6 per level); 8 bytes per row
 * and table.  Distinct windows, positions and levels of the attached tables (nullable outputs); returns their number. */
int bear_plan_cnn_window_rows(const bear_plan *plan, uint64_t *rows_out, int *pos_out, int *level_out, int capacity);
/* bear_cnn_forward_f64 over the plan's prefix levels when they were attached for this kmer_code pointer, lag and filter width
 * (the plain forward otherwise); t1_save is required. */
int bear_cnn_forward_plan_f64(bear_ws *ws, const bear_plan *plan, const uint64_t *kmer_code, uint64_t n_rows, int lag, int filter_width,
                              int num_filters, int layer1_width, const double *params, double *prior, double *t1_save, void *stream);
int bear_train_apply_f64(double *theta, int n_theta, const double *packed, double *adam_m, double *adam_v, double *adam_t,
                         double learning_rate, double scale, int train_ar, double *loss_buf, uint64_t loss_cap, void *stream);
int bear_ref_train_reduce_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *train, const uint32_t *ref, uint64_t n_rows,
                              const double *theta, double eps, int train_ar, double *packed, void *stream);
int bear_net_linear_train_reduce_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const uint64_t *kmer_index, int lag,
                                     uint64_t n_rows, const double *theta, double eps, int train_ar, double *packed, void *stream);
int bear_cnn_reserve(bear_ws *ws, uint64_t n_rows, int lag, int filter_width, int num_filters, int layer1_width);
int bear_net_cnn_train_reduce_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const uint64_t *kmer_code, uint64_t n_rows,
                                  int lag, int filter_width, int num_filters, int layer1_width, const double *theta, double *prior_buf,
                                  double *t1_buf, double *grad_rows_buf, double eps, int train_ar, double *packed, void *stream);
/* reduce + apply in one call (single rank); `out` / `packed` as above.  bear_ref_train_step_f64 and
 * bear_net_linear_train_step_f64 are ONE launch since round 6: the last block of the reduce kernel -- every other block has
 * arrived, i.e. is done reading theta -- runs the update of bear_train_apply_f64 behind its fixed-order sums (same source, same
 * bits as the two-launch form; BEAR_AMD_TWO_LAUNCH_STEP=1 in the environment of the call restores reduce + apply).  The
 * convolutional step stays forward / DM / backward launches + apply. */
int bear_ref_train_step_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *train, const uint32_t *ref, uint64_t n_rows,
                            double *theta, double *adam_m, double *adam_v, double *adam_t, double eps, int train_ar,
                            double learning_rate, double scale, double *out, double *loss_buf, uint64_t loss_cap, void *stream);
int bear_net_linear_train_step_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const uint64_t *kmer_index, int lag,
                                   uint64_t n_rows, double *theta, double *adam_m, double *adam_v, double *adam_t, double *packed,
                                   double eps, int train_ar, double learning_rate, double scale, double *loss_buf,
                                   uint64_t loss_cap, void *stream);
int bear_net_cnn_train_step_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const uint64_t *kmer_code, uint64_t n_rows,
                                int lag, int filter_width, int num_filters, int layer1_width, double *theta, double *adam_m,
                                double *adam_v, double *adam_t, double *prior_buf, double *t1_buf, double *grad_rows_buf,
                                double *packed, double eps, int train_ar, double learning_rate, double scale, double *loss_buf,
                                uint64_t loss_cap, void *stream);

/*
 * The whole bear_net training step for the linear AR function, fused on a plan: replaces
 * ar_func = make_ar_func_linear(...) (bear_model/ar_funcs.py:23-46), _train_step's forward and
 * grad_tape.gradient(loss, [h_signed, mat]) (bear_model/bear_net.py:146-197).
 *   kmer_code [dev] uint64 [n_rows]   packed contexts, letter l in bits [3l, 3l+3): 0..3 letters, 4 = start
 *                                     symbol '[', 5 = any other character (all-zero one-hot row, core.py:173);
 *                                     positions >= lag hold 5.  bear_pack_kmers_u64 builds it from the int8
 *                                     code matrix [n_rows, lag] (values outside 0..4 -> 5).  lag <= 21.
 *   kmer_index [dev] uint64 [n_rows]  what the linear-head entry points read: the same contexts as row numbers of the
 *                                     kernel's letter-group tables (pairs of letters in 6-bit fields, the last three
 *                                     letters in an 8-bit field behind them), built ONCE per batch from kmer_code by
 *                                     bear_linear_index_u64 (the contexts of a batch do not change between steps).
 *                                     16-byte aligned.  Fastest when the rows of the batch are sorted by k-mer (first
 *                                     letter most significant; the sums do not depend on the order): consecutive
 *                                     contexts then share their leading groups and the backward pass adds once per wave.
 *   mat       [dev] double [lag,5,5]  the AR parameter
 *   out       [dev] double [2]        { sum LL, d sum LL / d h_signed }
 *   grad_mat  [dev] double [lag,5,5]  d sum LL / d mat (overwritten)
 * Reads 8 bytes per context plus the plan; writes nothing per context.
 */
int bear_pack_kmers_u64(const int8_t *codes, uint64_t n_rows, int lag, uint64_t *packed, void *stream);
int bear_linear_index_u64(const uint64_t *kmer_code, uint64_t n_rows, int lag, uint64_t *kmer_index, void *stream);
/* ASCII k-mer bytes as parsed from the count file [dev] uint8 [n_rows, lag] -> int8 letter codes [dev] [n_rows, lag]:
 * 0..3 = A, C, G, T (U when rna == 1), 4 = '[', -1 = anything else (the all-zero one-hot row of core.py:173).
 * rna == 2 selects the protein alphabet instead: ARNDCEQGHILKMFPSTWYV -> 0..19, 20 = '[', -1 = anything else. */
int bear_encode_kmers_i8(const uint8_t *ascii, uint64_t n_rows, int lag, int rna, int8_t *codes, void *stream);
int bear_dm_linear_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const uint64_t *kmer_index,
                       const double *mat, int lag, uint64_t n_rows, double h_signed, double eps, int train_ar,
                       double *out, double *grad_mat, void *stream);
/*
 * Optional, once per batch, after bear_plan_create and bear_linear_index_u64 (and after the k-mer order below, if any): pairs
 * contexts of the plan's lists that share all letters but the last three, so that the fused step reads their shared table rows
 * once and reduces their gradients together, and orders the pairs of such a run so that the 16 lanes of a pass of an LDS atomic
 * meet on as few bank pairs as the run allows (copies of one k-mer share a lane and one add) -- about 15 % off a step on a
 * k-mer-sorted table; the sums are the same.  ~0.03 s per 1e8 contexts (3 ms for a batch of 5e6).  The pairing is tied to the buffer kmer_index (identity and contents: it must not change afterwards, like the
 * plan's count slab) and to lag: bear_dm_linear_f64 / bear_net_linear_train_*_f64 called with that pointer and lag take the
 * paired form, any other call the plain one.  A tile whose paired list would not fit the kernel's row threads (a stretch of
 * the table where neighbours share nothing) keeps its plain list; *paired (nullable) = 0 when that is true of more than half
 * of the tiles (a sparse table): the plan is then left as it was.  Synchronises `stream` (set-up path).
 */
int bear_plan_pair_contexts(bear_plan *plan, const uint64_t *kmer_index, int lag, int *paired, void *stream);
/* BEAR_AMD_DETERMINISTIC=1 (environment, read per call): parameter gradients that are bit-identical from run to run.
 *   bear_dm_linear_f64 / bear_net_linear_train_*: the gradient tables of the fused linear step hold 64-bit fixed-point integers
 *     scaled by 2^62 / bound, where bound >= the sum of |gradient| over everything that is added into one gradient -- derived from
 *     the table's counts (sum, non-zero cells, maximum) and the launch's h (kernels_linear.h, lin_fx_bound):
 *     d/d mat is then the exact integer sum of the contexts' rounded gradients -- independent of the order of the adds, of the
 *     cut into tiles and blocks and of the form of the plan's lists (a step that takes two launches -- paired tiles, then the
 *     tiles that kept their plain lists -- keeps the first launch's integers in the workspace's accumulator: round 6) -- turned into
 *     a double once at the end of the STEP.  Each context's gradient is rounded to bound * 2^-62 (instead of to its own last bit).
 *     Across ranks every rank converts its own integer sum before the all-reduce adds the doubles: bit-reproducible for a given
 *     number of ranks and cut of the batch, equal to rounding (<= 1e-15 of the largest entry) between different ones.
 *   bear_cnn_backward_f64 / bear_net_cnn_train_*: the backward kernel runs ONE wave per block (the block's gradient image takes its
 *     adds in program order); reproducible from run to run for a given launch geometry, at an eighth of the waves per CU.
 * The scalar sums (sum LL, d/dh, d/dtau, d/dnet_weight) are fixed-order sums in every mode.
 * bear_plan_count_total: total[3] / bound[3] [host, nullable] = {sum of all counts, cells that hold a count, largest count} of the
 *   plan's table / the values in force for the scale (default: the table's own).
 * bear_plan_set_count_bound: bound[3] >= the plan's own, each < 2^50 -- the same three of EVERYTHING that is added into one gradient
 *   with this plan's rows (ranks that share a batch: sums of the first two, maximum of the third, over the ranks). */
int bear_plan_count_total(const bear_plan *plan, double *total, double *bound);
/* 1 for libbear_hip_det.so (built with -DBEAR_DET_BUILD): everything above is always on AND the work units of a tile are dealt to
 * the waves statically instead of drawn, so that every sum of a launch -- sum LL and d/dh too -- is bit-identical from run to run
 * (in the regular library those are fixed-order across blocks, but which thread adds which item inside a block follows the draw). */
int bear_deterministic_build(void);
int bear_plan_set_count_bound(bear_plan *plan, const double *bound);
/* How the pairing went: tiles that take the paired form / tiles that keep their plain list (outputs nullable); returns 1 when the
 * plan is paired, 0 when it is not. */
int bear_plan_pair_info(const bear_plan *plan, uint64_t *paired_tiles, uint64_t *plain_tiles);

/*
 * The linear AR function as prior ROWS, forward and backward: replaces make_ar_func_linear's ar_func (bear_model/ar_funcs.py:41-45)
 * and grad_tape.gradient through it wherever the rows themselves are needed -- evaluation / h_scan (bear_model/bear_net.py:
 * 387-531), bear_ref with the linear net function (the rows are mixed with the reference prior, bear_model/bear_ref.py:63-68),
 * get_var_probs.  (bear_net's training step never forms them: bear_dm_linear_f64 above.)
 *   kmer_code  [dev] uint64 [n_rows]    packed contexts (bear_pack_kmers_u64); lag <= 21
 *   mat        [dev] double [lag,5,5]   the AR parameter
 *   forward:   prior [dev] double [n_rows,5] = softmax(sum_l mat[l, kmer[l], :]), 16-byte aligned; unknown letters add nothing
 *   backward:  grad_prior [dev] double [n_rows,5] = d L / d prior; prior = the forward rows;
 *              grad_mat [dev] double [lag,5,5] = d L / d mat (overwritten; LDS fp64 atomics: reproducible to rounding)
 * Row order: any; fastest in k-mer order (consecutive contexts share their leading letters and the backward pass adds once
 * per wave for them).  Asynchronous on `stream`; one launch each.
 */
int bear_linear_forward_f64(bear_ws *ws, const uint64_t *kmer_code, uint64_t n_rows, int lag, const double *mat, double *prior,
                            void *stream);
int bear_linear_backward_f64(bear_ws *ws, const uint64_t *kmer_code, uint64_t n_rows, int lag, const double *prior,
                             const double *grad_prior, double *grad_mat, void *stream);

/*
 * The same at the protein alphabet's row width (20 letters + stop): make_ar_func_linear(lag, 20)'s ar_func and its gradient.
 *   codes      [dev] int8 [n_rows,lag]   context letters, 16-byte aligned: 0..19 residues, 20 = '[', anything else (-1) an unknown
 *                                        letter = an all-zero one-hot row (bear_encode_kmers_i8 mode 2); there is no packed form
 *   width      21 (anything else: BEAR_ERR_INVALID_ARG); lag 1 .. LINEAR_WIDE_MAX_LAG (mat lives in LDS; else BEAR_ERR_INVALID_ARG)
 *   mat        [dev] double [lag,21,21]  the AR parameter
 *   forward:   prior [dev] double [n_rows,21] = softmax(sum_l mat[l, codes[l], :]) (max-shifted), 16-byte aligned
 *   backward:  prior = the forward rows, grad_prior [dev] double [n_rows,21] = d L / d prior (both 16-byte aligned);
 *              grad_mat [dev] double [lag,21,21] = d L / d mat, overwritten (n_rows == 0: zeros).  An fp64 matrix product per block,
 *              block partials summed in a fixed order: NO floating-point atomics -- the same inputs give the same bits from run to
 *              run for a given device (grid: min(n_rows / 128, 2 x CUs) blocks), identically in both builds of the library.
 * Row order: any.  Asynchronous on `stream`, nothing is read back to the host (both can be captured into a HIP graph); one launch each.
 */
#define LINEAR_WIDE_MAX_LAG 16
int bear_linear_forward_wide_f64(bear_ws *ws, const int8_t *codes, uint64_t n_rows, int lag, int width, const double *mat,
                                 double *prior, void *stream);
int bear_linear_backward_wide_f64(bear_ws *ws, const int8_t *codes, uint64_t n_rows, int lag, int width, const double *prior,
                                  const double *grad_prior, double *grad_mat, void *stream);

/*
 * bear_net's training step with the linear AR function at the protein alphabet's width as ONE launch (kernels_linear_wide.h): what
 * bear_linear_forward_wide_f64, bear_dm_prior_wide_f64 with gradient rows and bear_linear_backward_wide_f64 compute in three, without a
 * row ever reaching memory.  No plan, any row order.
 *   counts     [dev] uint32 [n_rows,21]  16-byte aligned;  codes [dev] int8 [n_rows,lag], 16-byte aligned (as above)
 *   width      21, lag 1 .. LINEAR_WIDE_MAX_LAG (anything else: BEAR_ERR_INVALID_ARG, nothing is launched)
 * bear_dm_linear_wide_f64: the primitive, constants by value (bear_dm_linear_f64 without a plan):
 *   mat [dev] double [lag,21,21];  out [dev] double [2] = {sum LL, d sum LL / d h_signed (0 with train_ar)};
 *   grad_mat [dev] double [lag,21,21] = d sum LL / d mat, overwritten.
 * bear_net_linear_train_reduce_wide_f64 / bear_net_linear_train_step_wide_f64: bear_net_linear_train_reduce_f64 /
 *   bear_net_linear_train_step_f64 at this width: theta [dev] double [1 + 441 lag] = {h_signed, mat...}, read on the device;
 *   packed [dev] double [2 + 441 lag] = {sum LL, d/dh, d/d mat...}.  The step form runs the tf.keras Adam update of theta (adam_m,
 *   adam_v [1 + 441 lag], adam_t [1]) and the loss record (bear_train_apply_f64's arguments) in the block that sums the partials:
 *   the same bits as reduce followed by bear_train_apply_f64, which is what BEAR_AMD_TWO_LAUNCH_STEP=1 makes of it.
 * n_rows == 0: zeros (the step form still updates and records).  No floating-point atomics: block partials are summed in a fixed
 * order, the same inputs give the same bits from run to run for a given device (grid: min(n_rows / 128, 2 x CUs) blocks), identically
 * in both builds of the library.  Asynchronous on `stream`, nothing is read back to the host: all three can be captured into a HIP graph.
 */
int bear_dm_linear_wide_f64(bear_ws *ws, const uint32_t *counts, const int8_t *codes, uint64_t n_rows, int lag, int width,
                            const double *mat, double h_signed, double eps, int train_ar, double *out, double *grad_mat, void *stream);
int bear_net_linear_train_reduce_wide_f64(bear_ws *ws, const uint32_t *counts, const int8_t *codes, uint64_t n_rows, int lag, int width,
                                          const double *theta, double eps, int train_ar, double *packed, void *stream);
int bear_net_linear_train_step_wide_f64(bear_ws *ws, const uint32_t *counts, const int8_t *codes, uint64_t n_rows, int lag, int width,
                                        double *theta, double *adam_m, double *adam_v, double *adam_t, double eps, int train_ar,
                                        double learning_rate, double scale, double *packed, double *loss_buf, uint64_t loss_cap,
                                        void *stream);

/*
 * bear_ref's prior rows for a net function with parameters (linear, cnn): replaces the arithmetic of _make_ref_ar_func's ar_func
 * (bear_model/bear_ref.py:63-68 with _counts_to_probs, :9-33) and grad_tape.gradient through it.  (With the stop net function
 * the mixing lives inside bear_dm_ref_*_f64 and no rows exist.)
 *   Every [n_rows,5] array is 16-byte aligned.
 *   net_rows  [dev] double [n_rows,5]  the net function's rows g (bear_linear_forward_f64, bear_cnn_forward_f64, ...)
 *   ref_rows  [dev] double [n_rows,5]  the reference column as the driver passes it: (counts + eps) with the stop column
 *                                      zeroed (bear_model/bear_ref.py:332-337)
 *   tau_signed, net_weight_signed [dev] double [1]  the two parameters, read on the device (the optimizer's tensors)
 *   forward:  prior [dev] double [n_rows,5] = (nw g + jukes_cantor(ref, tau)) / (nw + 1), 16-byte aligned
 *   backward: grad_prior [dev] double [n_rows,5] = d L / d prior;  grad_net_rows [dev] double [n_rows,5] = d L / d g (16-byte
 *             aligned);  grad_scalars [dev] double [2] = { d L / d tau_signed, d L / d net_weight_signed }
 * Asynchronous on `stream`; one launch each.  4-letter alphabets.
 */
int bear_ref_mix_forward_f64(bear_ws *ws, const double *net_rows, const double *ref_rows, uint64_t n_rows, const double *tau_signed,
                             const double *net_weight_signed, double *prior, void *stream);
int bear_ref_mix_backward_f64(bear_ws *ws, const double *net_rows, const double *ref_rows, const double *grad_prior, uint64_t n_rows,
                              const double *tau_signed, const double *net_weight_signed, double *grad_net_rows, double *grad_scalars,
                              void *stream);

/*
 * bear_ref's training step for a net function with parameters, the reference mixing INSIDE the DM step: replaces _train_step of
 * bear_model/bear_ref.py:207-259 from the net function's rows onwards -- the mixing of bear_ref.py:63-68 (as
 * bear_ref_mix_forward_f64), sum LL and its gradients (as bear_dm_prior_plan_grad_f64 with prior_normalized), and the way back
 * through the mixing (as bear_ref_mix_backward_f64) -- in one launch: 127 B per context instead of three launches and 367 B.
 *   plan       five-column plan of the training counts (bear_plan_create(ws, counts, n_rows, 5, ...))
 *   net_rows   [dev] double [n_rows,5]  the net function's rows g: non-negative, every row sums to one (softmax output)
 *   ref_rows   [dev] double [n_rows,5]  (reference counts + eps) with the stop column zeroed (bear_model/bear_ref.py:332-337)
 *   h_signed_dev, tau_signed_dev, net_weight_signed_dev  [dev] double [1] each (the optimizer's tensors)
 *   train_ar   != 0: the multinomial of bear_model/core.py:138-139 on the mixed rows (no h: out[1] = 0)
 *   out        [dev] double [4] = { sum LL, d/d h_signed, d/d tau_signed, d/d net_weight_signed }  (unscaled)
 *   grad_net_rows [dev] double [n_rows,5] = d sum LL / d g: what the net function's backward pass takes
 * Row arrays 16-byte aligned.
 */
int bear_dm_refmix_plan_grad_f64(bear_ws *ws, const bear_plan *plan, const uint32_t *counts, const double *net_rows,
                                 const double *ref_rows, uint64_t n_rows, const double *h_signed_dev, const double *tau_signed_dev,
                                 const double *net_weight_signed_dev, double eps, int train_ar, double *out, double *grad_net_rows,
                                 void *stream);

/*
 * The convolutional AR function of bear_net, forward and backward (replaces make_ar_func_cnn's ar_func,
 * bear_model/ar_funcs.py:49-99, and grad_tape.gradient through it, bear_model/bear_net.py:193) for 4-letter alphabets,
 * num_filters = 30 and kmer_layer1_width = 16 (every reference config), lag <= 21, filter_width <= lag.
 *   kmer_code [dev] uint64 [n_rows]      packed contexts (bear_pack_kmers_u64)
 *   params    [dev] double [bear_cnn_param_count(...)]  the parameters flattened and concatenated in the reference's
 *             order (ar_funcs.py:98-99): filters [fw,5,nf], intercept0 [P,nf], weights1 [P,nf,l1], intercept1 [l1],
 *             weights2 [l1,5], intercept2 [5], scale0 [P,nf], scale1 [l1];  P = lag - fw + 1
 *   forward:  prior [dev] double [n_rows,5] = ar_func rows; t1_save [dev, nullable] double [n_rows,16] = the layer-1
 *             pre-normalisation sums, which the backward entry takes instead of redoing the first tensordot
 *   backward: grad_prior [dev] double [n_rows,5] = d L / d prior (e.g. from bear_dm_prior_plan_grad_f64);
 *             grad_params [dev] double [param_count] = d L / d params (overwritten), same layout as params.
 *   Row order: any (the sums do not depend on it).  Both kernels are fastest when the rows are sorted by k-mer (first letter
 *   most significant, as bear_net.train uploads a batch): consecutive contexts then share their leading letters, a window that
 *   a whole wave (forward: 64 contexts) / tile (backward: 32) shares is evaluated once per distinct window, and the backward
 *   pass of such a position needs only the column sums of the tile's d t1 rows (it is linear in them) -- 18 / 52 ms instead
 *   of 33 / 104 ms per 1e8 contexts at lag 13, filter width 8.
 */
int bear_cnn_param_count(int lag, int filter_width, int num_filters, int layer1_width);
int bear_cnn_forward_f64(bear_ws *ws, const uint64_t *kmer_code, uint64_t n_rows, int lag, int filter_width, int num_filters,
                         int layer1_width, const double *params, double *prior, double *t1_save, void *stream);
int bear_cnn_backward_f64(bear_ws *ws, const uint64_t *kmer_code, uint64_t n_rows, int lag, int filter_width, int num_filters,
                          int layer1_width, const double *params, const double *t1_save, const double *prior,
                          const double *grad_prior, double *grad_params, void *stream);

/*
 * The same at the protein alphabet's row width (20 letters + stop): make_ar_func_cnn(lag, 20)'s ar_func and its gradient, as a plain
 * pair of row kernels (protein batches are not k-mer sorted and share no windows: no plan, no prefix levels).
 *   codes      [dev] int8 [n_rows,lag]   context letters, 16-byte aligned: 0..19 residues, 20 = '[', anything else (-1) an unknown
 *                                        letter = an all-zero one-hot row; there is no packed form
 *   width 21, num_filters 30, layer1_width 16, 1 <= filter_width <= lag <= CNN_WIDE_MAX_LAG; anything else: BEAR_ERR_INVALID_ARG
 *              (bear_cnn_param_count_wide returns the same code).  CNN_WIDE_MAX_LAG: the backward kernel keeps the filter image of
 *              filter_width taps (5208 B each, rows of 30 at a stride of 31) and the weights of the positions (4320 B each) next
 *              to the staged rows of a tile of 64 contexts (72 KiB) in a CU's 160 KiB of LDS -- 158 KiB at filter_width = lag =
 *              16, 17 taps do not fit -- and the positions are the 16 rows of one matrix tile.
 *   params     [dev] double [bear_cnn_param_count_wide(...)]  the reference's order: filters [fw,21,nf], intercept0 [P,nf],
 *              weights1 [P,nf,l1], intercept1 [l1], weights2 [l1,21], intercept2 [21], scale0 [P,nf], scale1 [l1];  P = lag - fw + 1
 *   forward:   prior [dev] double [n_rows,21] = ar_func rows; t1_save [dev, nullable] double [n_rows,16] = the layer-1
 *              pre-normalisation sums for the backward entry (both 16-byte aligned)
 *   backward:  prior, t1_save = what the forward entry wrote; grad_prior [dev] double [n_rows,21] = d L / d prior (16-byte aligned);
 *              grad_params [dev] double [param_count] = d L / d params, overwritten (n_rows == 0: zeros, nothing is launched).
 *              Every sum over contexts is an fp64 matrix product per block; block partials are summed in a fixed order: NO
 *              floating-point atomics -- the same inputs give the same bits from run to run for a given device (grid:
 *              min(ceil(n_rows / 64), CUs) blocks, at least one), identically in both builds of the library.  A tile of 64 contexts whose grad_prior
 *              rows are all zero is skipped.
 * Row order: any.  Asynchronous on `stream`, no allocation, nothing is read back to the host (both can be captured into a HIP
 * graph); one launch each.
 */
#define CNN_WIDE_MAX_LAG 16
int bear_cnn_param_count_wide(int lag, int filter_width, int num_filters, int layer1_width, int width);
int bear_cnn_forward_wide_f64(bear_ws *ws, const int8_t *codes, uint64_t n_rows, int lag, int filter_width, int num_filters,
                              int layer1_width, int width, const double *params, double *prior, double *t1_save, void *stream);
int bear_cnn_backward_wide_f64(bear_ws *ws, const int8_t *codes, uint64_t n_rows, int lag, int filter_width, int num_filters,
                               int layer1_width, int width, const double *params, const double *t1_save, const double *prior,
                               const double *grad_prior, double *grad_params, void *stream);

/*
 * bear_net's training step with the convolutional AR function at the protein alphabet's width as TWO launches (kernels_cnn_wide.h):
 * what bear_cnn_forward_wide_f64, bear_dm_prior_wide_f64 with gradient rows and bear_cnn_backward_wide_f64 compute in three, without
 * a prior row or a gradient row reaching memory.  The first launch runs the forward pass, the DM step on the count rows and the way
 * back through the softmax, a context per lane, and leaves the layer-1 sums and dz = d sum LL / d logits; the second is the backward
 * kernel on those rows.  A context whose counts are all zero forms no row and no item (its dz row is exact zeros).  No plan, any row order.
 *   counts     [dev] uint32 [n_rows,21]  16-byte aligned;  codes [dev] int8 [n_rows,lag], 16-byte aligned (as above)
 *   lag, filter_width, num_filters, layer1_width, width: as bear_cnn_forward_wide_f64 (anything else: BEAR_ERR_INVALID_ARG, nothing is
 *              launched; so is a NULL or misaligned pointer)
 *   dz_buf     [dev] double [n_rows,21], t1_buf [dev] double [n_rows,16]: scratch lent by the caller, 16-byte aligned, overwritten
 *              (may be NULL when n_rows == 0)
 * bear_dm_cnn_wide_f64: the primitive, constants by value:
 *   params [dev] double [bear_cnn_param_count_wide(...)];  out [dev] double [2] = {sum LL, d sum LL / d h_signed (0 with train_ar)};
 *   grad_params [dev] double [param count] = d sum LL / d params, overwritten.
 * bear_net_cnn_train_reduce_wide_f64 / bear_net_cnn_train_step_wide_f64: theta [dev] double [1 + param count] = {h_signed, params...},
 *   read on the device;  packed [dev] double [2 + param count] = {sum LL, d/dh, d/d params...}.  The step form runs the tf.keras Adam
 *   update of theta (adam_m, adam_v [1 + param count], adam_t [1]) and the loss record (bear_train_apply_f64's arguments) in the block
 *   of the second launch that sums the gradient's partials: the same bits as reduce followed by bear_train_apply_f64, which is what
 *   BEAR_AMD_TWO_LAUNCH_STEP=1 makes of it (three launches).
 * n_rows == 0: zeros (the step form still updates and records).  No floating-point atomics: block partials are summed in a fixed
 * order, the same inputs give the same bits from run to run for a given device (grids: min(ceil(n_rows / 256), CUs) and
 * min(ceil(n_rows / 64), CUs) blocks), identically in both builds of the library.  Asynchronous on `stream`, no allocation, nothing is
 * read back to the host: all three can be captured into a HIP graph.
 */
int bear_dm_cnn_wide_f64(bear_ws *ws, const uint32_t *counts, const int8_t *codes, uint64_t n_rows, int lag, int filter_width,
                         int num_filters, int layer1_width, int width, const double *params, double h_signed, double eps, int train_ar,
                         double *dz_buf, double *t1_buf, double *out, double *grad_params, void *stream);
int bear_net_cnn_train_reduce_wide_f64(bear_ws *ws, const uint32_t *counts, const int8_t *codes, uint64_t n_rows, int lag,
                                       int filter_width, int num_filters, int layer1_width, int width, const double *theta,
                                       double *dz_buf, double *t1_buf, double eps, int train_ar, double *packed, void *stream);
int bear_net_cnn_train_step_wide_f64(bear_ws *ws, const uint32_t *counts, const int8_t *codes, uint64_t n_rows, int lag, int filter_width,
                                     int num_filters, int layer1_width, int width, double *theta, double *adam_m, double *adam_v,
                                     double *adam_t, double *dz_buf, double *t1_buf, double eps, int train_ar, double learning_rate,
                                     double scale, double *packed, double *loss_buf, uint64_t loss_cap, void *stream);

/*
 * Held-out evaluation, one pass over a row range: replaces _evaluation_step of bear_model/bear_net.py:323-371
 * (and its bear_ref twin, bear_ref.py:391-446, with prior = the reference-mixed AR rows) and, with n_h > 1,
 * one batch of h_scan (bear_net.py:465-531).
 *   test   [dev] uint32 [n_rows,5]  held-out transition counts
 *   train  [dev] uint32 [n_rows,5]  or NULL (use_train = False)
 *   prior  [dev] double [n_rows,5]  ar_func rows (NULL only when n_h == 0 and with_ar == 0)
 *   h      [host] n_h > 0 values (not log-transformed); van_reg [host] n_van pseudo-counts; n_h + n_van <= 64
 *   out    [dev] double [2 (n_h + n_van) + 3] =
 *          { ll_ear[n_h], ll_arm, ll_van[n_van], correct_ear[n_h], correct_arm, correct_van[n_van], total_len }
 * The arg-max noise of core.py:69-71,134-136 is a counter-based hash of (noise_seed, model, row_base + row,
 * letter) -- the same sequence for any sharding of the rows -- restated in oracle/bear_oracle.py:eval_noise.
 */
int bear_eval_f64(bear_ws *ws, const uint32_t *test, const uint32_t *train, const double *prior, uint64_t n_rows,
                  const double *h, int n_h, int with_ar, const double *van_reg, int n_van, double eps,
                  uint64_t noise_seed, uint64_t row_base, double *out, void *stream);

/*
 * Rows of any supported width W (`width`: 21 for the protein alphabet, 5 for checking against the entry points above; anything
 * else is BEAR_ERR_INVALID_ARG).  DNA / RNA training and evaluation keep their 5-wide kernels and plans; these are the path of
 * a 21-letter table (kernels_wide.h: row tiles staged through LDS, one item per NON-ZERO cell, the row term once per context).
 *
 * bear_dm_prior_wide_f64: what bear_dm_prior_f64 computes, at width W, in ONE launch with nothing on the host in between:
 *   counts [dev] uint32 [n_rows, W], prior [dev] double [n_rows, W], grad_prior [dev] double [n_rows, W] or NULL -- 16-byte aligned
 *   h_signed_dev [dev] double [1], 8-byte aligned: read by the kernel (capturable into a HIP graph; may be NULL when train_ar)
 *   out [dev] double [2], 8-byte aligned: { sum LL, d sum LL / d h_signed } written by the last block in a fixed order (the
 *   same bits for the same inputs and n_rows).  BEAR mode alpha = prior / exp(h_signed) + eps; train_ar: probs = prior + eps,
 *   d/dh = 0, gradient rows c / probs.
 * bear_eval_wide_f64: bear_eval_f64 at width W -- same arguments, limits (n_h + n_van <= 64), alignment and output vector; the
 *   tie-breaking noise is the same counter-based stream with the cell key row * W + letter (oracle/bear_oracle.py:eval_noise with
 *   width = W), so at W = 5 every accuracy equals bear_eval_f64's.
 */
int bear_dm_prior_wide_f64(bear_ws *ws, const uint32_t *counts, const double *prior, uint64_t n_rows, int width,
                           const double *h_signed_dev, double eps, int train_ar, double *out, double *grad_prior, void *stream);
int bear_eval_wide_f64(bear_ws *ws, const uint32_t *test, const uint32_t *train, const double *prior, uint64_t n_rows, int width,
                       const double *h, int n_h, int with_ar, const double *van_reg, int n_van, double eps,
                       uint64_t noise_seed, uint64_t row_base, double *out, void *stream);

/*
 * bear_ref._train_step at width W (kernels_refmix_wide.h): the reference mixing of bear_ref.py:63-68 inside the DM step, from the
 * uint32 rows of the training and the reference column (no fp64 reference rows, no prior rows).  `width` as above; every row
 * pointer 16-byte aligned, out / packed / theta / the Adam state and the parameter pointers 8-byte aligned; n_rows = 0 writes zero
 * sums.  One launch each; the sums are written by the last block in a fixed order (the same bits for the same inputs and n_rows).
 *
 * bear_dm_ref_wide_f64: bear_dm_ref_f64 at width W -- the stop net function, parameters by value;
 *   out [dev] double [4] = { sum LL, d/d h_signed, d/d tau_signed, d/d net_weight_signed }.
 * bear_ref_train_reduce_wide_f64 / bear_ref_train_step_wide_f64: bear_ref_train_reduce_f64 / bear_ref_train_step_f64 without a plan:
 *   the constants from the device-resident theta [3] = { h_signed, tau_signed, net_weight_signed }; the step runs tf.keras Adam
 *   behind the sums in the same launch (BEAR_AMD_TWO_LAUNCH_STEP=1: reduce, then bear_train_apply_f64), capturable into a HIP graph.
 * bear_dm_refmix_wide_grad_f64: bear_dm_refmix_plan_grad_f64 at width W without a plan -- a net function with parameters:
 *   net_rows [dev] double [n_rows, W] its rows g (non-negative; NOT assumed normalised), ref [dev] uint32 [n_rows, W] the reference
 *   COUNTS (the kernel adds eps and drops the stop column itself), the three parameters read from device memory;
 *   out [4] as above, grad_net_rows [dev] double [n_rows, W] = d out[0] / d net_rows (rows of contexts without training counts are
 *   exact zeros).
 */
int bear_dm_ref_wide_f64(bear_ws *ws, const uint32_t *train, const uint32_t *ref, uint64_t n_rows, int width, double h_signed,
                         double tau_signed, double nu_signed, double eps, int train_ar, double *out, void *stream);
int bear_ref_train_reduce_wide_f64(bear_ws *ws, const uint32_t *train, const uint32_t *ref, uint64_t n_rows, int width,
                                   const double *theta, double eps, int train_ar, double *packed, void *stream);
int bear_ref_train_step_wide_f64(bear_ws *ws, const uint32_t *train, const uint32_t *ref, uint64_t n_rows, int width, double *theta,
                                 double *adam_m, double *adam_v, double *adam_t, double eps, int train_ar, double learning_rate,
                                 double scale, double *out, double *loss_buf, uint64_t loss_cap, void *stream);
int bear_dm_refmix_wide_grad_f64(bear_ws *ws, const uint32_t *counts, const double *net_rows, const uint32_t *ref, uint64_t n_rows,
                                 int width, const double *h_signed_dev, const double *tau_signed_dev, const double *net_weight_signed_dev,
                                 double eps, int train_ar, double *out, double *grad_net_rows, void *stream);

/*
 * The same on a sorted plan of the TEST column, for a table that stays resident (a held-out evaluation after training, the
 * train-set evaluation, every value of an h_scan): bear_eval_plan_create lists, per tile of 448 contexts, the cells and the rows
 * with a non-zero test count sorted by count, the rows whose largest TRAINING counts tie (their vanilla arg-max is decided
 * by the noise: which letters tie, most first) and the rows beyond the vanilla models' histogram bins (training + test total >=
 * 2048), and counts once what the vanilla models need of the table as a whole (histograms of the integer arguments of their
 * lgamma differences, the test counts under a unique largest training count, the total length) -- asynchronous on `stream`,
 * ~16 B of plan per context.  `train` [dev, nullable] is the conditioning column the
 * evaluations will use (NULL: none); bear_eval_plan_f64 must be given the same test / train buffers.  It streams the row slabs
 * and the plan through a three-slot LDS ring and evaluates wave-uniform units of equal counts without a workgroup barrier --
 * rows without test transitions cost nothing.  Arguments, output vector and noise stream are those of bear_eval_f64
 * (identical results up to the order of the fp64 sums; accuracies exactly).  The plan is valid for exactly the buffer contents
 * it was built from.  With vanilla models the plan's tie lists stand for the arg-max of count + van_reg + eps + noise only while
 * the noise cannot bridge a whole count: BEAR_ERR_INVALID_ARG unless 1750 eps < 0.5 and 0 <= van_reg <= 2^30 (bear_eval_f64
 * takes any values).
 *   row_ids [dev, nullable] uint32 [n_rows], 16-byte aligned: the buffers hold a COMPACTED batch -- only the contexts with
 *           held-out counts (nothing else enters any of the sums) -- and row i is row `row_base + row_ids[i]` of the table: the
 *           key of its tie-breaking noise, so the accuracies of a compacted batch equal those of the whole batch exactly.
 *           NULL: row i is row `row_base + i`.
 */
typedef struct bear_eval_plan bear_eval_plan;
int bear_eval_plan_create(bear_ws *ws, const uint32_t *test, const uint32_t *train, uint64_t n_rows, bear_eval_plan **out, void *stream);
int bear_eval_plan_destroy(bear_eval_plan *plan);
uint64_t bear_eval_plan_bytes(const bear_eval_plan *plan);
int bear_eval_plan_f64(bear_ws *ws, const bear_eval_plan *plan, const uint32_t *test, const uint32_t *train, const double *prior,
                       uint64_t n_rows, const double *h, int n_h, int with_ar, const double *van_reg, int n_van, double eps,
                       uint64_t noise_seed, uint64_t row_base, const uint32_t *row_ids, double *out, void *stream);

/*
 * BMM marginal likelihood of one dataset column: replaces _marginal_step of bear_model/dataloader.py:111-118,
 *   out[k] = sum_i lbeta(counts_i + alpha_k) - lbeta(alpha_k 1_5),   alpha [host] n_alpha <= 64, out [dev].
 */
int bear_bmm_f64(bear_ws *ws, const uint32_t *counts, uint64_t n_rows, const double *alpha, int n_alpha, double *out,
                 void *stream);

/*
 * bear_two_sample_f64: hypothesis tests on two count columns a, b of one table (kernels_twosample.h), one pass over its rows.
 * Per context k and model, with concentrations alpha_j > 0 and A = alpha_0 + ... + alpha_(W-1) added in that order,
 *   T(c) = lgamma(A) - lgamma(A + n) + sum_j [lgamma(alpha_j + c_j) - lgamma(alpha_j)],   n = sum_j c_j
 * -- the log marginal of the transitions as SEQUENCES (no multinomial coefficient, as bear_score_marg_f64: the coefficient of a
 * pooled row is not the product of the two).  Models in bear_score_marg_f64's order: n_h BEAR models alpha_j = prior[k, j] *
 * (1.0 / h_m), then n_van vanilla models alpha_j = van.
 *   a, b   [dev] uint32 [n_rows, W], prior [dev, nullable] double [n_rows, W]: 16-byte aligned; `width` W: 5 or 21.  A prior entry
 *          under a non-zero count must be > 0.
 *   h [host] n_h values, van [host] n_van values, each > 0 and finite: read before the entry returns;
 *          1 <= n_h + n_van <= BEAR_TWO_SAMPLE_MAX_MODELS.
 *   out    [dev] double [n_h + n_van, 4] = { M_a, M_b, M_ab, B }: M_a = sum_k T(a_k), M_b = sum_k T(b_k), M_ab = sum_k T(a_k + b_k),
 *          B = sum_k B_k with B_k = (T(a_k) + T(b_k)) - T(a_k + b_k) formed PER ROW: the log Bayes factor of "two distributions"
 *          over "one" (positive favours different).  A row with n_a = 0 or n_b = 0 has B_k = 0.0 exactly (no lgamma is evaluated
 *          for it; its T still enters M_a or M_b, and M_ab with the same bits); pooled counts are exact beyond 2^32.
 *   out_ar [dev, nullable] double [2] = { L_a, L_b }, L_a = sum_k sum_{j: a_j > 0} a_j log(prior[k, j]): the AR model's
 *          log-likelihood of each sample; M_a[m] - L_a is the goodness-of-fit log Bayes factor of BEAR(h_m) over its AR model.
 *   row_terms [dev, nullable] double [n_rows, n_h + n_van] = B_k.  out, out_ar, row_terms: 8-byte aligned.
 * Asynchronous on `stream`, allocates nothing; at most four models a launch, sixteen in four; per-thread -> wave -> block partial
 * -> fixed-order sum, no atomics: equal inputs give equal bits (for a given n_rows) in both libraries.  n_rows = 0 writes zeros.
 * BEAR_ERR_INVALID_ARG, before any device call: a width other than 5 or 21, n_h > 0 or out_ar without prior (of a table with rows:
 * as a, b, it may be NULL when n_rows = 0), an h or van that is
 * not > 0 and finite, n_h + n_van of 0 or beyond the maximum, a missing or misaligned pointer.
 * The stream is deliberately NOT the last parameter: tests/test_stream_contract_gpu.py keeps a row for every declaration that ends
 * in `void *stream`, and this entry came after that table.  The contract is not waived: tests/test_two_sample_gpu.py holds the
 * entry to it with the same harness (tests/stream_util.py).
 */
#define BEAR_TWO_SAMPLE_MAX_MODELS 16
int bear_two_sample_f64(bear_ws *ws, const uint32_t *a, const uint32_t *b, const double *prior, uint64_t n_rows, int width,
                        const double *h, int n_h, const double *van, int n_van, void *stream,
                        double *out, double *out_ar, double *row_terms);

/*
 * bear_k_sample_f64: bear_two_sample_f64 among G = n_groups columns of one table at once (kernels_ksample.h) -- which samples differ
 * from which, and are all of them one distribution -- in ONE pass: every column is read once and T(c_g) evaluated once, where a loop
 * of G (G - 1) / 2 two-sample calls does both G - 1 times.  T, the order and meaning of the models, prior, h, van and the widths
 * are exactly bear_two_sample_f64's.
 *   counts, col_rows: row k of column g is at counts + (col_rows[g] + k) * W; col_rows [host] n_groups values, read before the
 *          entry returns; every column start 16-byte aligned.  A [num_ds, N, W] device table and any subset or order of its
 *          columns is used in place (col_rows[g] = column * N).  2 <= n_groups <= BEAR_K_SAMPLE_MAX_GROUPS.
 *   With M = n_h + n_van and the P = G (G - 1) / 2 pairs in the order (0, 1), (0, 2), ..., (G - 2, G - 1):
 *   out_group [dev] double [M, G]    = sum_k T(c_g)
 *   out_pair  [dev] double [M, P, 2] = { sum_k T(c_g + c_g'), sum_k B_k }, B_k = (T(c_g) + T(c_g')) - T(c_g + c_g') formed PER ROW
 *   out_all   [dev] double [M, 2]    = { sum_k T(sum_g c_g), sum_k [(sum_g T(c_g)) - T(sum_g c_g)] }, the bracket formed per row and
 *          the T(c_g) added in group order: the log Bayes factor of "G distributions" over "one"
 *   out_ar    [dev, nullable] double [G] = sum_k sum_j c_gj log(prior[k, j])
 *   row_terms [dev, nullable] double [n_rows, M] = the per-row bracket of out_all[:, 1]: which contexts drive the difference
 *   scratch   [dev] double [n_scratch], n_scratch >= bear_k_sample_scratch(ws, n_rows, width, n_groups): the block partials (the
 *          workspace's evaluation partials are too small for up to 258 sums a model); the query needs no device and no workspace
 *          (ws may be NULL there) and is 0 for a width or n_groups the entry refuses.
 * Exact zeros: a pair whose row has an empty side adds exactly +0.0 to B, the row's pooled T is the other side's T (no item is
 * evaluated again); a row with at most one non-empty group adds exactly +0.0 to out_all[:, 1] and has row_terms +0.0; a row with no
 * transition costs its bytes only.  Pooled counts are exact integers (a pair's cell below 2^33, all sixteen below 2^36, a row total
 * below 2^41).
 * Asynchronous on `stream`, allocates nothing; no floating-point atomics: equal inputs give equal bits for a given n_rows and
 * n_groups, in both libraries -- NOT the bits of bear_two_sample_f64 on a pair, nor the same bits under a permutation of the columns
 * (other reduction orders).  At most four models a launch; more are further launches, each with the bits of a call of its own.
 * n_rows = 0 writes zeros.  Out of scope: more than 16 groups a call, sharded tables.
 * BEAR_ERR_INVALID_ARG, before any device call: everything bear_two_sample_f64 refuses, n_groups out of range, a missing col_rows,
 * n_scratch below the query, a missing scratch, out_group, out_pair or out_all, a misaligned column (16 bytes) or output (8).
 * The stream is deliberately NOT the last parameter, as for bear_two_sample_f64; tests/test_k_sample_gpu.py holds the entry to the
 * contract with the harness of tests/stream_util.py.
 */
#define BEAR_K_SAMPLE_MAX_GROUPS 16
uint64_t bear_k_sample_scratch(bear_ws *ws, uint64_t n_rows, int width, int n_groups);
int bear_k_sample_f64(bear_ws *ws, const uint32_t *counts, const uint64_t *col_rows, int n_groups, const double *prior,
                      uint64_t n_rows, int width, const double *h, int n_h, const double *van, int n_van, void *stream,
                      double *scratch, uint64_t n_scratch, double *out_group, double *out_pair, double *out_all,
                      double *out_ar, double *row_terms);

/*
 * The primitive underneath both entry points, item by item (tests / diagnostics): for x > 0 and
 * integer c >= 0,  D[i] = lgamma(x+c) - lgamma(x)  and  P[i] = digamma(x+c) - digamma(x)
 * -- the two quantities TFP's lbeta and its autodiff yield in bear_model/core.py:73-74.
 *   path 0: the code path the fused kernels choose (product + table log for c <= 31, shifted
 *           Stirling series above);  path 1 / 2: the general routine for every item, on the library
 *           log / on the table log (the form the planned kernels use for large counts).
 *   x, D, P [dev] double [n];  c [dev] uint32 [n]
 */
int bear_dm_items_f64(bear_ws *ws, const double *x, const uint32_t *c, uint64_t n, int path, double *D,
                      double *P, void *stream);

/*
 * The device math routines underneath every kernel, one routine per launch and element by element (tests / diagnostics, as
 * bear_dm_items_f64; no production path calls it).  The kernel calls the routine the production kernels call, on tables staged
 * as they stage them (the workspace's log table into LDS, the exp table by exp2(k / 128) on the device).
 *   a, out0 [dev] double [n];  b, out1 [dev] double [n], read and written by the item routines only (NULL elsewhere)
 *   out0[i] = routine(a[i]):
 *     RCP 1/a;  LOG_TAB[_V] the table log, a > 0 finite (_V: the form with its leading coefficient in vector registers; the same
 *     bits);  LOG1P_SMALL[_V] log(1 + a), |a| <= 2^-8;  LOG1P_POS log(1 + a), a >= 0;  EXP_TAB / CNN_EXP_NEG exp(a), a <= 0 (0 /
 *     exp(-700) below -700);  LIN_EXP_UNITS 2^(a / 128);  STIR_LG / STIR_PSI the Stirling tails of lgamma / digamma at y = 1 / a;
 *     WAVE_SUM / WAVE_MAX the sum / the largest (of non-negative values) of each whole wave of 64 elements, in every lane of it
 *     (elements past n count as 0);  PSI / PSI1 digamma / trigamma of a, a > 0 finite and normal (bear_psi, bear_psi1: the routines of
 *     bear_score_moments_f64)
 *   item routines, x = a[i] and the count c = b[i], an exact integer >= 1 as a double (row totals pass 2^32):
 *     out0[i] = lgamma(x + c) - lgamma(x), out1[i] = digamma(x + c) - digamma(x) by
 *     SRT_GENERAL[_FAST|_AUTO] the sorted / planned family's general routine on the library log, on the table log (NaN outside
 *     0 < x < 2^1000), and the kernels' choice between the two;  ROW_ITEM_TAB / ROW_ITEM the rows family's item with / without
 *     the log table.  x <= 0 or NaN gives NaN from SRT_GENERAL, SRT_GENERAL_FAST and SRT_GENERAL_AUTO.
 */
#define BEAR_PROBE_RCP 0
#define BEAR_PROBE_LOG_TAB 1
#define BEAR_PROBE_LOG_TAB_V 2
#define BEAR_PROBE_LOG1P_SMALL 3
#define BEAR_PROBE_LOG1P_SMALL_V 4
#define BEAR_PROBE_LOG1P_POS 5
#define BEAR_PROBE_EXP_TAB 6
#define BEAR_PROBE_CNN_EXP_NEG 7
#define BEAR_PROBE_LIN_EXP_UNITS 8
#define BEAR_PROBE_STIR_LG 9
#define BEAR_PROBE_STIR_PSI 10
#define BEAR_PROBE_WAVE_SUM 11
#define BEAR_PROBE_WAVE_MAX 12
#define BEAR_PROBE_SRT_GENERAL 13
#define BEAR_PROBE_SRT_GENERAL_FAST 14
#define BEAR_PROBE_SRT_GENERAL_AUTO 15
#define BEAR_PROBE_ROW_ITEM_TAB 16
#define BEAR_PROBE_ROW_ITEM 17
#define BEAR_PROBE_PSI 18
#define BEAR_PROBE_PSI1 19
#define BEAR_PROBE_N_OPS 20
int bear_math_probe_f64(bear_ws *ws, int op, const double *a, const double *b, uint64_t n, double *out0, double *out1,
                        void *stream);

/*
 * Posterior sampling of transition probabilities (inference apps).
 *
 * bear_log_gamma_f64 replaces log_gamma.log_gamma(concs, size) (bear_model/log_gamma.py:17-76):
 *   conc [dev] double [n] > 0;  out [dev] double [n_samples, n],  out[s, i] ~ log Gamma(conc[i], 1)
 *   -- accurate for tiny concentrations, where exp(out) underflows.  The reference draws from numpy's global
 *   generator; here a draw is a pure function of (seed, s, i), restated in oracle/bear_oracle.py:log_gamma_hash.
 *
 * bear_logdir_sample_f64 replaces the concentration assembly + sampling (or MAP) of get_var_probs.get_pdf
 * (bear_model/get_var_probs.py:128-183), output='numpy' layout:
 *   counts [dev, nullable] uint32 [n_rows,5]  training-column counts (NULL = unseen k-mers, all zero, :441-444)
 *   prior  [dev, nullable] double [n_rows,5]  ar_func rows (required when n_h > 0 or with_ar)
 *   h [host] n_h values; van [host] n_van values; n_h + n_van <= 64
 *   model order: (AR if with_ar) , BEAR h_0.., vanilla van_0..   (get_var_probs.py:146-153)
 *   map != 0: log(conc / sum conc), mc_samples forced to 1; with_ar requires map
 *   out [dev] double [n_rows, 5, n_models, mc_samples]  normalised log transition probabilities
 *   a draw is a pure function of (seed, model, sample, row_base + row, letter): any sharding of the rows
 *   reproduces the same table.
 *
 * bear_logdir_sample_wide_f64: bear_logdir_sample_f64 for rows of `width` letters (21: the protein alphabet; 5 gives
 *   bear_logdir_sample_f64's output bit for bit) -- the same arguments, limits and model order; counts, prior [n_rows, width],
 *   out [n_rows, width, n_models, mc_samples]; the draw of a cell is keyed by (seed, model, sample, (row_base + row) * width +
 *   letter).  Any other width is BEAR_ERR_INVALID_ARG.
 */
int bear_log_gamma_f64(const double *conc, uint64_t n, uint64_t n_samples, uint64_t seed, double *out, void *stream);
int bear_logdir_sample_f64(const uint32_t *counts, const double *prior, uint64_t n_rows, const double *h, int n_h,
                           int with_ar, const double *van, int n_van, int mc_samples, int map, uint64_t seed,
                           uint64_t row_base, double *out, void *stream);
int bear_logdir_sample_wide_f64(const uint32_t *counts, const double *prior, uint64_t n_rows, int width, const double *h,
                                int n_h, int with_ar, const double *van, int n_van, int mc_samples, int map, uint64_t seed,
                                uint64_t row_base, double *out, void *stream);

/*
 * Synthetic "k=13 sparse" count table for measurement: rows
 * [row0, row0 + n_rows) of a table defined by a counter-based hash of (seed, row), so any
 * shard of the same table can be generated independently on any GPU.
 *   train, test, ref [dev, each nullable] uint32 [n_rows, 5]
 *   dense != 0 selects the large-count stress distribution (ysd1-like, counts 1e3..3e5).
 */
int bear_synth_counts_u32(uint64_t seed, uint64_t row0, uint64_t n_rows, int dense, uint32_t *train,
                          uint32_t *test, uint32_t *ref, void *stream);
/* Read-only pass over n_bytes of device memory (16-byte lane loads, nothing written): the measured HBM read ceiling that
 * bench.py reports next to the 8 TB/s spec peak. */
int bear_stream_read(bear_ws *ws, const void *src, uint64_t n_bytes, void *stream);
/* prior [dev] double [n_rows, 5]: positive rows summing to 1 (softmax of hashed logits). */
int bear_synth_prior_f64(uint64_t seed, uint64_t row0, uint64_t n_rows, double *prior, void *stream);

/*
 * Host-side reader of the summarize.py count-table format (bear_model/summarize.py:429-449;
 * replaces the CsvDataset + tfio decode_json path of bear_model/dataloader.py:35-46).
 * Row: kmer '\t' '[[' c,c,c,c,c '],[' ... ']]' '\n' with num_ds groups of 5.
 *   bear_count_rows: number of non-empty lines.
 *   bear_count_newlines: `wc -l` of the file (newline bytes) -- the reference's num_kmers (models/train_bear_net.py:52-55).
 *   bear_parse_counts_tsv: fills, for rows [0, max_rows):
 *     kmers  [host] char  [max_rows, lag]      (no terminator; '[' padded as in the file)
 *     counts [host] uint32 [num_ds, max_rows, 5] (planar by dataset column)
 *   *n_rows_out receives the number of rows parsed.
 * Host threads: the counters, the dense readers and bear_write_counts_tsv[_wide] work on one chunk of the text (of the selected
 * rows) per thread -- the hardware threads, or BEAR_PARSE_THREADS [environment] of them, at most 64; one thread for a text below
 * 1 MiB, and for the writer at least 64 Ki rows per thread.  No result depends on the thread count.  BEAR_ERR_NOMEM: a thread or a
 * host buffer could not be had (the threads already started have ended when the call returns).
 */
int bear_count_rows(const char *path, uint64_t *n_rows_out);
int bear_count_newlines(const char *path, uint64_t *n_out);
/* The sparse row format of dataloader.sparse_dataloader (bear_model/dataloader.py:52-109): `kmer; [[ds, col], ...]; [value, ...]`,
 * one line per k-mer behind `skip_lines` header lines.  counts [host] uint32 [num_ds, max_rows, width] (zeroed here, then filled). */
int bear_parse_sparse_counts(const char *path, int num_ds, int width, int lag, uint64_t skip_lines, uint64_t max_rows,
                             char *kmers, uint32_t *counts, uint64_t *n_rows_out);
int bear_parse_counts_tsv(const char *path, int num_ds, int lag, uint64_t max_rows, char *kmers,
                          uint32_t *counts, uint64_t *n_rows_out);
/*
 * One rank's rows of a row-sharded table (replaces strategy.experimental_distribute_dataset,
 * bear_model/bear_net.py:273): the table of total_rows rows (this file holds global rows [row_base, row_base + file rows)) is
 * cut into batches of batch_rows rows (last one short, dataloader.py:37) and every batch into `world` contiguous pieces,
 * base = m / world rows each, the first m % world pieces one row longer; rank `rank` decodes only the lines of its pieces, in
 * file order, into kmers [host] char [max_rows, lag] and counts [host] uint32 [num_ds, max_rows, 5]; the other lines are
 * stepped over.  skip_lines header lines are ignored first (dataloader.py:7 `header`; world = 1 makes this the plain reader with
 * a header).  bear_shard_rows_count gives the number of local rows (the size to allocate) from the row counts alone.
 */
int bear_shard_rows_count(uint64_t row_base, uint64_t file_rows, uint64_t total_rows, uint64_t batch_rows, int rank, int world,
                          uint64_t *n_local_out);
int bear_parse_counts_tsv_shard(const char *path, int num_ds, int lag, uint64_t skip_lines, uint64_t row_base, uint64_t total_rows,
                                uint64_t batch_rows, int rank, int world, uint64_t max_rows, char *kmers, uint32_t *counts,
                                uint64_t *n_local_out, uint64_t *n_file_rows_out);
/* bear_parse_counts_tsv and bear_parse_counts_tsv_shard for rows of `width` counts per dataset column (21: the protein alphabet;
 * 5: the readers above): counts [host] uint32 [num_ds, max_rows, width].  Any other width: BEAR_ERR_INVALID_ARG. */
int bear_parse_counts_tsv_wide(const char *path, int num_ds, int width, int lag, uint64_t max_rows, char *kmers, uint32_t *counts,
                               uint64_t *n_rows_out);
int bear_parse_counts_tsv_shard_wide(const char *path, int num_ds, int width, int lag, uint64_t skip_lines, uint64_t row_base,
                                     uint64_t total_rows, uint64_t batch_rows, int rank, int world, uint64_t max_rows, char *kmers,
                                     uint32_t *counts, uint64_t *n_local_out, uint64_t *n_file_rows_out);

/*
 * Binary cache of a parsed count table: what bear_parse_counts_tsv produced, stored as it is uploaded,
 * so later runs / other ranks skip the text decode (the reference re-decodes per process and caches in RAM only,
 * bear_model/dataloader.py:47-48).  File: 64-byte header {"BEARCT01", n_rows, lag, num_ds, size and mtime of the
 * source text, offsets}, k-mer bytes [n_rows, lag], uint32 counts [num_ds, n_rows, 5].
 *   bear_stat_source: size / mtime (ns) of a text file, the staleness key stored in the header.
 *   bear_cache_write: atomic (temporary file + rename).
 *   bear_cache_read:  rows [row0, row0 + n_rows) into kmers [host, nullable] char [n_rows, lag] and
 *                     counts [host] uint32 [num_ds, n_rows, 5] -- a rank reads only its shard.
 */
int bear_stat_source(const char *path, uint64_t *size_out, int64_t *mtime_ns_out);
int bear_cache_write(const char *path, const char *kmers, const uint32_t *counts, uint64_t n_rows, int lag, int num_ds,
                     uint64_t src_size, int64_t src_mtime_ns);
int bear_cache_info(const char *path, uint64_t *n_rows, int *lag, int *num_ds, uint64_t *src_size, int64_t *src_mtime_ns);
int bear_cache_read(const char *path, uint64_t row0, uint64_t n_rows, char *kmers, uint32_t *counts);

/*
 * On-device shuffle of resident rows (replaces the `shuf` step the reference asks for before training,
 * docs/usage.rst:191-200): dst[i] = src[perm(i)], perm a keyed bijection of [0, n_rows) (4-round Feistel network with
 * cycle walking; bear_shuffle_source_row evaluates it on the host, oracle/bear_oracle.py:shuffle_perm restates it).
 *   src, dst [dev] n_rows rows of row_bytes bytes (20: a count slab; 8: packed k-mers; lag: k-mer bytes); dst != src.
 * Calling it with the same seed on every column of a table keeps the columns aligned.
 *
 * A range of the shuffled rows, for an epoch whose whole columns do not go through the device (a streamed epoch, a rank's pieces):
 * batch [a, b) of the shuffled table is rows perm(a) .. perm(b - 1) of the table in file order.
 *   bear_shuffle_rows_range: dst[j] = src[perm(first + j)] for j < n_out, perm as above (bear_shuffle_rows is first = 0, n_out =
 *     n_rows).  src [dev] n_rows rows; dst [dev] n_out rows, dst != src.  Asynchronous on `stream`; first + n_out > n_rows is
 *     BEAR_ERR_INVALID_ARG, n_out = 0 BEAR_OK without a launch.  The lanes that read one row read neighbouring words (bytes).
 *     (bear_amd itself calls it through bear_shuffle_rows only: its streamed epochs gather on the host, below.)
 *   bear_shuffle_gather_host: the same rows from host `src` into host `dst` by n_threads (clamped to 1 .. 64) host threads, each
 *     a contiguous piece of the range.  Needs no device; synchronous.  This is how a streamed epoch and a rank's pieces of a
 *     shuffled table are gathered: the block then goes up like any other.
 */
int bear_shuffle_rows(const void *src, void *dst, uint64_t n_rows, uint32_t row_bytes, uint64_t seed, void *stream);
uint64_t bear_shuffle_source_row(uint64_t i, uint64_t n_rows, uint64_t seed);
int bear_shuffle_rows_range(const void *src, void *dst, uint64_t n_rows, uint64_t first, uint64_t n_out, uint32_t row_bytes,
                            uint64_t seed, void *stream);
int bear_shuffle_gather_host(const void *src, void *dst, uint64_t n_rows, uint64_t first, uint64_t n_out, uint32_t row_bytes,
                             uint64_t seed, int n_threads);

/*
 * k-mer order of a batch.  The sums of a training step (bear_net.py:146-197) do not depend on the order of a batch's rows, and
 * the fused AR-function entries below (bear_dm_linear_f64, bear_cnn_forward / backward_f64, bear_net_*_train_*_f64) run about
 * twice as fast when consecutive contexts share their leading letters -- 1.8 vs 2.9 ms (linear) and 54 vs 104 ms (cnn) per
 * 1e8 contexts: they are CORRECT for any order, the order is a performance precondition.  A caller establishes it once per
 * batch, before bear_plan_create (a plan is tied to the row order of the count slab it was built from):
 *   bear_kmer_order_u64: perm [dev] uint32 [n_rows] such that kmer_code[perm[0]] <= kmer_code[perm[1]] <= ... lexicographically
 *                        with the FIRST letter most significant (stable: equal contexts keep their order); kmer_code [dev] is
 *                        the bear_pack_kmers_u64 form; n_rows < 2^32.  The scratch is the CALLER's: call once with
 *                        scratch = NULL to get the size in *scratch_bytes (about 20 B per row + rocPRIM's temporary storage),
 *                        then with a 256-byte aligned device buffer of at least that size (*scratch_bytes = its size).
 *                        Asynchronous on `stream`: nothing is allocated, freed or waited for on the host.
 *   bear_gather_rows:    dst[i] = src[perm[i]] for rows of row_bytes bytes (20: a count slab; 8: packed contexts; lag: k-mer
 *                        bytes); dst != src; asynchronous on `stream`.
 * bear_amd.bear_net.train does exactly this at upload (bear_amd/_train.py: ResidentBatches(kmer_order=True)).
 */
int bear_kmer_order_u64(const uint64_t *kmer_code, uint64_t n_rows, int lag, uint32_t *perm, void *scratch, uint64_t *scratch_bytes,
                        void *stream);
int bear_gather_rows(const void *src, const uint32_t *perm, void *dst, uint64_t n_rows, uint32_t row_bytes, void *stream);

/*
 * k-mer transition counting on the device: the rows summarize.py produces through KMC and its stage-3
 * heap merge (bear_model/summarize.py:380-622), computed from the sequences as bear_model/tests/test_summarize.py:88-115
 * defines them.  Per lag: emit (context, group*5 + next letter) per transition, radix sort by context, run-length reduce.
 *   text  [dev] uint8 [n_pos]  per sequence: 5 (start), letters 0..3 (6 = any other character), 4 (stop); n_pos < 2^32
 *   group [dev] uint8 [n_pos]  group id of the sequence each position belongs to
 *   bear_kmer_sort_create: synchronous; *n_rows_out = number of distinct contexts (rows of the lag-`lag` table).
 *   bear_kmer_sort_reduce: kmers [dev, nullable] uint8 [n_rows, lag] ASCII ('[' padded as summarize.py:442);
 *                          kmer_code [dev, nullable] uint64 [n_rows] (bear_pack_kmers_u64 form);
 *                          counts [dev] uint32 [n_groups, n_rows, 5] (planar, the layout of bear_parse_counts_tsv).
 *   Rows come out sorted by packed context code; shuffle with bear_shuffle_rows before training.
 * bear_write_counts_tsv [host]: rows row_begin, row_begin + row_step, ... in the summarize.py text format
 *   (summarize.py:429-449), e.g. step = number of output bins.
 * bear_fastx_size / bear_fastx_encode [host]: a FASTA (fastq == 0) or FASTQ file as that code text (replacing the Biopython
 *   readers of summarize.py:96-100); reverse != 0 appends every sequence's reverse complement (summarize.py:202-207);
 *   group_out [nullable] receives `group` at every position.  Size first, then fill (`capacity` positions).
 *
 * The protein alphabet (rows of 21): the `_wide` twins take the row width, 5 or 21 (anything else BEAR_ERR_INVALID_ARG, checked
 * with every other argument before any device call); width 5 is the entry above, bit for bit.  At width 21
 *   text  per sequence: 21 (start), residues ARNDCEQGHILKMFPSTWYV -> 0..19 (22 = any other character), 20 (stop)
 *   key   5 bits per letter, letter l of the context in bits [5l, 5l + 5), 20 = '['; the sort reads 5 lag + 1 bits: lag <= 12
 *   value group * 21 + next letter;  a transition whose context or next letter holds a 22 is dropped, the others count
 *   bear_kmer_sort_reduce on such a handle (it remembers its width): kmers ASCII from "ARNDCEQGHILKMFPSTWYV[", counts uint32
 *     [n_groups, n_rows, 21] (the layout of bear_parse_counts_tsv_wide), rows ascending in the key; kmer_code must be NULL
 *     (the packed 3-bit code belongs to the 4-letter fused heads)
 *   bear_fastx_size_wide / bear_fastx_encode_wide: reverse != 0 is refused (no complement); a '*' that is the last character
 *     of a record is the stop the encoder writes anyway and is left out by both passes, any other '*' is a 22
 *   bear_write_counts_tsv_wide: the same rows with `width` counts per group (what bear_parse_counts_tsv_wide reads)
 *
 * Counting in passes over key ranges, for a text beyond one device sort (n_pos >= 2^32 - 1, or about 30 B per position more than
 * the device has).  The sort order is the key order, so the tables of disjoint ascending key ranges, concatenated, are the table.
 *   bin        of a valid transition: the top BITS * HL bits of its context key, key >> (BITS * (lag - HL)), with BITS = 3 and
 *              HL = min(lag, BEAR_COUNT_BIN_LETTERS) at width 5, BITS = 5 and HL = min(lag, BEAR_COUNT_BIN_LETTERS_WIDE) at width
 *              21: the context's last HL letters.  n_bins = 1 << (BITS * HL), at most 2^18 resp. 2^15.
 *   width      5 or 21, lag within the limits of bear_kmer_sort_create_wide; anything else is BEAR_ERR_INVALID_ARG
 *   bear_kmer_sort_bytes: peak device bytes of one counting pass over n_pairs pairs (the buffers of bear_kmer_sort_create and
 *              rocPRIM's temporary storage, asked of rocPRIM; nothing is allocated); n_pairs < 2^32 - 1
 *   bear_kmer_bin_hist: hist [dev] uint64 [n_bins] = valid transitions per bin (a dropped transition is counted nowhere); zeroed
 *              here; asynchronous on `stream`; n_bins must be the number the bin rule gives; n_pos may exceed 2^32
 *   bear_kmer_sort_create_range: bear_kmer_sort_create[_wide] over the transitions whose bin lies in [bin_lo, bin_hi), with
 *              bin_lo < bin_hi <= n_bins; capacity = their number (the histogram's sum over the range), < 2^32 - 1; synchronous.
 *              If the pass meets another number of pairs it returns BEAR_ERR_INVALID_ARG and leaves *out NULL (the text and the
 *              histogram do not belong together); it never writes beyond `capacity` pairs.  The handle goes to
 *              bear_kmer_sort_reduce and bear_kmer_sort_destroy like any other; *n_rows_out = the rows of the range.
 */
#define BEAR_COUNT_BIN_LETTERS 6      /* letters of a context that form its bin at 3 bits per letter (width 5) */
#define BEAR_COUNT_BIN_LETTERS_WIDE 3 /* ... at 5 bits per letter (width 21) */
int bear_fastx_size(const char *path, int fastq, int reverse, uint64_t *n_pos_out, uint64_t *n_seqs_out);
int bear_fastx_encode(const char *path, int fastq, int reverse, int group, uint64_t capacity, uint8_t *text,
                      uint8_t *group_out, uint64_t *n_pos_out);
typedef struct bear_kmer_sort bear_kmer_sort;
int bear_kmer_sort_create(const uint8_t *text, const uint8_t *group, uint64_t n_pos, int lag, bear_kmer_sort **out,
                          uint64_t *n_rows_out, void *stream);
int bear_kmer_sort_reduce(const bear_kmer_sort *h, int n_groups, uint8_t *kmers, uint64_t *kmer_code, uint32_t *counts,
                          void *stream);
int bear_kmer_sort_destroy(bear_kmer_sort *h);
int bear_count_last_hip_error(void);
int bear_write_counts_tsv(const char *path, const char *kmers, const uint32_t *counts, uint64_t n_rows, int lag, int num_ds,
                          uint64_t row_begin, uint64_t row_step, int append);
int bear_fastx_size_wide(const char *path, int fastq, int reverse, int width, uint64_t *n_pos_out, uint64_t *n_seqs_out);
int bear_fastx_encode_wide(const char *path, int fastq, int reverse, int width, int group, uint64_t capacity, uint8_t *text,
                           uint8_t *group_out, uint64_t *n_pos_out);
int bear_kmer_sort_create_wide(const uint8_t *text, const uint8_t *group, uint64_t n_pos, int lag, int width, bear_kmer_sort **out,
                               uint64_t *n_rows_out, void *stream);
int bear_write_counts_tsv_wide(const char *path, const char *kmers, const uint32_t *counts, uint64_t n_rows, int lag, int num_ds,
                               int width, uint64_t row_begin, uint64_t row_step, int append);
int bear_kmer_sort_bytes(uint64_t n_pairs, int lag, int width, uint64_t *bytes_out);
int bear_kmer_bin_hist(const uint8_t *text, uint64_t n_pos, int lag, int width, uint64_t *hist, uint64_t n_bins, void *stream);
int bear_kmer_sort_create_range(const uint8_t *text, const uint8_t *group, uint64_t n_pos, int lag, int width, uint64_t bin_lo,
                                uint64_t bin_hi, uint64_t capacity, bear_kmer_sort **out, uint64_t *n_rows_out, void *stream);

/*
 * Variant and sequence scoring on the device (get_var_probs.get_bear_probs / get_bear_probs_seqs with a DeviceCounter): what
 * stands between a count table in device memory and the samplers' tables above, and the exact marginal of whole segments, which
 * needs no table.  All four launch on `stream`; the look-ups (bear_score_transitions_u64, bear_kmer_find_u64) and a
 * bear_score_sum_f64 over a text of at most BEAR_SCORE_CHUNK positions are asynchronous, the entries that hold scratch of their own
 * (bear_score_sum_f64 beyond that, bear_score_marg_f64, bear_score_moments_f64) free it before they return, which waits for the
 * device: their outputs are then complete, and they do not belong inside a graph capture.
 *
 * The symbol text: uint8 codes as in the counting text -- letters 0 .. width - 2, the stop ']' = width - 1, the start '[' = width
 * -- with every start and stop written out (nothing is padded implicitly), cut into n_seg segments by
 *   seg [dev] uint64 [n_seg + 1], ascending, seg[0] = 0, seg[n_seg] = the number of symbols
 * (a variant window, a padded sequence).  A transition sits at every symbol that stands at least `lag` symbols into its segment.
 *
 * bear_score_transitions_u64: per symbol the key of the `lag` symbols in front of it and its letter.
 *   text [dev] uint8 [n_sym];  width 5 (lag <= 21, 3 bits per letter) or 21 (lag <= 12, 5 bits per letter)
 *   rank [host] uint8 [width + 1]: rank[c] = position of the character of code c among the alphabet's characters and '[' in byte
 *        order, 0xFF for the stop (which is no letter of a context).  key = sum over the context's letters of rank << bits *
 *        (lag - 1 - position): the first letter is the most significant, so the integer order of the keys is the order of the
 *        k-mer strings, and the number of a k-mer among the sorted distinct keys is its number in sorted(set(strings)).
 *   keys [dev] uint64 [n_sym], letters [dev] uint8 [n_sym]: the key and the letter index (stop = width - 1) of the transition at
 *        the symbol; 0xFF in every byte of both where there is none -- less than `lag` symbols into the segment, or a symbol
 *        that is no letter of its place (callers refuse those before the launch).
 * bear_kmer_find_u64: rows[q] = the index of query[q] in `table`, or 0xFFFFFFFF where it is absent.
 *   table [dev] uint64 [n_table] ascending and distinct, n_table < 2^32 - 1;  query [dev] uint64 [n_query] in any order (sorted
 *   queries keep the lanes of a wave on neighbouring entries);  rows [dev] uint32 [n_query].  n_table = 0 and n_query = 0 are valid.
 * bear_score_sum_f64: scores[i, :] = sum over the transitions t of segment i, in text order, of lp[rows[t], letters[t], :].
 *   lp [dev] double [n_rows, width, n_values]: the table bear_logdir_sample[_wide]_f64 leaves (n_values = n_models * mc_samples)
 *   rows [dev] uint32 [n_t], letters [dev] uint8 [n_t]: per position of the text the table row and the letter; a position with
 *        letter 0xFF (or a row >= n_rows, a letter >= width) adds nothing;  seg as above with seg[n_seg] = n_t
 *   scores [dev] double [n_seg, n_values].  A segment of at most BEAR_SCORE_CHUNK transitions is summed front to back; a longer one
 *        in chunks of BEAR_SCORE_CHUNK transitions from its start, whose partial rows are added in chunk order.  No atomics: the
 *        same arguments give the same bits, in both libraries, wherever the segment stands in the text.  Holds two partial rows
 *        per BEAR_SCORE_CHUNK positions of a text longer than that, and frees them before it returns.
 */
#define BEAR_SCORE_CHUNK 2048
int bear_score_transitions_u64(const uint8_t *text, const uint64_t *seg, uint64_t n_sym, uint64_t n_seg, int lag, int width,
                               const uint8_t *rank, uint64_t *keys, uint8_t *letters, void *stream);
int bear_kmer_find_u64(const uint64_t *table, uint64_t n_table, const uint64_t *query, uint64_t n_query, uint32_t *rows,
                       void *stream);
int bear_score_sum_f64(const double *lp, uint64_t n_rows, int width, uint64_t n_values, const uint32_t *rows, const uint8_t *letters,
                       uint64_t n_t, const uint64_t *seg, uint64_t n_seg, double *scores, void *stream);

/*
 * bear_score_marg_f64: the exact Dirichlet-multinomial marginal of every segment under n_h BEAR and n_van vanilla models
 * (get_bear_probs_seqs(..., get_marg=True)): scores[s, m] = sum over the distinct k-mers r of segment s of
 *     lgamma(A) - lgamma(A + n) + sum over the letters j with q_j > 0 of [lgamma(a_j + q_j) - lgamma(a_j)]
 * with q[] the letter counts of r's transitions inside s, n their sum, c[] = train[r, :],
 *     a_j = fma(prior[r, j], 1 / h_m, c_j) for the BEAR model m < n_h,   a_j = van_(m - n_h) + c_j for a vanilla model,
 * and A the sum of a_0 .. a_(width - 1) in that order.  Both brackets are log rising factorials over an exact integer (the item
 * routine of the training kernels); there is no multinomial coefficient.
 *   rows [dev] int32 [n_t], letters [dev] uint8 [n_t]: per position of the text the k-mer's row in `train` and the letter, SORTED
 *        inside every segment by (row, letter), so that seg stays valid; a position without a transition has a negative row and
 *        the letter 0xFF and sorts in front (a row >= n_rows or a letter >= width is such a position too).  A run -- a maximal
 *        stretch of equal (row, letter) inside a segment -- is one q_j, the stretch of equal row is the k-mer's n.  Unsorted input
 *        gives another sum (every run is then a k-mer's letter of its own); nothing is read outside the arrays whatever they hold.
 *   seg  [dev] uint64 [n_seg + 1] as above with seg[n_seg] = n_t;  width 5 or 21
 *   train [dev] uint32 [n_rows, width] (n_rows < 2^32 - 1);  prior [dev, nullable] double [n_rows, width], needed when n_h > 0
 *   h [host] double [n_h], van [host] double [n_van], every value > 0;  1 <= n_h + n_van <= BEAR_MARG_MAX_MODELS
 *   scores [dev] double [n_seg, n_h + n_van]: BEAR models first, then the vanilla ones; a segment without transitions scores 0.
 * Every position's term is formed once (one thread per position; the head of a run finds its end by binary search), then summed
 * per segment in chunks of BEAR_MARG_CHUNK positions cut from the segment's own start: inside a chunk position p goes to lane
 * (p - chunk start) mod 64, a lane adds its positions front to back, the 64 lanes are added in a fixed tree, and the chunks'
 * sums are added in chunk order.  No atomics: a segment's bits depend on its own content only -- not on where it stands in the
 * text, on the other segments, on the grid or on the library.  Holds n_t * (n_h + n_van) terms and, for a text beyond
 * BEAR_MARG_CHUNK positions, two partial rows per BEAR_MARG_CHUNK positions, and frees them before it returns.
 * Refused with BEAR_ERR_INVALID_ARG before any device call: a width other than 5 / 21, n_h > 0 without a prior, an h or van that
 * is not > 0, n_h + n_van of 0 or beyond BEAR_MARG_MAX_MODELS, n_rows >= 2^32 - 1, a missing or misaligned pointer.  n_seg = 0 is
 * valid and launches nothing.
 */
#define BEAR_MARG_CHUNK 2048
#define BEAR_MARG_MAX_MODELS 16
int bear_score_marg_f64(const int32_t *rows, const uint8_t *letters, uint64_t n_t, const uint64_t *seg, uint64_t n_seg, int width,
                        const uint32_t *train, const double *prior, uint64_t n_rows, const double *h, int n_h, const double *van,
                        int n_van, double *scores, void *stream);

/*
 * bear_score_groups_f64: bear_score_marg_f64 under every group (column) of a count table at once, with an optional leave-one-out
 * group per segment (bear_amd.classify, kernels_groups.h): which group does a segment belong to.  rows, letters, seg, width, prior,
 * h and van are exactly bear_score_marg_f64's, positions sorted by (row, letter) inside each segment; a position's run, its k-mer's
 * stretch and its prior row are found once and serve every group.
 *   train [dev] uint32 [n_rows, n_groups, width]: the n_groups count rows of one k-mer are adjacent;  1 <= n_groups <= BEAR_GROUPS_MAX
 *   own   [dev, nullable] int32 [n_seg]: the group whose counts contain segment s itself; negative or >= n_groups: none; NULL: no
 *         segment has one
 *   scores [dev] double [n_seg, n_groups, n_h + n_van]: the formula of bear_score_marg_f64 with c[] = train[r, g, :] -- and with
 *         c_j - q_j in place of c_j, for every letter j of the k-mer, an exact integer subtraction before the conversion to double,
 *         where g = own[s]: the marginal of s under the posterior of the group WITHOUT s.  Without own, scores[:, g, :] are the
 *         bits of bear_score_marg_f64 on column g; with it, scores[s, own[s], :] are its bits on that column less the segment's
 *         counts.
 *   short_of [dev] uint8 [n_seg], zeroed by the entry: 1 where some c_j < q_j in the segment's own group -- the table does not
 *         hold that segment.  Its own-group scores are NaN; every other score of the call is what it is without that own[s].
 * Terms [n_groups * (n_h + n_van), n_t] and the sums of bear_score_marg_f64 with n_groups * (n_h + n_van) models; no atomics: a
 * segment's bits depend on its content, its own[] value and the table only, in both libraries.  Asynchronous on `stream`: the
 * terms and the partial rows come from the device's memory pool in stream order (hipMallocAsync / hipFreeAsync), the entry waits
 * for nothing; outputs are valid once the stream is synchronised.  It does not belong inside a graph capture.
 * Refused with BEAR_ERR_INVALID_ARG before any device call: everything bear_score_marg_f64 refuses, n_groups out of range, a missing
 * scores or short_of, a misaligned own.  n_seg = 0 is valid and launches nothing.
 * The stream is deliberately NOT the last parameter, as for bear_two_sample_f64 and for the same reason; tests/test_classify_gpu.py
 * holds the entry to the contract with the harness of tests/stream_util.py.
 */
#define BEAR_GROUPS_MAX 256
int bear_score_groups_f64(const int32_t *rows, const uint8_t *letters, uint64_t n_t, const uint64_t *seg, uint64_t n_seg,
                          int width, const uint32_t *train, int n_groups, const double *prior, uint64_t n_rows,
                          const int32_t *own, const double *h, int n_h, const double *van, int n_van,
                          void *stream, double *scores, uint8_t *short_of);

/*
 * Segmenting sequences among the groups of a count table (bear_amd.classify.segment, kernels_segment.h): WHERE in a sequence does
 * which group speak.  Two entries: the log-probability of every position's letter under every group, and a hidden-Markov chain
 * over the groups.  Both are asynchronous on `stream`, which is deliberately NOT their last parameter (as for
 * bear_score_groups_f64 and for the same reason; tests/test_segment_gpu.py holds them to the contract with the harness of
 * tests/stream_util.py).
 *
 * bear_score_emit_groups_f64: the posterior-predictive log-probability of the letter of every position under every group and model.
 * rows, letters, width, train, n_groups, prior, n_rows, h, van are bear_score_groups_f64's, but the positions stand in TEXT order
 * (nothing is sorted, there are no segments here: a position is one transition).  For position t with row r and letter l, group g
 * and model m, with c[] = train[r, g, :],
 *     a_j = fma(prior[r, j], 1 / h_m, c_j) for the BEAR model m < n_h,   a_j = van_(m - n_h) + c_j for a vanilla model,
 *     A = a_0 + ... + a_(width - 1) in that order  (a_j and A bit for bit those of bear_score_groups_f64),
 *     emit[m, t, g] = log(a_l) - log(A): a DIFFERENCE of two logs, not one log of the quotient -- each log is off by its own
 *     rounding only, so the error is relative to |log a_l| + |log A| even where both are tiny (an unseen k-mer at h = 1 under a
 *     prior row that one letter dominates: a_l and A are both next to 1, and the quotient's rounding would be all of the value).
 * This is the exact marginal of the single transition, so a k-mer that no group has seen scores through the prior alone.  A
 * position without a transition (a negative row, a row >= n_rows, a letter >= width) has exactly 0.0 for every group and model.
 *   emit [dev] double [n_h + n_van, n_t, n_groups]: model-major, the n_groups values of a position adjacent -- plane m is the
 *        emit [n_t, n_states] that bear_hmm_groups_f64 takes.
 * One thread per position; the prior row and the k-mer's n_groups rows are read once.  Refused with BEAR_ERR_INVALID_ARG before
 * any device call: everything bear_score_groups_f64 refuses of these arguments (the width, the models, n_groups, n_rows), a missing
 * or misaligned pointer.  n_t = 0 is valid and launches nothing.
 *
 * bear_hmm_groups_f64: a hidden-Markov chain over n_states states along every segment, generic over where its emissions came from.
 *   emit [dev] double [n_t, n_states];  seg [dev] uint64 [n_seg + 1] ascending offsets into the steps, seg[0] = 0 and seg[n_seg] =
 *        n_t -- the entry cannot check device values: a step that no segment covers keeps whatever path and log_post held: segment i
 *        has the steps 0 .. T - 1 = seg[i] .. seg[i + 1] - 1, e_t its emission rows.  Every step emits: the entry knows no silent
 *        step (the caller drops the positions without a transition, or keeps their zeros as uninformative steps).
 *   log_trans [host] double [n_states, n_states], from-state by row;  log_start [host] double [n_states].  -inf is allowed and
 *        rows need not be normalised;  1 <= n_states <= BEAR_HMM_MAX_STATES
 *   Sum-product:  alpha_0 = log_start + e_0;  alpha_t(g) = e_t(g) + lse_h(alpha_(t-1)(h) + log_trans[h, g]);  beta_(T-1) = 0;
 *        beta_t(g) = lse_h(log_trans[g, h] + e_(t+1)(h) + beta_(t+1)(h));  lse = max + log(sum of exp(x - max)) in state order, and
 *        -inf over only -inf, never NaN.
 *   Max-plus: the same recurrences with max in place of lse give delta and eta.
 *   log_evidence [dev] double [n_seg] = lse_g alpha_(T-1)(g);   log_best [dev] double [n_seg] = max_g delta_(T-1)(g)
 *   path [dev] uint8 [n_t]: the LOWEST g that maximises the max-marginal delta_t(g) + eta_t(g).  Wherever the best path is unique
 *        this is the Viterbi path.  On a tie the lowest index is taken position by position, which need not be one consistent
 *        path (two best paths A A B B and A B B B give A A B B here only by the index rule).
 *   log_post [dev, nullable] double [n_t, n_states] = alpha_t(g) + beta_t(g) - log_evidence; exactly -inf for a state no path of
 *        finite value passes through at t.  NULL: not formed -- the sum pass then carries no backward vector and only a
 *        segment's last chunk recomputes its forward values, for log_evidence (the max pass runs whole: path needs eta).
 *   T = 0: log_evidence = lse(log_start), log_best = max(log_start), nothing per position.  Every path -inf: log_evidence and
 *        log_best are -inf, the segment's log_post is NaN and its path 255.
 * The chunk rule.  A segment is cut from its own start into chunks of BEAR_HMM_CHUNK steps.  A segment of one chunk is run front
 * to back and back to front by one lane group, nothing else.  For a longer one (1) every chunk's n_states x n_states transfer
 * matrix is formed -- row i: the forward recurrence over the chunk's steps from the unit vector of state i, in the semiring of the
 * pass; the first chunk's first step takes no transition --, (2) the vector that enters each chunk (log_start, then one
 * vector-matrix product per chunk in chunk order) and the vector that leaves it (0, then one product per chunk in reverse order)
 * are carried along, (3) every chunk recomputes its forward values from the vector that enters it and its backward values from
 * the one that leaves it.  The scalars are those of the last chunk's recomputed forward values, and (4) one more launch takes that
 * log_evidence off the alpha + beta of every step of such a segment, so log_post + log_evidence is alpha + beta to the bit in
 * every chunk.  A text beyond BEAR_HMM_CHUNK steps that holds only short segments still pays for the launches of (1), (2) and
 * (4) and for the scratch below: the host sees n_t, not the offsets -- their items find no long segment and form nothing.
 * No atomics; every reduction runs in state order: a segment's bits depend on its own emissions and the chain
 * only -- not on where it stands in the text, on its neighbours, on the grid or on the library.
 * Holds n_t * n_states forward values and, for a text beyond BEAR_HMM_CHUNK steps, two matrices and four vectors per
 * BEAR_HMM_CHUNK steps, from the device's memory pool in stream order (hipMallocAsync / hipFreeAsync): the entry waits for
 * nothing, outputs are valid once the stream is synchronised; it does not belong inside a graph capture.
 * Refused with BEAR_ERR_INVALID_ARG before any device call: n_states out of range; a log_trans or log_start that is missing, holds
 * a NaN or +inf, or has a row (log_start: the vector) without a finite entry; a missing or misaligned pointer.  n_seg = 0 is valid
 * and launches nothing (n_t = 0 with segments: every one is empty and gets the T = 0 scalars).
 */
#define BEAR_HMM_MAX_STATES 16
#define BEAR_HMM_CHUNK 512
int bear_score_emit_groups_f64(const int32_t *rows, const uint8_t *letters, uint64_t n_t, int width, const uint32_t *train,
                               int n_groups, const double *prior, uint64_t n_rows, const double *h, int n_h,
                               const double *van, int n_van, void *stream, double *emit);
int bear_hmm_groups_f64(const double *emit, uint64_t n_t, const uint64_t *seg, uint64_t n_seg, int n_states,
                        const double *log_trans, const double *log_start, void *stream,
                        double *log_evidence, double *log_best, uint8_t *path, double *log_post);

/*
 * bear_score_moments_f64: the exact posterior mean and variance of every segment's score under n_h BEAR and n_van vanilla models
 * (get_bear_probs / get_bear_probs_seqs with moments=True): what the mc_samples axis of bear_logdir_sample[_wide]_f64 +
 * bear_score_sum_f64 samples, in closed form.  The arguments, models, concentrations (a_j and A bit for bit), sums, checks and
 * status codes of bear_score_marg_f64, and
 *   weight_prefix [dev, nullable] int64 [n_t + 1]: weight_prefix[k] = the sum of the weights (+1: the transition counts for the
 *        score, a sequence or a mutant window; -1: against it, the wild-type window) of the SORTED positions in front of k, so
 *        weight_prefix[0] = 0; NULL: every weight is +1.  The signed count of a stretch is the difference of two entries.
 *   moments [dev] double [n_seg, n_h + n_van, 2]: with m_j the signed count of the run (r, j) inside segment s and M_r their sum,
 *        moments[s, m, 0] = sum over the k-mers r of s of [sum_j m_j psi(a_j) - M_r psi(A)]                    (the mean)
 *        moments[s, m, 1] = sum over the k-mers r of s of [sum_j m_j^2 psi1(a_j) - M_r^2 psi1(A)]              (the variance)
 *        psi the digamma, psi1 the trigamma function (log p of p ~ Dirichlet(a) has the covariance delta_jk psi1(a_j) - psi1(A);
 *        the k-mers are independent).  The variance comes out as summed: rounding can leave it a few ulps of its terms below 0,
 *        nothing is clamped.  A run with m_j = 0 and a k-mer with M_r = 0 add exact zeros: psi is not evaluated for them.
 * Holds 2 * n_t * (n_h + n_van) terms and, for a text beyond BEAR_MARG_CHUNK positions, two partial rows per BEAR_MARG_CHUNK
 * positions, and frees them before it returns.  Refused with BEAR_ERR_INVALID_ARG before any device call: everything
 * bear_score_marg_f64 refuses, and a misaligned weight_prefix.  n_seg = 0 is valid and launches nothing.
 */
int bear_score_moments_f64(const int32_t *rows, const uint8_t *letters, const int64_t *weight_prefix, uint64_t n_t, const uint64_t *seg,
                           uint64_t n_seg, int width, const uint32_t *train, const double *prior, uint64_t n_rows, const double *h,
                           int n_h, const double *van, int n_van, double *moments, void *stream);

/*
 * Sequence generation on the device (assemble.assemble_no_ends with a DeviceCounter): every sequence grows from its end k-mer, one
 * letter per step, under the transition table of a count column -- sampled from its posterior, one sample per sequence, or at its
 * MAP value.  Asynchronous on `stream`; one launch.
 *
 * bear_generate_steps_f64: steps t = step0 .. step0 + n_steps - 1 of the sequences that have letters left.
 *   table  [dev, nullable] uint64 [n_table] ascending and distinct keys of bear_score_transitions_u64 (same lag, width, rank),
 *          n_table < 2^32 - 1;  counts [dev, nullable] uint32 [n_table, width], row j the counts of table[j] (KEY order).  A k-mer
 *          that is absent is a row of zeros; n_table = 0 (then both may be NULL) is valid.
 *   lag, width, rank [host] uint8 [width + 1]: as for bear_score_transitions_u64
 *   keys   [dev] uint64 [n_seq]: the end key of every sequence; read, and written back after its last step here
 *   sample [dev] uint64 [n_seq]: the sample index s of every sequence (two sequences with one index share their table)
 *   left   [dev] uint32 [n_seq]: letters still to write; a sequence takes min(left, n_steps) steps and left goes down by as many
 *   Per step, for the letters b < width - 1 (the stop is never drawn), with c[] the count row of the key q:
 *     concentration  mode BEAR_GEN_BMM: van + c[b];  BEAR_GEN_BEAR: fma(prior[i, b], 1 / h, c[b]);  BEAR_GEN_AR: prior[i, b]
 *     table value    map == 0: one log Gamma(concentration) draw keyed by (seed, model 0, s, mix64(q) + b) -- the draw of
 *                    bear_log_gamma_f64; a pure function of the key, so a sequence that returns to a k-mer meets the same row;
 *                    map != 0: log(concentration).  (The row's common normaliser is not formed: it cannot change the letter.)
 *     letter         the lowest b with the largest value + Gumbel draw keyed by (seed, model 3000, s, t * width + b); it goes to
 *                    letters[i * letters_stride + t] and q becomes ((q << bits) | rank[letter]) & (2^(bits * lag) - 1)
 *   prior  [dev, nullable] double [n_seq, width]: the rows of the sequences' CURRENT end k-mers (an AR function's output); with a
 *          prior n_steps must be at most 1 (the caller forms the next rows from `codes`); NULL: BEAR_GEN_BMM only, any n_steps --
 *          a whole flank in one launch.  BEAR_GEN_AR is a table only at its MAP value (map != 0).
 *   letters [dev] uint8 [n_seq, letters_stride], letters_stride >= step0 + n_steps; entries of steps not taken are left alone
 *   codes  [dev, nullable] int8 [n_seq, lag]: the new end k-mer of EVERY sequence as letter codes 0 .. width - 2, '[' = width - 1
 *          (what an AR function takes)
 * Refused with BEAR_ERR_INVALID_ARG before any launch: a width other than 5 / 21, a lag outside 1..21 / 1..12, n_steps > 1 with a
 * prior, a mode that needs a prior without one, BEAR_GEN_AR without map, h (BEAR_GEN_BEAR) or van (BEAR_GEN_BMM) not > 0, a
 * letters_stride below step0 + n_steps.  No atomics and no sums across lanes: the same arguments give the same letters in both
 * libraries, and n steps in one launch are the letters of any cut of them into launches that continue at step0.
 */
#define BEAR_GEN_BMM 0
#define BEAR_GEN_BEAR 1
#define BEAR_GEN_AR 2
int bear_generate_steps_f64(const uint64_t *table, const uint32_t *counts, uint64_t n_table, int lag, int width, const uint8_t *rank,
                            int mode, int map, double h, double van, const double *prior, uint64_t seed, uint64_t *keys,
                            const uint64_t *sample, uint32_t *left, uint64_t n_seq, uint64_t step0, uint64_t n_steps,
                            uint8_t *letters, uint64_t letters_stride, int8_t *codes, void *stream);

/*
 * bear_generate_whole_f64: whole sequences, from a start context to the stop (assemble.generate_sequences).  The steps, streams
 * and arguments of bear_generate_steps_f64, with the stop b = width - 1 drawn like a letter: per step the values of ALL width
 * letters are formed (for b < width - 1 bit for bit those of bear_generate_steps_f64: same keys, same concentration) and the
 * lowest b with the largest value wins.
 *   the stop wins:    stopped[i] = 1, left[i] = 0; nothing is written to letters, the key is not advanced
 *   a letter wins:    letters[i * letters_stride + t] = b, the key is shifted as above, length[i] += 1, left[i] -= 1
 *   left    [dev] uint32 [n_seq]: steps the sequence may still take (the cut: a sequence that reaches 0 unstopped was cut there)
 *   length  [dev] uint32 [n_seq]: letters written so far;  stopped [dev] uint8 [n_seq]: set to 1 by the stop, else left alone.
 *           keys, left, length and stopped are the whole state, read and written: n steps in one launch are the bytes of any cut
 *           of them into launches that continue at step0.
 *   The rows f of the AR function (BEAR_GEN_BEAR: fma(f[b], 1 / h, c[b]); BEAR_GEN_AR: f[b]) come from one of
 *   prior  [dev, nullable] double [n_seq, width]: the rows of the CURRENT end k-mers, n_steps at most 1, as above; or
 *   mat    [dev, nullable] double [lag, 21, 21], width 21 only: the linear AR function inside the kernel -- per step the row
 *          softmax_b(sum_l mat[l, code[l], b]) of the end k-mer's codes ('[' = 20), bit for bit the row
 *          bear_linear_forward_wide_f64 writes for them; any n_steps: whole sequences under a trained linear model in one launch.
 *          mat and the exp table are staged in LDS once per block; the grid of this variant is capped at 512 blocks.
 * Refused with BEAR_ERR_INVALID_ARG before any device call: everything bear_generate_steps_f64 refuses (a mode that needs rows
 * with neither prior nor mat), prior and mat both given, mat at width 5, n_steps > 1 with a prior, a missing or misaligned
 * length or stopped.  n_seq = 0 is valid and launches nothing.  No atomics and no sums across lanes: the same bytes in both
 * libraries.
 */
int bear_generate_whole_f64(const uint64_t *table, const uint32_t *counts, uint64_t n_table, int lag, int width, const uint8_t *rank,
                            int mode, int map, double h, double van, const double *prior, const double *mat, uint64_t seed,
                            uint64_t *keys, const uint64_t *sample, uint32_t *left, uint32_t *length, uint8_t *stopped, uint64_t n_seq,
                            uint64_t step0, uint64_t n_steps, uint8_t *letters, uint64_t letters_stride, int8_t *codes, void *stream);

/*
 * bear_ref models downstream of training.  The AR function's row of a k-mer under a model trained by bear_ref is a function of the
 * k-mer's REFERENCE count row as well: with A = width - 1 letters, the stop last, ref the uint32 row of the reference column (zeros
 * where the reference table lacks the k-mer) and g the net function's row (the one-hot at the stop for the stop net function),
 *     r_b = ref_b + eps (b < A), r_A = 0;   R = sum_b r_b, added as NumPy's add.reduce adds W contiguous doubles
 *     dev_b = r_b / R - 1/A (b < A), dev_A = 0: the quotient rounded as a division, the subtraction unfused
 *     jc_b = fma(E, dev_b, [b < A] / A);   f_b = fma(nw, g_b, jc_b) * V;   prior_b = f_b + eps
 * E = exp(-tau) and V = 1 / (nw + 1) are formed ONCE on the host from tau and net_weight (the model's exp(tau_signed) and
 * exp(net_weight_signed)) and reach the kernel by value; on the device there is nothing but add, multiply, fma and the rounded
 * quotient, so a host replica with an exact fma gives the same bits.  prior is "the AR function's row" every consumer takes: the
 * + eps is load_bear's wrapper of an AR function, not the f / h + c + eps of a training step.
 *
 * bear_ref_prior_rows_f64: prior[q, :] for every query key.
 *   ref_table [dev, nullable] uint64 [n_ref] ascending and distinct keys of bear_score_transitions_u64, n_ref < 2^32 - 1;
 *   ref_counts [dev, nullable] uint32 [n_ref, width], row j the reference counts of ref_table[j] (KEY order); n_ref = 0 is valid
 *   query [dev] uint64 [n_query] in any order;  net_rows [dev, nullable] double [n_query, width]: g, NULL for the stop net function
 *   prior [dev] double [n_query, width].  n_query = 0 is valid and launches nothing.  One thread per query; no atomics.
 * Refused with BEAR_ERR_INVALID_ARG before any launch: a width other than 5 / 21, tau or net_weight not finite and > 0, eps not
 * finite and >= 0, n_ref >= 2^32 - 1, a missing or misaligned pointer.
 *
 * bear_generate_whole_ref_f64: bear_generate_whole_f64 under such a model -- its arguments, steps, streams and state, with the row
 * f of the current end k-mer formed inside the step: the group's first lane finds the k-mer in `table` and in `ref_table`, every
 * letter lane forms R of the reference row itself (the same additions in the same order: equal bits on all lanes, no sum across
 * lanes) and its own prior_b, and goes on as bear_generate_whole_f64 does with f from `prior`.  The net function's row g is
 *   net BEAR_GEN_NET_STOP  the one-hot at the stop; prior and mat NULL, any n_steps: whole sequences in one launch
 *   net BEAR_GEN_NET_ROWS  prior [dev] double [n_seq, width]: g of the CURRENT end k-mers, n_steps at most 1
 *   net BEAR_GEN_NET_MAT   formed from mat [dev] double [lag, 21, 21] as bear_generate_whole_f64 forms f from it; width 21, any n_steps
 * mode is BEAR_GEN_BEAR (fma(prior_b, 1 / h, c[b])) or BEAR_GEN_AR (prior_b; map != 0); van is not read.
 * Refused with BEAR_ERR_INVALID_ARG before any device call: everything bear_generate_whole_f64 refuses, BEAR_GEN_BMM, a net other
 * than the three, prior or mat given or missing against `net`, tau / net_weight / eps as above, n_ref >= 2^32 - 1, a missing or
 * misaligned ref_table / ref_counts with n_ref > 0.  n_seq = 0 is valid and launches nothing.  The same bytes in both libraries
 * and for any cut of the steps into launches.
 */
#define BEAR_GEN_NET_STOP 0
#define BEAR_GEN_NET_ROWS 1
#define BEAR_GEN_NET_MAT 2
int bear_ref_prior_rows_f64(const uint64_t *ref_table, const uint32_t *ref_counts, uint64_t n_ref, int width, const uint64_t *query,
                            uint64_t n_query, const double *net_rows, double tau, double net_weight, double eps, double *prior,
                            void *stream);
int bear_generate_whole_ref_f64(const uint64_t *table, const uint32_t *counts, uint64_t n_table, int lag, int width, const uint8_t *rank,
                                int mode, int map, double h, double van, const double *prior, const double *mat, uint64_t seed,
                                uint64_t *keys, const uint64_t *sample, uint32_t *left, uint32_t *length, uint8_t *stopped, uint64_t n_seq,
                                uint64_t step0, uint64_t n_steps, uint8_t *letters, uint64_t letters_stride, int8_t *codes,
                                const uint64_t *ref_table, const uint32_t *ref_counts, uint64_t n_ref, double tau, double net_weight,
                                double eps, int net, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BEAR_HIP_H */
