"""Developer: the bits of every width-taking entry, of the width-5 convolutional entries and of the width-5 fused linear step on seeded
inputs, for holding one build of the library against another.
    BEAR_AMD_LIB=before/libbear_hip.so python scripts/dev/wide_bits.py > before.json
    BEAR_AMD_LIB=bear_amd/libbear_hip.so python scripts/dev/wide_bits.py > after.json        # then: cmp before.json after.json
Section names (the functions below: row_kernels, linear_kernels, cnn_kernels, cnn5_kernels, linear5_kernels, exact_kernels) behind
the script's name run those sections alone; none: all of them.  One SHA-256 per output buffer, as one JSON object (case -> digest).  These kernels use no floating-point atomics and the library is
built without contraction: on one device two builds that compute the same thing give the same file, and any difference is a
difference in the arithmetic or in its order.  Each build runs in a process of its own (the library is loaded once).

Shapes: the smallest at which the routines the width-21 kernels share can go wrong -- the code bytes of a tile not a whole number
of dwords, a ragged last tile and a second tile per block, rows of 3 tiles + 77 at either width, and per kernel one table with more
tiles than its capped grid has blocks (cap * tile + tile + 3 rows).

The width-5 convolutional head (kernels_cnn.h; packed contexts, start symbols and unknown letters mixed in; one table in random and
one in k-mer order with duplicate contexts per shape, so that shared and carried windows occur): the forward kernels, the row sums
and the dT1 rows use no atomics and are hashed in either build.  The part kernel and the 64-context kernel add to their block's
gradient image with LDS floating-point atomics from several waves: their parameter gradients are hashed in libbear_hip_det.so only
(one wave per block); so is `packed` of the step over levels and tables, the head-only backward kernel's gradients included -- that
kernel has no atomics itself, but the part-kernel launches of the same step add to the same partial rows.

The width-5 fused linear step (kernels_linear.h, `dm_linear`): sizes of one context, 3 tiles + 77 and a second tile for every block
(a tile is 1664 contexts, one block per CU); lags 1 and 3 (the triple alone), 5, 13, 14 (the specialised group counts), 9 and 21
(run-time count; 21: the last arm of the switch), each once more with BEAR_AMD_LINEAR_GENERIC=1; three tables of contexts (`codes5`
in k-mer order with copies of a k-mer, `codes5_prefixes`, `codes5` in random order, where pairing declines), each with its plain
and its paired lists, BEAR and AR form; parameters that give tables of exponentials, tables of logits and a saturated softmax.  The
section runs with BEAR_AMD_DETERMINISTIC=1 (set inside it only, restored after): the gradient tables are then fixed-point and
`grad_mat` is the same bits in either library whatever the order of the adds -- hashed in both; `out` (sum LL, d/dh) is summed in
the order the work units were drawn in libbear_hip.so and is hashed in libbear_hip_det.so only.  Without the switch d/d mat goes
through LDS floating-point atomics from several waves and is not hashable in either library: those instantiations are held to the
oracle by the parity tests.  A tile denser than its in-tile lists (the loop over the plan's overflow items) comes from the parity
tests' `mixed_heavy_table`, in libbear_hip_det.so only: the other library's plan of such a table differs from build to build of
the plan in which cells overflow, and with it the fixed-point roundings.

The exact marginals and the Bayes factors (`exact_kernels`: score_marg, score_moments, score_groups; two_sample, k_sample) have no
atomics and are hashed in both libraries, at both widths.  One text for the first three: 3 * 256 + 77 positions cut into four
segments, one of them empty, then one segment of 2 * MARG_CHUNK + 5 positions that holds a run of 150 equal (row, letter);
positions with SCORE_SKIP, with a negative row and with a row beyond the table.  score_groups at G = 1 and 3, without `own` and
with an `own` that holds -1, a value >= G and, for the long segment, a group whose counts do not hold it (NaN scores, `short_of`);
the other segments' own groups hold them.  The tables of the Bayes factors: tile - 1 and tile + 1 rows and one table beyond the
capped grid; four models (two BEAR, two vanilla) and five (a second launch), each plain and with the AR sums and the row terms;
k_sample at G = 2, 3 and 16 columns of an 18-column table."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bear_amd import kernels  # noqa: E402

OUT = {}
POINT = (0.37, -1.2, -0.8)
# tiles and grid caps (blocks per CU) that bear_amd.kernels does not name: kernels_wide.h (WIDE_TILE, WIDE_BLOCKS_PER_CU; EVW_THREADS
# and the workspace's eval_blocks), kernels_linrows_wide.h (LNW_FWD_TILE, one block per CU), kernels_cnn_wide.h (CNW_FWD_TILE, at most
# two blocks per CU; CNW_BWD_TILE, CNW_BWD_BLOCKS_PER_CU)
PRIOR_TILE, PRIOR_PER_CU = {21: 128, 5: 512}, 4
EVAL_TILE, EVAL_PER_CU = 128, 8
LINEAR_FWD_TILE, LINEAR_FWD_PER_CU = 512, 1
CNN_FWD_TILE, CNN_FWD_PER_CU = 256, 2
CNN_BWD_TILE, CNN_BWD_PER_CU = 64, 1
# the width-5 convolutional kernels (kernels_cnn.h, bear_cnn.hip): waves per CU of each capped grid and contexts per wave tile
CNN5_FWD_WAVES_PER_CU, CNN5_FWD_TILE = 16 * 4, 64
CNN5_PARTS_WAVES_PER_CU, CNN5_HEAD_WAVES_PER_CU, CNN5_PARTS_TILE = 8, 12, 32
# the width-5 fused linear step (kernels_plan.h: PLN_RMAX contexts per tile, one block per CU)
LINEAR5_TILE, LINEAR5_PER_CU = 1664, 1


def beyond(cus, per_cu, tile):
    """Rows of a table with more tiles than the capped grid has blocks: every block a second tile, one a ragged third."""
    return cus * per_cu * tile + tile + 3


def put(name, *tensors):
    for i, t in enumerate(tensors):
        OUT["%s/%d" % (name, i)] = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def counts(rng, n, width, p=0.13, lam=6.0):
    c = np.where(rng.random((n, width)) < p, rng.poisson(lam, (n, width)), 0).astype(np.uint32)
    c[::7] = 0                                           # contexts without counts
    return torch.from_numpy(c.view(np.int32)).cuda()


def rows(rng, n, width):
    z = rng.normal(size=(n, width)) * 2.0
    g = np.exp(z - z.max(1, keepdims=True))
    return torch.from_numpy(np.ascontiguousarray(g / g.sum(1, keepdims=True))).cuda()


def codes(rng, n, lag):
    c = rng.integers(0, 21, (n, lag)).astype(np.int8)
    c[rng.random((n, lag)) < 0.05] = -1                  # unknown letters
    return torch.from_numpy(c).cuda()


def f64(*v):
    return torch.tensor(v, dtype=torch.float64, device="cuda")


def row_kernels(cus):
    for width in kernels.WIDE_WIDTHS:
        sizes = {"prior": [3 * PRIOR_TILE[width] + 77, beyond(cus, PRIOR_PER_CU, PRIOR_TILE[width])],
                 "eval": [3 * EVAL_TILE + 77, beyond(cus, EVAL_PER_CU, EVAL_TILE)],
                 "ref": [3 * kernels.REF_WIDE_TILE[width] + 77, beyond(cus, kernels.REF_WIDE_BLOCKS_PER_CU, kernels.REF_WIDE_TILE[width])],
                 "mix": [3 * kernels.REFMIX_WIDE_TILE[width] + 77,
                         beyond(cus, kernels.REFMIX_WIDE_BLOCKS_PER_CU, kernels.REFMIX_WIDE_TILE[width])]}
        for n in sizes["prior"]:
            rng = np.random.default_rng(n + width)
            c, f, h = counts(rng, n, width), rows(rng, n, width), f64(-0.3)
            for ar in (False, True):
                for grad in (False, True):
                    out, g = kernels.dm_prior_wide(c, f, h, train_ar=ar, want_grad=grad)
                    put("dm_prior_wide/w%d/n%d/ar%d/grad%d" % (width, n, ar, grad), out, *([g] if grad else []))
        for n in sizes["eval"]:
            rng = np.random.default_rng(n + width + 1)
            t, tr, f = counts(rng, n, width), counts(rng, n, width, 0.3), rows(rng, n, width)
            put("eval_wide/w%d/n%d" % (width, n), kernels.evaluate_wide(t, f, [0.5, 2.0, 30.0], [0.1, 1.0], train=tr, noise_seed=3))
        for n in sizes["ref"]:
            rng = np.random.default_rng(n + width + 2)
            c, rf, theta = counts(rng, n, width), counts(rng, n, width, 0.2, 9.0), f64(*POINT)
            for ar in (False, True):
                packed = torch.zeros(4, dtype=torch.float64, device="cuda")
                kernels.ref_train_reduce_wide(c, rf, theta, packed, train_ar=ar)
                put("dm_ref_wide/w%d/n%d/ar%d" % (width, n, ar), kernels.dm_ref_wide(c, rf, *POINT, train_ar=ar))
                put("ref_train_reduce_wide/w%d/n%d/ar%d" % (width, n, ar), packed)
        for n in sizes["mix"]:
            rng = np.random.default_rng(n + width + 3)
            c, rf, g = counts(rng, n, width), counts(rng, n, width, 0.2, 9.0), rows(rng, n, width)
            for ar in (False, True):
                put("dm_refmix_wide_grad/w%d/n%d/ar%d" % (width, n, ar),
                    *kernels.dm_refmix_wide_dev(c, g, rf, f64(POINT[0]), f64(POINT[1]), f64(POINT[2]), train_ar=ar))


def linear_kernels(cus):
    # the last size is beyond the grid of the forward kernel (and so of the backward kernel and the fused step, whose tiles are smaller)
    assert LINEAR_FWD_PER_CU * LINEAR_FWD_TILE >= kernels.LINEAR_STEP_WIDE_BLOCKS_PER_CU * kernels.LINEAR_STEP_WIDE_TILE
    for lag, n in ((1, 1), (3, 129), (5, 70), (16, 257),
                   (5, beyond(cus, kernels.LINEAR_STEP_WIDE_BLOCKS_PER_CU, kernels.LINEAR_STEP_WIDE_TILE)),
                   (5, beyond(cus, LINEAR_FWD_PER_CU, LINEAR_FWD_TILE))):
        rng = np.random.default_rng(1000 * lag + n)
        cd, c, q = codes(rng, n, lag), counts(rng, n, 21), rows(rng, n, 21)
        mat = torch.from_numpy(rng.normal(size=(lag, 21, 21))).cuda()
        f = kernels.linear_forward_wide(cd, mat, lag)
        put("linear_forward_wide/lag%d/n%d" % (lag, n), f)
        put("linear_backward_wide/lag%d/n%d" % (lag, n), kernels.linear_backward_wide(cd, lag, f, q - 0.3))
        theta = torch.cat([f64(-0.3), mat.reshape(-1)])
        for ar in (False, True):
            put("dm_linear_wide/lag%d/n%d/ar%d" % (lag, n, ar), *kernels.dm_linear_wide(c, cd, mat, -0.3, train_ar=ar))
            packed = torch.zeros(theta.numel() + 1, dtype=torch.float64, device="cuda")
            kernels.net_linear_train_reduce_wide(c, cd, lag, theta, packed, train_ar=ar)
            put("net_linear_train_reduce_wide/lag%d/n%d/ar%d" % (lag, n, ar), packed)


def cnn_kernels(cus):
    for lag, fw, n in ((5, 3, 65), (16, 16, 257), (16, 1, 130), (5, 3, beyond(cus, CNN_BWD_PER_CU, CNN_BWD_TILE)),
                       (5, 3, beyond(cus, CNN_FWD_PER_CU, CNN_FWD_TILE))):          # beyond the grid of either kernel
        rng = np.random.default_rng(100 * lag + fw + n)
        cd, q = codes(rng, n, lag), rows(rng, n, 21)
        params = torch.from_numpy(rng.normal(size=kernels.cnn_param_count_wide(lag, fw)) * 0.3).cuda()
        f, t1 = kernels.cnn_forward_wide(cd, params, lag, fw)
        put("cnn_forward_wide/lag%d/fw%d/n%d" % (lag, fw, n), f, t1)
        put("cnn_backward_wide/lag%d/fw%d/n%d" % (lag, fw, n), kernels.cnn_backward_wide(cd, params, lag, fw, t1, f, q - 0.3))
        # the fused step (drawn after everything above: the entries above keep their inputs); the last size is beyond its head
        # kernel's grid too (one block of CNN_STEP_WIDE_TILE per CU)
        assert CNN_FWD_PER_CU * CNN_FWD_TILE >= kernels.CNN_STEP_WIDE_BLOCKS_PER_CU * kernels.CNN_STEP_WIDE_TILE
        c = counts(rng, n, 21)
        theta = torch.cat([f64(-0.3), params])
        for ar in (False, True):
            bufs = kernels.cnn_step_buffers_wide(n, "cuda")
            put("dm_cnn_wide/lag%d/fw%d/n%d/ar%d" % (lag, fw, n, ar), *kernels.dm_cnn_wide(c, cd, params, lag, fw, -0.3, train_ar=ar, bufs=bufs))
            put("dm_cnn_wide/lag%d/fw%d/n%d/ar%d/bufs" % (lag, fw, n, ar), *bufs)
            packed = torch.zeros(theta.numel() + 1, dtype=torch.float64, device="cuda")
            kernels.net_cnn_train_reduce_wide(c, cd, lag, fw, theta, bufs, packed, train_ar=ar)
            put("net_cnn_train_reduce_wide/lag%d/fw%d/n%d/ar%d" % (lag, fw, n, ar), packed)


def codes5(rng, n, lag, in_kmer_order):
    """Packed contexts over ACGT with start symbols and unknown letters mixed in; in k-mer order with duplicates, or in random order."""
    if in_kmer_order:
        pool = rng.integers(0, 4, (max(1, (n + 2) // 3), lag)).astype(np.int8)
        c = pool[rng.integers(0, pool.shape[0], n)]
    else:
        c = rng.integers(0, 4, (n, lag)).astype(np.int8)
    c[rng.random(n) < 0.1, 0] = 4                        # '[' at a sequence start
    c[rng.random((n, lag)) < 0.03] = -1                  # unknown letters
    if in_kmer_order:
        key = np.zeros(n, np.int64)
        for l in range(lag):
            key = key * 6 + np.where(c[:, l] >= 0, c[:, l], 5)
        c = c[np.argsort(key, kind="stable")]
    return kernels.pack_kmers(torch.from_numpy(np.ascontiguousarray(c)).cuda())


def cnn5_pass(name, packed, lag, fw, rng, det, forms=("parts", "ctx64")):
    n = packed.shape[0]
    params = torch.from_numpy(rng.normal(size=kernels.cnn_param_count(lag, fw)) * 0.3).cuda()
    f, t1 = kernels.cnn_forward(packed, params, lag, fw)
    put("cnn_forward/" + name, f, t1)
    if det:
        g = rows(rng, n, 5) - 0.3
        for form in forms:
            if form == "ctx64":
                os.environ["BEAR_CNN_BACKWARD"] = "1"
            try:
                put("cnn_backward/%s/%s" % (form, name), kernels.cnn_backward(packed, params, lag, fw, t1, f, g))
            finally:
                os.environ.pop("BEAR_CNN_BACKWARD", None)


def cnn5_step(lag, fw, n, det):
    """The training step over prefix levels and window tables (the tables of test_cnn_step_over_window_tables_equals_the_plain_kernels)."""
    dev = torch.device("cuda", 0)
    gen = torch.Generator(dev).manual_seed(lag * 131 + fw)
    codes = torch.randint(0, 4, (n, lag), dtype=torch.int8, device=dev, generator=gen)
    odd = torch.randperm(n, device=dev, generator=gen)[:max(2, n // 150)]
    codes[odd[::2], 0] = 4
    codes[odd[1::2], torch.randint(0, lag, (odd[1::2].numel(),), device=dev, generator=gen)] = -1
    key = torch.zeros(n, dtype=torch.int64, device=dev)
    for l in range(lag):
        c = codes[:, l].to(torch.int64)
        key = key * 6 + torch.where(c >= 0, c, torch.full_like(c, 5))
    packed = kernels.pack_kmers(codes[torch.argsort(key, stable=True)].contiguous())
    counts = kernels.synth_counts(11, 0, n, dev, want=("train",))["train"]
    counts[:, 4] += (counts == 0).all(dim=1).to(counts.dtype)
    flat = torch.from_numpy(np.random.default_rng(lag * 100 + fw).normal(size=kernels.cnn_param_count(lag, fw)) * 0.3).cuda()
    theta = torch.cat([f64(0.2), flat]).contiguous()
    plan = kernels.Plan(counts, 5)
    bufs = kernels.cnn_step_buffers(n, lag, fw, dev, ws=plan.ws)
    plan.attach_cnn_levels(packed, lag, fw)
    (level_rows, letters), tables = plan.cnn_level_rows(with_letters=True), plan.cnn_window_rows()
    own_hi = lag - fw + 1 - sum(1 for lev, _, _ in tables if lev == 0)
    own_lo = letters[0] - fw + 1 if letters else 0
    name = "lag%d/fw%d/n%d" % (lag, fw, n)
    OUT["cnn_step/%s/shape" % name] = "levels %s tables %s head-only %s" % (level_rows, tables, own_lo >= own_hi)
    for ar in (False, True):
        pk = torch.zeros(2 + flat.numel(), dtype=torch.float64, device=dev)
        kernels.net_cnn_train_reduce(plan, packed, lag, fw, theta, bufs, pk, train_ar=ar)
        put("cnn_step/%s/ar%d/bufs" % (name, ar), *bufs)
        if det:
            put("cnn_step/%s/ar%d/packed" % (name, ar), pk)
    put("cnn_forward_plan/" + name, *kernels.cnn_forward(packed, flat, lag, fw, plan=plan))


def cnn5_kernels(cus, det):
    for lag, fw, n in ((1, 1, 1), (2, 1, 3), (13, 8, 31), (13, 8, 33), (13, 8, 63), (13, 8, 65), (7, 7, 64),
                       (21, 21, 130),                    # the window mask is 63 bits wide
                       (21, 16, 200)):                   # only the 64-context form of the backward kernel fits
        for order in ("random", "kmer"):
            rng = np.random.default_rng(10000 * lag + 100 * fw + n + (order == "kmer"))
            cnn5_pass("lag%d/fw%d/n%d/%s" % (lag, fw, n, order), codes5(rng, n, lag, order == "kmer"), lag, fw, rng, det)
    # more groups than the grid has waves: every wave a range of two or more groups, the last one ragged
    n_fwd = beyond(cus, CNN5_FWD_WAVES_PER_CU, CNN5_FWD_TILE)
    rng = np.random.default_rng(n_fwd)
    packed = codes5(rng, n_fwd, 13, True)
    params = torch.from_numpy(rng.normal(size=kernels.cnn_param_count(13, 8)) * 0.3).cuda()
    put("cnn_forward/beyond/n%d" % n_fwd, *kernels.cnn_forward(packed, params, 13, 8))
    n_parts = beyond(cus, CNN5_PARTS_WAVES_PER_CU, CNN5_PARTS_TILE)
    rng = np.random.default_rng(n_parts)
    cnn5_pass("beyond/n%d" % n_parts, codes5(rng, n_parts, 13, True), 13, 8, rng, det, forms=("parts",))
    for lag, fw, n in ((7, 3, 50_000), (8, 2, 100_000), (7, 3, beyond(cus, CNN5_HEAD_WAVES_PER_CU, CNN5_PARTS_TILE))):
        cnn5_step(lag, fw, n, det)


def codes5_prefixes(rng, n, lag):
    """K-mer order; the first 70 % of the rows on a few prefixes (runs of many contexts that share all but the last three letters),
    one row in 33 of them random; the rest random behind a first letter of their own, so that at the long lags the table ends in a
    stretch of runs of one context, whose tiles keep their plain lists (the construction of test_fused_linear_head_paired_contexts,
    plus that stretch)."""
    lead = max(lag - 3, 0)
    c = rng.integers(0, 4, (n, lag)).astype(np.int8)
    head = n - (3 * n) // 10
    pre = rng.integers(0, 3, (max(1, n // 40), lead)).astype(np.int8)
    keep = rng.random(head) >= 1.0 / 33.0
    c[:head][keep, :lead] = pre[rng.integers(0, pre.shape[0], int(keep.sum()))]
    if lead:
        c[:head, 0] = np.minimum(c[:head, 0], 2)
        c[head:, 0] = 3
    c[rng.random(n) < 0.02, 0] = 4                       # '[' at a sequence start
    c[rng.random((n, lag)) < 0.01] = -1                  # unknown letters
    key = np.zeros(n, np.int64)
    for l in range(lag):
        key = key * 6 + np.where(c[:, l] >= 0, c[:, l], 5)
    return kernels.pack_kmers(torch.from_numpy(np.ascontiguousarray(c[np.argsort(key, kind="stable")])).cuda())


def counts5(rng, n):
    """Four contexts in five with counts, in one cell or two: tiles of the full 1664 rows (a denser table is cut into shorter
    tiles by its items) whose lists of contexts with counts are long enough that a stretch of runs of one context does not fit
    the paired form."""
    c = np.zeros((n, 5), np.uint32)
    rows = np.arange(n)
    live = rng.random(n) < 0.8
    c[rows[live], rng.integers(0, 5, n)[live]] = rng.poisson(6.0, int(live.sum())) + 1
    two = live & (rng.random(n) < 0.15)
    c[rows[two], rng.integers(0, 5, n)[two]] += rng.poisson(3.0, int(two.sum())).astype(np.uint32)
    if n == 1:
        c[0, 1] = 3
    return torch.from_numpy(c.view(np.int32)).cuda()


def linear5_mats(rng, lag):
    """Parameters for tables of exponentials, for tables of logits (plain softmax) and for a saturated softmax (the shifted form)."""
    mats = {}
    for scale in (0.4, 150.0, 3000.0):
        m = rng.normal(size=(lag, 5, 5)) * scale
        if scale > 1:
            m[0, 0] *= 0.001                             # contexts starting with letter 0 keep small logits from that position
        mats["m%g" % scale] = torch.from_numpy(m).cuda()
    return mats


def linear5_steps(name, plan, idx, lag, mats, det):
    """The step over the plan's plain lists, then -- where pairing takes -- over its paired lists."""
    for form in ("plain", "paired"):
        if form == "paired":
            took = plan.pair_contexts(idx, lag)
            n_paired, n_plain = plan.pair_info()
            assert n_paired + n_plain == len(plan.tiles()[0]) and (n_paired >= 1) == took
            OUT["dm_linear/%s/shape" % name] = "tiles paired %d plain %d" % (n_paired, n_plain) if took else "pairing declined"
            if not took:
                return
        for generic in (0, 1):
            if generic:
                os.environ["BEAR_AMD_LINEAR_GENERIC"] = "1"
            try:
                for ar in (False, True):
                    for mname, mat in mats.items():
                        out, grad = kernels.dm_linear(plan, idx, mat, 0.3 if ar else 0.2, train_ar=ar)
                        case = "dm_linear/%s/%s/generic%d/ar%d/%s" % (name, form, generic, ar, mname)
                        put(case + "/grad_mat", grad)
                        if det:
                            put(case + "/out", out)
            finally:
                os.environ.pop("BEAR_AMD_LINEAR_GENERIC", None)


def linear5_kernels(cus, det):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests"))
    from util import mixed_heavy_table                   # (NumPy only)
    before = os.environ.get("BEAR_AMD_DETERMINISTIC")
    os.environ["BEAR_AMD_DETERMINISTIC"] = "1"
    try:
        for n in (1, 3 * LINEAR5_TILE + 77, beyond(cus, LINEAR5_PER_CU, LINEAR5_TILE)):
            for lag in (1, 3, 5, 9, 13, 14, 21):
                rng = np.random.default_rng(100 * n + lag)
                c = counts5(rng, n)
                mats = linear5_mats(rng, lag)
                for table, packed in (("twins", codes5(rng, n, lag, True)), ("prefixes", codes5_prefixes(rng, n, lag)),
                                      ("random", codes5(rng, n, lag, False))):
                    linear5_steps("n%d/lag%d/%s" % (n, lag, table), kernels.Plan(c, 5), kernels.linear_index(packed, lag), lag, mats, det)
        # tiles denser than their in-tile lists: the plan's overflow items and contexts.  WHICH large-count cells of such a tile
        # stay inside it is decided by atomic counters when libbear_hip.so builds the plan, and an overflow item's part of its
        # context's gradient is rounded to fixed point on its own: the same bits from plan to plan in libbear_hip_det.so only
        if not det:
            return
        heavy = mixed_heavy_table()[0]
        c = torch.from_numpy(np.ascontiguousarray(heavy).view(np.int32)).cuda()
        for lag in (5, 13):
            rng = np.random.default_rng(7000 + lag)
            mats = linear5_mats(rng, lag)
            packed = codes5(rng, c.shape[0], lag, True)
            linear5_steps("mixed_heavy/lag%d" % lag, kernels.Plan(c, 5), kernels.linear_index(packed, lag), lag, mats, det)
    finally:
        if before is None:
            os.environ.pop("BEAR_AMD_DETERMINISTIC", None)
        else:
            os.environ["BEAR_AMD_DETERMINISTIC"] = before


def exact_text(rng, K, width):
    """-> (rows int32, letters uint8, seg int64, weights int8) on the device, and the host rows / letters / offsets."""
    n_short, n_long = 3 * 256 + 77, 2 * kernels.MARG_CHUNK + 5
    offsets = np.array([0, 100, 100, 400, n_short, n_short + n_long], dtype=np.int64)
    r = rng.integers(0, K, n_short + n_long).astype(np.int32)
    l = rng.integers(0, width, n_short + n_long).astype(np.uint8)
    r[n_short + 300:n_short + 450], l[n_short + 300:n_short + 450] = 5, 2      # a run longer than a wave
    l[::17] = kernels.SCORE_SKIP
    r[3::29] = -1
    r[11::31] = K + 3
    w = np.where(rng.random(r.size) < 0.4, -1, 1).astype(np.int8)
    return [torch.from_numpy(x).cuda() for x in (r, l, offsets, w)], (r, l, offsets)


def exact_kernels(cus):
    hs, vs = [0.5, 2.0], [0.1, 1.0]
    for width in kernels.WIDE_WIDTHS:
        K = 37
        rng = np.random.default_rng(4200 + width)
        (r, l, seg, wts), (hr, hl, offsets) = exact_text(rng, K, width)
        prior = rows(rng, K, width)
        name = "w%d" % width
        put("score_marg/" + name, kernels.score_marg(r, l, seg, counts(rng, K, width, 0.5), prior, hs, vs))
        train = counts(rng, K, width, 0.5)
        put("score_moments/%s/weights0" % name, kernels.score_moments(r, l, seg, train, prior, hs, vs))
        put("score_moments/%s/weights1" % name, kernels.score_moments(r, l, seg, train, prior, hs, vs, weights=wts))
        for G in (1, 3):
            table = counts(rng, K * G, width, 0.5).cpu().numpy().view(np.uint32).reshape(K, G, width)
            own = np.array([G - 1, G // 2, -1, G, 0], dtype=np.int32)       # the long segment: group 0, which does not hold it
            for s in (0, 1, 3):
                if 0 <= own[s] < G:
                    a, b = offsets[s], offsets[s + 1]
                    live = (hr[a:b] >= 0) & (hr[a:b] < K) & (hl[a:b] < width)
                    np.add.at(table[:, own[s], :], (hr[a:b][live], hl[a:b][live]), 1)
            table = torch.from_numpy(np.ascontiguousarray(table).view(np.int32)).cuda()
            put("score_groups/%s/G%d/own0" % (name, G), *kernels.score_groups(r, l, seg, table, prior, hs, vs))
            scores, short_of = kernels.score_groups(r, l, seg, table, prior, hs, vs, own=torch.from_numpy(own).cuda())
            assert short_of.cpu().tolist() == [0, 0, 0, 0, 1] and bool(scores[4, 0].isnan().all()), "the long segment alone is short"
            put("score_groups/%s/G%d/own1" % (name, G), scores, short_of)
        models = {"m4": ([0.5, 2.0], [0.1, 1.0]), "m5": ([0.05, 0.7, 3.0], [0.1, 1.0])}         # m5: two launches
        tile = kernels.TWO_SAMPLE_TILE[width]
        for n in (tile - 1, tile + 1, beyond(cus, kernels.TWO_SAMPLE_BLOCKS_PER_CU, tile)):
            rng = np.random.default_rng(n + width + 4)
            a, b, f = counts(rng, n, width), counts(rng, n, width, 0.2), rows(rng, n, width)
            for mname, (h, v) in models.items():
                for more in (False, True):
                    out = kernels.two_sample(a, b, f, h, v, want_ar=more, want_rows=more)
                    put("two_sample/%s/n%d/%s/more%d" % (name, n, mname, more), *[t for t in out if t is not None])
        for G in (2, 3, 16):
            tile = kernels.k_sample_tile(width, G)
            cols = [int(c) for c in np.random.default_rng(G).permutation(18)[:G]]
            for n in (tile - 1, tile + 1, beyond(cus, kernels.K_SAMPLE_BLOCKS_PER_CU, tile)):
                rng = np.random.default_rng(n + width + G + 5)
                table, f = counts(rng, 18 * n, width).reshape(18, n, width), rows(rng, n, width)
                for mname, (h, v) in models.items():
                    for more in (False, True):
                        out = kernels.k_sample(table, cols, f, h, v, want_ar=more, want_rows=more)
                        put("k_sample/%s/G%d/n%d/%s/more%d" % (name, G, n, mname, more), *[t for t in out if t is not None])


if __name__ == "__main__":
    from bear_amd import _lib
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    det = os.path.basename(_lib.LIB_PATH) == "libbear_hip_det.so"
    sections = {"row_kernels": lambda: row_kernels(cus), "linear_kernels": lambda: linear_kernels(cus), "cnn_kernels": lambda: cnn_kernels(cus),
                "cnn5_kernels": lambda: cnn5_kernels(cus, det), "linear5_kernels": lambda: linear5_kernels(cus, det),
                "exact_kernels": lambda: exact_kernels(cus)}
    unknown = [a for a in sys.argv[1:] if a not in sections]
    if unknown:
        sys.exit("no section %s: %s" % (unknown, list(sections)))
    for name, run in sections.items():
        if name in sys.argv[1:] or not sys.argv[1:]:
            run()
    torch.cuda.synchronize()
    print(json.dumps(OUT, indent=0, sort_keys=True))
