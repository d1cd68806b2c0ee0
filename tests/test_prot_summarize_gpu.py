"""GPU tests of the 21-wide device summarize path: protein count tables from residue sequences (bear_kmer_sort_create_wide +
the summarize host mirror with alphabet='prot') against a dictionary counter written here, the width-5 twin against the 4-letter
entry, conservation and folding at scale, the files summarize writes, training from a device-resident protein table, and variant
scoring through the sequence counter.  Counts are bit exact."""
import ctypes
import types

import numpy as np
import pytest

from test_prot_cpu import PROT

pytestmark = pytest.mark.gpu

KEY_LETTERS = PROT + "["                  # 5-bit codes of a context: residues 0..19, '[' = 20
COLS = {ch: i for i, ch in enumerate(PROT + "]")}


def dict_count(seqs, groups, lag, n_groups):
    """The rule of the reference's test (tests/test_summarize.py:88-115) over the protein alphabet: full = '[' * L + seq + ']',
    counts[full[j-L:j]][group][full[j]] += 1; a window (context + next letter) holding a character outside the 20 residues is
    dropped.  -> {context: int64 [n_groups, 21]}"""
    ok = set(PROT + "[]")
    out = {}
    for s, g in zip(seqs, groups):
        full = "[" * lag + s.upper() + "]"
        for j in range(lag, len(full)):
            win = full[j - lag:j + 1]
            if all(c in ok for c in win):
                out.setdefault(win[:lag], np.zeros((n_groups, 21), dtype=np.int64))[g, COLS[win[lag]]] += 1
    return out


def keys_of(kmers):
    """The 5-bit sort key recomputed from ASCII k-mers uint8 [n, lag]: letter l in bits [5l, 5l + 5)."""
    lut = np.full(256, 255, dtype=np.uint64)
    for i, ch in enumerate(KEY_LETTERS):
        lut[ord(ch)] = i
    codes = lut[kmers]
    assert codes.max(initial=0) <= 20
    return (codes << (5 * np.arange(kmers.shape[1], dtype=np.uint64))).sum(axis=1, dtype=np.uint64)


def random_protein(rng, n):
    return "".join(rng.choice(list(PROT), size=int(n)))


def test_exact_counts_against_dictionary_counter():
    from bear_amd import _lib, summarize
    rng = np.random.default_rng(0)
    seqs = [random_protein(rng, n) for n in rng.integers(1, 300, size=300)]
    seqs += ["A", "MK", "", "XBZUOJ-", "X", "MKVXLAARND", "ARNDBCEQGHILKZ", "mkvlaarnd", "WYVWYVWYVWYVWYVW*YVWYV"]
    for i in (3, 50, 120):                                  # invalid residues inside long sequences
        s = seqs[i] + random_protein(rng, 40)
        seqs[i] = s[:len(s) // 2] + "X" + s[len(s) // 2:]
    groups = [int(g) for g in rng.integers(0, 4, size=len(seqs))]
    text, grp = summarize.encode_sequences(seqs, groups, alphabet="prot")
    for lag in (1, 2, 5, 8, 12):
        kmers, counts = summarize.count_transitions(text, grp, lag, 4, alphabet="prot")
        assert kmers.shape == (counts.shape[1], lag) and counts.shape[0] == 4 and counts.shape[2] == 21 and counts.dtype == np.uint32
        want = dict_count(seqs, groups, lag, 4)
        got = {bytes(k).decode(): counts[:, i].astype(np.int64) for i, k in enumerate(kmers)}
        assert len(got) == kmers.shape[0] and set(got) == set(want), lag
        for k in want:
            assert np.array_equal(got[k], want[k]), (lag, k)
        keys = keys_of(kmers)
        assert np.all(keys[1:] > keys[:-1]), lag             # strictly ascending in the 5-bit key
    # totals: one transition per residue plus one stop per clean sequence
    clean = [(s, g) for s, g in zip(seqs, groups) if all(c in PROT for c in s.upper())]
    kmers, counts = summarize.count_transitions(*summarize.encode_sequences([s for s, _ in clean], [g for _, g in clean], alphabet="prot"),
                                                3, 4, alphabet="prot")
    assert int(counts.sum()) == sum(len(s) + 1 for s, _ in clean)
    assert int(counts[..., 20].sum()) == len(clean)
    # the packed 3-bit k-mer code does not exist at width 21
    import torch
    L = _lib.lib()
    t, g = torch.from_numpy(text).cuda(), torch.from_numpy(grp).cuda()
    h, n_rows = ctypes.c_void_p(), ctypes.c_uint64()
    assert L.bear_kmer_sort_create_wide(t.data_ptr(), g.data_ptr(), t.numel(), 3, 21, ctypes.byref(h), ctypes.byref(n_rows), None) == 0
    try:
        code = torch.zeros(n_rows.value, dtype=torch.int64, device="cuda")
        cn = torch.zeros((4, n_rows.value, 21), dtype=torch.int32, device="cuda")
        assert L.bear_kmer_sort_reduce(h, 4, None, code.data_ptr(), cn.data_ptr(), None) == -1
        assert L.bear_kmer_sort_reduce(h, 4, None, None, cn.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert int(cn.sum()) == sum(int(v.sum()) for v in dict_count(seqs, groups, 3, 4).values())
    finally:
        L.bear_kmer_sort_destroy(h)


def test_width_5_twin_is_bit_identical_to_the_dna_entry():
    """The DNA inputs of test_summarize_gpu.test_random_sequences_many_bins_and_invalid_letters through both entries."""
    import torch
    from bear_amd import _lib, summarize
    rng = np.random.default_rng(0)
    seqs = ["".join(rng.choice(list("ACGT"), size=int(n))) for n in rng.integers(1, 400, size=300)]
    seqs += ["A", "", "ACGTNACGT", "NNNN"]
    groups = [int(g) for g in rng.integers(0, 4, size=len(seqs))]
    text, grp = summarize.encode_sequences(seqs, groups)
    t, g = torch.from_numpy(text).cuda(), torch.from_numpy(grp).cuda()
    L = _lib.lib()

    def run(lag, wide):
        h, n_rows = ctypes.c_void_p(), ctypes.c_uint64()
        if wide:
            st = L.bear_kmer_sort_create_wide(t.data_ptr(), g.data_ptr(), t.numel(), lag, 5, ctypes.byref(h), ctypes.byref(n_rows), None)
        else:
            st = L.bear_kmer_sort_create(t.data_ptr(), g.data_ptr(), t.numel(), lag, ctypes.byref(h), ctypes.byref(n_rows), None)
        assert st == 0
        try:
            n = n_rows.value
            km = torch.zeros((n, lag), dtype=torch.uint8, device="cuda")
            code = torch.zeros(n, dtype=torch.int64, device="cuda")
            cn = torch.zeros((4, n, 5), dtype=torch.int32, device="cuda")
            assert L.bear_kmer_sort_reduce(h, 4, km.data_ptr(), code.data_ptr(), cn.data_ptr(), None) == 0
            torch.cuda.synchronize()
        finally:
            L.bear_kmer_sort_destroy(h)
        return km.cpu().numpy(), code.cpu().numpy(), cn.cpu().numpy()
    for lag in (1, 5, 13, 21):
        a, b = run(lag, False), run(lag, True)
        assert a[0].shape[0] > 0
        for x, y in zip(a, b):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), lag


def _device_text(reads, rl, n_groups, seed):
    """`reads` sequences of `rl` uniform residues each as the 21-wide code text, made on the device."""
    import torch
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(seed)
    body = torch.randint(0, 20, (reads, rl), dtype=torch.uint8, device=dev, generator=gen)
    text = torch.cat([torch.full((reads, 1), 21, dtype=torch.uint8, device=dev), body,
                      torch.full((reads, 1), 20, dtype=torch.uint8, device=dev)], 1).reshape(-1).contiguous()
    grp = (torch.arange(reads, device=dev) % n_groups).to(torch.uint8).repeat_interleave(rl + 2).contiguous()
    return text, grp


def test_full_size_count_conservation_prot():
    """1e7 positions in 3 groups at lag 5: every residue and every stop is exactly one transition, rows are distinct, and the
    lag-5 table folds onto the lag-2 table (marginalising the 3 leading letters preserves each 2-mer's counts).  Lag 12 on 2e6
    positions, where nearly every context is distinct: conservation and distinctness.  Host copies: 3 x 3.2e6 x 21 x 4 B = 0.8 GB
    at lag 5, 0.17 GB at lag 12."""
    from bear_amd import summarize
    reads, rl = 33_000, 300
    text, grp = _device_text(reads, rl, 3, 3)
    assert text.numel() == reads * (rl + 2)
    k5, c5 = summarize.count_transitions(text, grp, 5, 3, alphabet="prot")
    k2, c2 = summarize.count_transitions(text, grp, 2, 3, alphabet="prot")
    assert c5.shape == (3, k5.shape[0], 21)
    assert int(c5.sum(dtype=np.uint64)) == int(c2.sum(dtype=np.uint64)) == reads * (rl + 1)
    per_group = np.bincount(np.arange(reads) % 3, minlength=3) * (rl + 1)
    assert np.array_equal(c5.sum(axis=(1, 2), dtype=np.int64), per_group) and np.array_equal(c2.sum(axis=(1, 2), dtype=np.int64), per_group)
    assert int(c5[..., 20].sum()) == reads                        # one stop per sequence
    key5, key2 = keys_of(k5), keys_of(k2)
    assert np.all(key5[1:] > key5[:-1]) and np.all(key2[1:] > key2[:-1])       # ascending and distinct
    # fold: the last 2 letters of every 5-mer context
    suf = keys_of(k5[:, 3:])
    order = np.argsort(suf, kind="stable")
    uk, start = np.unique(suf[order], return_index=True)
    folded = np.add.reduceat(c5[:, order].astype(np.int64), start, axis=1)
    assert np.array_equal(uk, key2) and np.array_equal(folded, c2.astype(np.int64))
    del k5, c5, folded
    reads12 = 6_600
    text, grp = _device_text(reads12, rl, 1, 4)
    k12, c12 = summarize.count_transitions(text, grp, 12, 1, alphabet="prot")
    assert c12.shape == (1, k12.shape[0], 21) and int(c12.sum(dtype=np.uint64)) == reads12 * (rl + 1)
    key12 = keys_of(k12)
    assert np.all(key12[1:] > key12[:-1])
    assert k12.shape[0] > 0.9 * reads12 * (rl + 1)                # nearly every context is distinct


def _two_fastas(tmp_path, rng, n=60):
    paths = []
    for f in range(2):
        fa = tmp_path / f"p{f}.fa"
        with open(fa, "w") as fh:
            for i, m in enumerate(rng.integers(20, 180, size=n)):
                s = random_protein(rng, m)
                if i % 9 == 0:
                    s = s[:7] + "X" + s[7:]                  # a residue outside the 20
                if i % 5 == 0:
                    s += "*"                                 # an explicit stop
                if i % 7 == 0:
                    s = s.lower()
                fh.write(f">s{f}_{i}\n" + "\n".join(s[a:a + 60] for a in range(0, len(s), 60)) + "\n")
        paths.append(fa)
    lst = tmp_path / "list.csv"
    lst.write_text(f"{paths[0]},0,fa\n{paths[1]},1,fa\n")
    return str(lst)


def test_summarize_main_writes_protein_tables(tmp_path):
    from bear_amd import dataloader, summarize
    lst = _two_fastas(tmp_path, np.random.default_rng(11))
    max_lag = 3
    tables = summarize.count_tables(lst, max_lag, alphabet="prot")
    assert [t.alphabet for t in tables] == ["prot"] * max_lag and all(t.width == 21 and t.num_ds == 2 for t in tables)
    seqs, groups = summarize._load_sequences(lst)
    for li, t in enumerate(tables):                               # the tables themselves, against the dictionary counter
        want = dict_count([s[:-1] if s.endswith("*") else s for s in seqs], groups, li + 1, 2)
        got = {bytes(k).decode(): t.counts[:, i].astype(np.int64) for i, k in enumerate(t.kmers)}
        assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)
    args = types.SimpleNamespace(file=lst, out_prefix=str(tmp_path / "out"), l=max_lag, nf=False, r=False, mf=1e-4, a="prot")
    n_bins, n_bins_rev = summarize.main(args)
    assert n_bins > 1 and n_bins_rev is None
    for li, t in enumerate(tables):
        parts = [dataloader.dataloader(f"{tmp_path / 'out'}_lag_{li + 1}_file_{b}.tsv", "prot", 1000, 2) for b in range(n_bins)]
        assert all(p.alphabet == "prot" and p.width == 21 for p in parts)
        for b, p in enumerate(parts):                             # rows are dealt round-robin to the bins
            assert np.array_equal(p.kmers, t.kmers[b::n_bins]) and np.array_equal(p.counts, t.counts[:, b::n_bins])
        assert sum(p.num_rows for p in parts) == t.num_rows


def test_device_resident_protein_tables_train_like_host_tables(tmp_path):
    """count -> (shuffle) -> train without the table leaving HBM: same losses as the host-table path (the tolerances of
    test_summarize_gpu.test_device_resident_tables_train_like_host_tables)."""
    import torch
    from bear_amd import ar_funcs, bear_net, core, kernels, summarize
    lst = _two_fastas(tmp_path, np.random.default_rng(5), n=100)
    lag = 3
    host = summarize.count_tables(lst, lag, alphabet="prot")[lag - 1]
    dev = summarize.count_tables(lst, lag, alphabet="prot", on_device=True)[lag - 1]
    assert dev.alphabet == "prot" and dev.width == 21 and dev.kmers_dev.is_cuda and dev.counts_dev.is_cuda
    assert dev.num_rows == host.num_rows and np.array_equal(dev.counts, host.counts) and np.array_equal(dev.kmers, host.kmers)
    # the device twin of core.encode_kmers: the table's k-mers, and every byte value
    assert np.array_equal(kernels.encode_kmers(dev.kmers_dev, "prot").cpu().numpy(), core.encode_kmers(host.kmers, "prot"))
    every = np.arange(256, dtype=np.uint8).reshape(64, 4)
    assert np.array_equal(kernels.encode_kmers(torch.from_numpy(every).cuda(), "prot").cpu().numpy(), core.encode_kmers(every, "prot"))
    losses = []
    for data in (host, dev, host.shuffle(3), dev.shuffle(3)):
        torch.manual_seed(0)
        ls = []
        bear_net.train(data.repeat(2), data.num_rows, 2, 0, "prot", lag, ar_funcs.make_ar_func_linear, {}, 0.01, "Adam", False, loss_save=ls)
        losses.append(ls)
    assert len(losses[0]) == 2 and np.all(np.isfinite(losses[0]))
    assert np.allclose(losses[0], losses[1], rtol=1e-13) and np.allclose(losses[2], losses[3], rtol=1e-13)
    assert np.isclose(losses[0][0], losses[2][0], rtol=1e-11)       # one batch = the whole table: order does not matter


def test_variant_scores_counter_equals_table_scan(tmp_path):
    """get_bear_probs on protein variants: counts looked up through make_sequence_counter against a scan of the table summarize
    wrote from the same sequences.  MAP with vanilla (BMM) models is closed form -- log((van + c_b) / (21 van + sum c)) per
    transition -- and both paths feed it the same integer counts; what may differ is the order in which a score's terms are added
    (the scan adds batch by batch).  A score is a sum of fewer than 100 such logs, each below 10 in magnitude: differences stay
    below 100 * 10 * 2.2e-16 < 1e-12."""
    from bear_amd import dataloader, get_var_probs, summarize
    rng = np.random.default_rng(21)
    lag = 3
    seqs = [random_protein(rng, n) for n in rng.integers(30, 80, size=40)] + ["MKXLV", "arndc*"]
    fa = tmp_path / "train.fa"
    fa.write_text("".join(f">t{i}\n{s}\n" for i, s in enumerate(seqs)))
    lst = tmp_path / "list.csv"
    lst.write_text(f"{fa},0,fa\n")
    args = types.SimpleNamespace(file=str(lst), out_prefix=str(tmp_path / "tab"), l=lag, nf=False, r=False, mf=0.1, a="prot")
    assert summarize.main(args) == (1, None)
    wt = seqs[0][:25]                                             # contexts the table holds ...
    variants = []
    for p in (0, 4, 11, 17, 24):                                  # ... and, through the substitutions, contexts it does not
        new = PROT[(PROT.index(wt[p]) + 7) % 20]
        variants.append(f"{wt[p]}{p}{new}")
    variants.append(f"{wt[8:10]}8{'WWW'}")
    all_kmers = get_var_probs._get_all_kmers_vars([get_var_probs.parse_var(v) for v in variants], lag * "[" + wt + "]", lag)
    data = dataloader.dataloader(f"{tmp_path / 'tab'}_lag_{lag}_file_0.tsv", "prot", 97, 1)
    in_table = {bytes(k).decode() for k in data.kmers}
    assert set(all_kmers) - in_table and set(all_kmers) & in_table
    vans = [0.1, 1.0, 10.0]
    counter = get_var_probs.make_sequence_counter(seqs, lag, reverse=False, alphabet_name="prot")
    rows = counter(np.array(sorted(in_table)[:5] + ["WWW"]))
    assert rows.shape == (6, 21) and np.array_equal(rows[:5], data.counts[0, np.argsort([bytes(k).decode() for k in data.kmers])[:5]])
    a = get_var_probs.get_bear_probs(None, wt, variants, 0, vans=vans, get_map=True, lag=lag, alphabet_name="prot", counter=counter)
    b = get_var_probs.get_bear_probs(None, wt, variants, 0, vans=vans, get_map=True, lag=lag, alphabet_name="prot", data=data)
    assert a.shape == (len(variants), len(vans)) and np.all(np.isfinite(a)) and np.any(a != 0)
    assert np.allclose(a, b, rtol=1e-12, atol=1e-12)
    # the counter from the file list, and no_end
    c = get_var_probs.get_bear_probs(None, wt, variants, 0, vans=vans, get_map=True, lag=lag, alphabet_name="prot",
                                     counter=get_var_probs.make_sequence_counter(str(lst), lag, reverse=False, alphabet_name="prot"))
    assert np.allclose(a, c, rtol=1e-12, atol=1e-12)
    ne = get_var_probs.make_sequence_counter(seqs, lag, reverse=False, no_end=True, alphabet_name="prot")
    some = np.array(sorted(in_table))
    r_ne, r_all = ne(some), counter(some)
    full = np.array(["[" not in k for k in some])
    assert np.all(r_ne[:, 20] == 0) and np.array_equal(r_ne[full, :20], r_all[full, :20]) and np.all(r_ne[~full] == 0)
