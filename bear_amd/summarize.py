"""k-mer transition count tables from sequence files: host mirror of ``bear_model/summarize.py``.

``main(args)`` / ``run(args)`` keep the reference's arguments (summarize.py:650-696: ``file`` -- a csv of
``FILE, GROUP, TYPE`` rows with TYPE ``fa`` / ``fq`` --, ``out_prefix``, ``l`` max lag, ``nf``, ``r``, ``mf``; the KMC
options ``mk``, ``p``, ``t``, ``pr``, ``s12``, ``s3`` are accepted and ignored) and write the same files,
``<out_prefix>_lag_<L>_file_<b>.tsv`` with rows ``kmer \\t [[A,C,G,T,$ of group 0],[group 1],...]``, '[' padded
(summarize.py:429-449, 472-473).  Where the reference writes prefix / suffix / full FASTQ files, runs the external KMC
counter and heap-merges its dumps (stages 1-3), this build counts on the device: the sequences are uploaded once as a
code text and every lag is one emit + radix sort + run-length reduce (``bear_kmer_sort_*``, bear_count.hip).  What is
counted is what the reference's test defines (tests/test_summarize.py:88-115).  ``count_tables`` returns the tables as
``CountDataset`` objects without writing text at all.

``alphabet='prot'`` (command line ``-a prot``) counts residues instead: the same pass with 5 bits per letter and rows of 21
counts (``bear_kmer_sort_create_wide``), for lags up to 12, without reverse complements.  The reference has no such path (KMC is
DNA-only); the rule is the same one over another alphabet.

A text beyond one device sort -- 2^32 - 1 positions or more (row indices are 32-bit), or more pairs than the about 30 B per
position of emit + sort fit next to it -- is counted in passes over ranges of the key space (``count_passes``): a histogram of
the transitions over the context's last letters (``bear_kmer_bin_hist``), a greedy cut of its bins into ranges of at most
``max_pairs`` transitions (``cut_ranges``), and one compacted emit + sort + reduce per range (``bear_kmer_sort_create_range``).
The sort order is the key order, so the slices of ascending ranges, concatenated, are the table of the single pass, row for row.
``-mk`` stays ignored (the reference's default of 12 GB would turn every default run into passes); the environment variable
``BEAR_AMD_COUNT_MAX_PAIRS`` sets ``max_pairs`` for every call that passes none.

Rows come out sorted by packed k-mer code and are dealt round-robin to the output bins (the reference assigns rows to
random bins, summarize.py:439,447, and states that the order carries no meaning, :72); shuffle before training
(``CountDataset.shuffle`` or ``shuf``) exactly as with the reference's files.
"""
import csv
import ctypes
import datetime
import os

import numpy as np
import torch

from . import _lib
from .dataloader import CountDataset, DeviceCountDataset

alphabet = {"A": 0, "C": 1, "G": 2, "T": 3, "]": 4}     # summarize.py:380

_START, _STOP, _OTHER = 5, 4, 6
_LUT = np.full(256, _OTHER, dtype=np.uint8)
for _ch, _v in (("A", 0), ("C", 1), ("G", 2), ("T", 3)):
    _LUT[ord(_ch)] = _v
_COMP = np.array([3, 2, 1, 0, 4, 5, 6], dtype=np.uint8)    # reverse complement on codes

# the protein code text: residues in the order of core.alphabets_en['prot'], stop 20, start marker 21, any other character 22
PROT_LETTERS = "ARNDCEQGHILKMFPSTWYV"
_PROT_START, _PROT_STOP, _PROT_OTHER = 21, 20, 22
_PROT_LUT = np.full(256, _PROT_OTHER, dtype=np.uint8)
for _v, _ch in enumerate(PROT_LETTERS):
    _PROT_LUT[ord(_ch)] = _v
WIDTHS = {"dna": 5, "prot": 21}
MAX_LAG = {"dna": 21, "prot": 12}       # 3 lag + 1 resp. 5 lag + 1 key bits in one uint64
BITS = {"dna": 3, "prot": 5}            # key bits per letter
BIN_LETTERS = {"dna": 6, "prot": 3}     # BEAR_COUNT_BIN_LETTERS, BEAR_COUNT_BIN_LETTERS_WIDE (include/bear_hip.h)
PAIR_LIMIT = 2 ** 32 - 1                # positions of the single pass and pairs of a counting pass stay below (32-bit row indices)


def _width(alphabet, reverse=False):
    if alphabet not in WIDTHS:
        raise ValueError(f"summarize counts the alphabets {tuple(WIDTHS)}, not {alphabet!r}")
    if alphabet == "prot" and reverse:
        raise ValueError("the protein alphabet has no reverse complement: pass reverse=False (no -r)")
    return WIDTHS[alphabet]


def _check_lag(lag, alphabet):
    """The protein limit, with its reason (the 4-letter path keeps reporting the library's status for a lag beyond 21)."""
    if alphabet == "prot" and not 1 <= int(lag) <= MAX_LAG["prot"]:
        raise ValueError(f"lag {lag}: protein tables are counted for lags 1..{MAX_LAG['prot']} "
                         "(5 bits per residue: a longer context does not fit the 64-bit sort key)")


def load_input(in_file, file_type):
    """summarize.py:96-100 (Biopython's SimpleFastaParser / FastqGeneralIterator): yields ``(name, seq)``."""
    if file_type == "fa":
        name, parts = None, []
        for line in in_file:
            line = line.rstrip("\n\r")
            if line.startswith(">"):
                if name is not None:
                    yield name, "".join(parts)
                name, parts = line[1:], []
            elif name is not None:
                parts.append(line.strip())
        if name is not None:
            yield name, "".join(parts)
    elif file_type == "fq":
        while True:
            head = in_file.readline()
            if not head:
                return
            if not head.strip():
                continue
            seq = in_file.readline().rstrip("\n\r")
            in_file.readline()
            in_file.readline()
            yield head[1:].rstrip("\n\r"), seq
    else:
        raise ValueError("file type must be 'fa' or 'fq'")


def read_file_list(seq_list_file):
    """summarize.py:252-256: rows ``FILE, GROUP, TYPE``."""
    rows = []
    with open(seq_list_file, newline="") as fh:
        for row in csv.reader(fh):
            if row:
                rows.append((row[0].strip(), int(row[1]), row[2].strip()))
    return rows


def encode_sequences(seqs, groups, reverse=False, alphabet="dna"):
    """Sequences (str) with their group ids -> the device text of bear_kmer_sort_create: per sequence a start marker,
    the letter codes and the stop code; with ``reverse`` every sequence is followed by its reverse complement
    (summarize.py:202-207).  ``alphabet='prot'``: the 21-wide text (a ``*`` that ends a sequence is the stop and is left
    out).  Returns ``(text uint8 [n_pos], group uint8 [n_pos])``."""
    prot = _width(alphabet, reverse) == 21
    lut, start, stop = (_PROT_LUT, _PROT_START, _PROT_STOP) if prot else (_LUT, _START, _STOP)
    parts, gparts = [], []
    for seq, g in zip(seqs, groups):
        if not 0 <= int(g) <= 254:
            raise ValueError("group ids must lie in [0, 254]")
        if prot and seq.endswith("*"):
            seq = seq[:-1]
        codes = lut[np.frombuffer(seq.upper().encode("ascii", "replace"), dtype=np.uint8)]
        for c in ((codes, _COMP[codes[::-1]]) if reverse else (codes,)):
            parts.append(np.concatenate([[start], c, [stop]]).astype(np.uint8))
            gparts.append(np.full(c.size + 2, int(g), dtype=np.uint8))
    if not parts:
        return np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8)
    return np.concatenate(parts), np.concatenate(gparts)


def _device_text(text, group, lag, alphabet, device):
    """The checks every counting entry makes first -> (text, group) as CUDA tensors and the row width."""
    width = _width(alphabet)
    _check_lag(lag, alphabet)
    if not torch.cuda.is_available():
        raise RuntimeError("bear_amd counts on an MI355X only (libbear_hip.so has no CPU fallback)")
    device = torch.device(device or "cuda")
    t = text if isinstance(text, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(text)).to(device)
    g = group if isinstance(group, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(group)).to(device)
    if t.dtype != torch.uint8 or g.dtype != torch.uint8 or t.shape != g.shape or t.dim() != 1:
        raise ValueError("text and group must be uint8 vectors of the same length")
    return t, g, width


def _reduce_and_destroy(h, n_rows, lag, n_groups, width, device, stream):
    """The rows of a sorted handle as device tensors; the handle is destroyed, whatever happens."""
    try:
        kmers = torch.empty((n_rows, lag), dtype=torch.uint8, device=device)
        counts = torch.empty((n_groups, n_rows, width), dtype=torch.int32, device=device)
        _lib.call("bear_kmer_sort_reduce", h, int(n_groups), kmers.data_ptr(), None, counts.data_ptr(), stream)
        torch.cuda.current_stream().synchronize()
    finally:
        _lib.lib().bear_kmer_sort_destroy(h)
    return kmers, counts


def n_bins_of(lag, alphabet="dna"):
    """Bins of the histogram of a lag: one per value of the context's last min(lag, BIN_LETTERS) letters."""
    return 1 << (BITS[alphabet] * min(int(lag), BIN_LETTERS[alphabet]))


def bin_letters(b, n_bins, alphabet="dna"):
    """The context letters a bin stands for, first letter first ('[': before the sequence's start)."""
    bits, names = BITS[alphabet], ("ACGT[" if alphabet == "dna" else PROT_LETTERS + "[")
    return "".join(names[min((int(b) >> (bits * j)) & ((1 << bits) - 1), len(names) - 1)] for j in range((int(n_bins).bit_length() - 1) // bits))


def cut_ranges(hist, max_pairs, alphabet="dna"):
    """Cuts the bins of a histogram (transitions per bin, ascending in the sort key) into the ranges of the counting passes:
    ``[(bin_lo, bin_hi, pairs), ...]``, ascending and disjoint, from a non-empty bin to just behind a non-empty bin.  Greedy: a
    range takes bins while its sum stays ``<= max_pairs``; one bin above ``max_pairs`` is a range of its own (a pass can try
    it, and nothing smaller exists) unless it reaches the 2^32 - 1 pairs no pass can index: ``ValueError`` naming its letters."""
    hist = np.asarray(hist, dtype=np.uint64)
    max_pairs = max(1, int(max_pairs))
    bins = np.flatnonzero(hist)
    if bins.size == 0:
        return []
    over = bins[hist[bins] >= PAIR_LIMIT]
    if over.size:
        b = int(over[0])
        raise ValueError(f"bin {b} (contexts ending in {bin_letters(b, hist.size, alphabet)!r}) holds {int(hist[b])} transitions: "
                         f"a counting pass indexes fewer than 2^32 - 1 pairs and a bin is not split")
    ends = np.cumsum(hist[bins], dtype=np.uint64)      # (below 2^64: a text has fewer positions than that)
    out, i = [], 0
    while i < bins.size:
        before = int(ends[i - 1]) if i else 0
        j = max(int(np.searchsorted(ends, before + max_pairs, side="right")), i + 1)
        out.append((int(bins[i]), int(bins[j - 1]) + 1, int(ends[j - 1]) - before))
        i = j
    return out


def pass_plan(n_pos, pass_bytes, free_bytes):
    """The automatic decision as a pure function: ``None`` for the single pass, else the ``max_pairs`` of the passes.
    ``pass_bytes``: ``bear_kmer_sort_bytes`` of ``min(n_pos, 2^32 - 2)`` pairs; ``free_bytes``: free device memory.  A pass may
    take half of what is free -- the other half is for its output slabs and the slices already made, whose size is not known
    before the count; ``count_passes`` halves ``max_pairs`` when a pass still runs out of memory."""
    budget = int(free_bytes) // 2
    if n_pos < PAIR_LIMIT and pass_bytes <= budget:
        return None
    per_pair = max(1.0, pass_bytes / max(1, min(int(n_pos), PAIR_LIMIT - 1)))
    return int(max(1, min(PAIR_LIMIT - 1, budget // per_pair)))


def _is_nomem(e):
    return isinstance(e, torch.cuda.OutOfMemoryError) or (isinstance(e, _lib.BearError) and e.status == _lib.ERR_NOMEM)


def count_passes(text, group, lag, n_groups, max_pairs, device=None, alphabet="dna"):
    """One lag in passes over key ranges of at most ``max_pairs`` transitions each: yields ``(kmers, counts)`` device tensors
    (as ``count_transitions(..., on_device=True)``), one slice of the table per range, ascending -- concatenated they are the
    table.  A pass that runs out of device memory halves ``max_pairs`` for the bins not yet counted; once such a range is a
    single bin the error stands."""
    t, g, width = _device_text(text, group, lag, alphabet, device)
    n_bins = n_bins_of(lag, alphabet)

    def on_text(fn):          # (the device is current for the call only: a generator must not keep it between its yields)
        with torch.cuda.device(t.device):
            return fn(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def histogram(stream):
        hist_dev = torch.empty(n_bins, dtype=torch.int64, device=t.device)
        _lib.call("bear_kmer_bin_hist", t.data_ptr(), t.numel(), int(lag), width, hist_dev.data_ptr(), n_bins, stream)
        return hist_dev.cpu().numpy().view(np.uint64)

    def one_range(lo, hi, pairs):
        def run(stream):
            h, n_rows = ctypes.c_void_p(), ctypes.c_uint64()
            _lib.call("bear_kmer_sort_create_range", t.data_ptr(), g.data_ptr(), t.numel(), int(lag), width, lo, hi, pairs,
                      ctypes.byref(h), ctypes.byref(n_rows), stream)
            return _reduce_and_destroy(h, n_rows.value, lag, n_groups, width, t.device, stream)
        return run

    hist = on_text(histogram)
    ranges = cut_ranges(hist, max_pairs, alphabet)
    while ranges:
        lo, hi, pairs = ranges[0]
        try:
            piece = on_text(one_range(lo, hi, pairs))
        except Exception as e:
            if not _is_nomem(e) or np.count_nonzero(hist[lo:hi]) == 1:
                raise
            torch.cuda.empty_cache()
            max_pairs = max(1, min(int(max_pairs), pairs) // 2)
            rest = hist.copy()
            rest[:lo] = 0
            ranges = cut_ranges(rest, max_pairs, alphabet)
            continue
        ranges.pop(0)
        yield piece
        del piece


def count_transitions(text, group, lag, n_groups, device=None, on_device=False, alphabet="dna", max_pairs=None):
    """One lag on the device.  text / group: uint8 arrays or CUDA tensors.  Returns
    ``(kmers uint8 [n_rows, lag] ASCII, counts uint32 [n_groups, n_rows, 5])`` as numpy arrays, or with ``on_device`` as
    CUDA tensors (counts in int32 storage).  ``alphabet='prot'``: rows of 21, lags up to 12.

    ``max_pairs``: count in passes over key ranges of at most that many transitions (``count_passes``); the table is the same.
    ``None``: ``BEAR_AMD_COUNT_MAX_PAIRS`` if the environment sets it, else decided here (``pass_plan``): the single pass when
    the text has fewer than 2^32 - 1 positions and ``bear_kmer_sort_bytes`` of them fit half the free device memory.  Slices
    are concatenated on the device with ``on_device``; otherwise each goes to the host as it is made and is freed on the device."""
    t, g, width = _device_text(text, group, lag, alphabet, device)
    if max_pairs is None and os.environ.get("BEAR_AMD_COUNT_MAX_PAIRS"):
        max_pairs = int(os.environ["BEAR_AMD_COUNT_MAX_PAIRS"])
    if max_pairs is None and t.numel():
        need = ctypes.c_uint64()
        with torch.cuda.device(t.device):
            _lib.call("bear_kmer_sort_bytes", min(t.numel(), PAIR_LIMIT - 1), int(lag), width, ctypes.byref(need))
            max_pairs = pass_plan(t.numel(), need.value, torch.cuda.mem_get_info(t.device)[0])
    if max_pairs is not None:
        kparts, cparts = [], []
        for kmers, counts in count_passes(t, g, lag, n_groups, max_pairs, alphabet=alphabet):
            kparts.append(kmers if on_device else kmers.cpu().numpy())
            cparts.append(counts if on_device else counts.cpu().numpy().view(np.uint32))
            del kmers, counts
        if on_device:
            if not kparts:
                return (torch.empty((0, lag), dtype=torch.uint8, device=t.device),
                        torch.empty((n_groups, 0, width), dtype=torch.int32, device=t.device))
            return torch.cat(kparts, 0), torch.cat(cparts, 1)
        if not kparts:
            return np.zeros((0, lag), dtype=np.uint8), np.zeros((n_groups, 0, width), dtype=np.uint32)
        return np.concatenate(kparts, 0), np.concatenate(cparts, 1)
    h, n_rows = ctypes.c_void_p(), ctypes.c_uint64()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    with torch.cuda.device(t.device):
        head, tail = (t.data_ptr(), g.data_ptr(), t.numel(), int(lag)), (ctypes.byref(h), ctypes.byref(n_rows), stream)
        if width == 5:
            _lib.call("bear_kmer_sort_create", *head, *tail)
        else:
            _lib.call("bear_kmer_sort_create_wide", *head, width, *tail)
        kmers, counts = _reduce_and_destroy(h, n_rows.value, lag, n_groups, width, t.device, stream)
    if on_device:
        return kmers, counts
    return kmers.cpu().numpy(), counts.cpu().numpy().view(np.uint32)


def _load_sequences(seq_list_file):
    seqs, groups = [], []
    for path, group, ftype in read_file_list(seq_list_file):
        with open(path) as fh:
            for _, seq in load_input(fh, ftype):
                seqs.append(seq)
                groups.append(group)
    return seqs, groups


def load_text(seq_list_file, reverse=False, alphabet="dna"):
    """Every file of the list as the device code text (C++ readers, ``bear_fastx_encode`` / ``_wide``): ``(text, group, n_groups)``."""
    width = _width(alphabet, reverse)
    parts, gparts, groups = [], [], []
    for path, group, ftype in read_file_list(seq_list_file):
        if ftype not in ("fa", "fq"):
            raise ValueError("file type must be 'fa' or 'fq'")
        n = ctypes.c_uint64()
        if width == 5:
            size, encode, head = "bear_fastx_size", "bear_fastx_encode", (path.encode(), int(ftype == "fq"), int(bool(reverse)))
        else:       # the wide twins take the width and refuse reverse
            size, encode, head = "bear_fastx_size_wide", "bear_fastx_encode_wide", (path.encode(), int(ftype == "fq"), 0, width)
        _lib.call(size, *head, ctypes.byref(n), None)    # (leaves a record's closing '*' out, as the encoding pass does)
        text = np.empty(n.value, dtype=np.uint8)
        grp = np.empty(n.value, dtype=np.uint8)
        got = ctypes.c_uint64()
        _lib.call(encode, *head, int(group), n.value, text.ctypes.data, grp.ctypes.data, ctypes.byref(got))
        if got.value != n.value:      # the file changed between the sizing pass and the encoding pass
            raise RuntimeError(f"{path}: {got.value} positions encoded, {n.value} counted")
        parts.append(text)
        gparts.append(grp)
        groups.append(group)
    if not parts:
        return np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), 1
    return np.concatenate(parts), np.concatenate(gparts), max(groups) + 1


def count_tables(seq_list_file, max_lag, reverse=False, batch_size=1 << 30, device=None, on_device=False, alphabet="dna",
                 max_pairs=None):
    """The tables of every lag 1..max_lag as ``CountDataset`` objects (index L-1), never written as text; with
    ``on_device`` as ``DeviceCountDataset`` objects that never leave HBM (count -> shuffle -> plan -> train).
    ``alphabet='prot'``: tables with ``alphabet == 'prot'`` and rows of 21 (max_lag <= 12, no ``reverse``).  ``max_pairs``: as
    ``count_transitions``."""
    _width(alphabet, reverse)
    if max_lag >= 1:
        _check_lag(max_lag, alphabet)
    text, grp, n_groups = load_text(seq_list_file, reverse, alphabet)
    device = torch.device(device or "cuda")
    t, g = torch.from_numpy(text).to(device), torch.from_numpy(grp).to(device)
    out = []
    for lag in range(1, max_lag + 1):
        kmers, counts = count_transitions(t, g, lag, n_groups, on_device=on_device, alphabet=alphabet, max_pairs=max_pairs)
        out.append(DeviceCountDataset(kmers, counts, alphabet, batch_size) if on_device else CountDataset(kmers, counts, alphabet, batch_size))
    return out


def compute_n_bin_bits(total_size, n_groups, mf):
    """summarize.py:594-598."""
    if total_size <= 0:
        return 0
    return int(max([np.ceil(np.log(total_size * n_groups / (mf * 1e9)) / np.log(2)), 0]))


def write_tables(tables, out_prefix, n_bins):
    """``<out_prefix>_lag_<L>_file_<b>.tsv`` (summarize.py:472-473, 529-530), rows dealt round-robin to the bins."""
    for li, d in enumerate(tables):
        km = np.ascontiguousarray(d.kmers)
        cn = np.ascontiguousarray(d.counts)
        for b in range(n_bins):
            path = "{}_lag_{}_file_{}.tsv".format(out_prefix, li + 1, b)
            head = (path.encode(), km.ctypes.data, cn.ctypes.data, d.num_rows, li + 1, d.num_ds)
            if d.width == 5:
                _lib.call("bear_write_counts_tsv", *head, b, n_bins, 0)
            else:
                _lib.call("bear_write_counts_tsv_wide", *head, int(d.width), b, n_bins, 0)


def run(args):
    """summarize.py:622-645: all stages for one direction."""
    print("Start: counting on the device...", datetime.datetime.now())
    tables = count_tables(args.file, args.l, reverse=bool(args.r), alphabet=getattr(args, "a", "dna"))
    n_groups = tables[0].num_ds if tables else 1
    # the reference sizes the bins from the KMC dump sizes (kmer \\t count \\n per distinct k+1-mer); same formula
    total_size = sum(int((d.counts > 0).sum()) * (li + 2 + 4) for li, d in enumerate(tables))
    n_bins = 2 ** compute_n_bin_bits(total_size, n_groups, float(getattr(args, "mf", None) or 0.1))
    write_tables(tables, args.out_prefix, n_bins)
    print("Finished.", datetime.datetime.now())
    return n_bins


def main(args):
    """summarize.py:648-665: forward tables under ``out_prefix``, with ``-r`` forward + reverse-complement tables under
    ``out_prefix + '_rev'``.  Returns ``(n_bins, n_bins_rev)``."""
    store_r, prefix = bool(getattr(args, "r", False)), args.out_prefix
    _width(getattr(args, "a", "dna"), store_r)       # -r with -a prot: refused before any file is read
    n_bins = n_bins_rev = None
    if not getattr(args, "nf", False):
        args.r = False
        n_bins = run(args)
    if store_r:
        args.r = True
        args.out_prefix = prefix + "_rev"
        n_bins_rev = run(args)
    args.r, args.out_prefix = store_r, prefix
    return n_bins, n_bins_rev


if __name__ == "__main__":
    import argparse
    parser = argparse.ArgumentParser(description="Count k-mer transitions for BEAR training (device build).")
    parser.add_argument("file")
    parser.add_argument("out_prefix")
    parser.add_argument("-l", default=10, type=int)
    parser.add_argument("-a", default="dna", choices=["dna", "prot"], help="alphabet of the sequences (prot: rows of 21, -l <= 12, no -r)")
    parser.add_argument("-mk", default=12, type=float, help="ignored (passes are decided from the free device memory)")
    parser.add_argument("-mf", default=0.1, type=float)
    parser.add_argument("-p", default="")
    parser.add_argument("-nf", action="store_true", default=False)
    parser.add_argument("-r", action="store_true", default=False)
    parser.add_argument("-pr", action="store_true", default=False)
    parser.add_argument("-t", default="tmp/")
    parser.add_argument("-s12", action="store_true", default=False)
    parser.add_argument("-s3", action="store_true", default=False)
    main(parser.parse_args())
