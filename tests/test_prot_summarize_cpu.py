"""Protein count tables from sequence files, the host side: the 21-wide code text of the FASTA / FASTQ readers, the 21-wide
table writer, and the refusals that need no device (every argument check of bear_kmer_sort_create_wide happens before its first
device call).  No GPU needed."""
import ctypes
import types

import numpy as np
import pytest

from bear_amd import _lib, dataloader, summarize
from test_prot_cpu import PROT, make_prot_table, write_prot_tsv

INVALID_ARG = -1      # BEAR_ERR_INVALID_ARG


def _encode_file(path, fastq, width, group, reverse=0):
    """Both passes of the native reader -> (status, text, group array)."""
    L = _lib.lib()
    n = ctypes.c_uint64()
    st = L.bear_fastx_size_wide(str(path).encode(), fastq, reverse, width, ctypes.byref(n), None)
    if st != 0:
        return st, None, None
    text, grp = np.full(n.value, 255, dtype=np.uint8), np.full(n.value, 255, dtype=np.uint8)
    got = ctypes.c_uint64()
    st = L.bear_fastx_encode_wide(str(path).encode(), fastq, reverse, width, group, n.value, text.ctypes.data, grp.ctypes.data,
                                  ctypes.byref(got))
    assert st != 0 or got.value == n.value, "the sizing pass and the encoding pass disagree"
    return st, text, grp


# lower case, residues outside the 20, an inner '*', a trailing '*', a sequence that is only a '*', an empty record
PROT_SEQS = ["ARNDCEQGHILKMFPSTWYV", "arndceqghilkmfpstwyv", "MKXBZUOJ-LV", "MK*LV*", "ACDEFGHIKLMNPQRSTVWY" * 7 + "*", "", "*", "A**",
             "WYV"]


def _write_fasta(path, seqs, wrap, eol):
    with open(path, "w", newline="") as fh:
        for i, s in enumerate(seqs):
            fh.write(f">seq{i} some description{eol}")
            for a in range(0, len(s), wrap):
                fh.write(s[a:a + wrap] + eol)


def _write_fastq(path, seqs, eol):
    with open(path, "w", newline="") as fh:
        for i, s in enumerate(seqs):
            fh.write(f"@read{i}{eol}{s}{eol}+{eol}{'I' * len(s)}{eol}")


@pytest.mark.parametrize("eol", ["\n", "\r\n"])
def test_protein_code_text_matches_the_python_encoder(tmp_path, eol):
    want_text, want_grp = summarize.encode_sequences(PROT_SEQS, [3] * len(PROT_SEQS), alphabet="prot")
    # the code text itself, spelled out once: start 21, residues in the order of core.alphabets_en['prot'], 22, stop 20
    one, _ = summarize.encode_sequences(["MK*LV*", "mX"], [0, 0], alphabet="prot")
    assert one.tolist() == [21, PROT.index("M"), PROT.index("K"), 22, PROT.index("L"), PROT.index("V"), 20, 21, PROT.index("M"), 22, 20]
    for wrap in (7, 60, 1000):
        fa = tmp_path / f"p{wrap}.fa"
        _write_fasta(fa, PROT_SEQS, wrap, eol)
        st, text, grp = _encode_file(fa, 0, 21, 3)
        assert st == 0
        assert text.tobytes() == want_text.tobytes() and grp.tobytes() == want_grp.tobytes()
    fq = tmp_path / "p.fq"
    _write_fastq(fq, PROT_SEQS, eol)
    st, text, grp = _encode_file(fq, 1, 21, 3)
    assert st == 0 and text.tobytes() == want_text.tobytes() and grp.tobytes() == want_grp.tobytes()
    # the Python reader of the same files sees the same sequences (what make_sequence_counter counts from a file list)
    lst = tmp_path / "l.csv"
    lst.write_text(f"{fq},3,fq\n{tmp_path / 'p7.fa'},3,fa\n")
    seqs, groups = summarize._load_sequences(str(lst))
    assert seqs == PROT_SEQS + PROT_SEQS and set(groups) == {3}
    # load_text: both files, through the size / encode pair with its mismatch check
    text2, grp2, n_groups = summarize.load_text(str(lst), alphabet="prot")
    assert n_groups == 4 and text2.tobytes() == want_text.tobytes() * 2 and grp2.tobytes() == want_grp.tobytes() * 2
    # no complement: reverse is refused by both passes, and by the Python side before any file is read
    L = _lib.lib()
    n = ctypes.c_uint64()
    assert L.bear_fastx_size_wide(str(fq).encode(), 1, 1, 21, ctypes.byref(n), None) == INVALID_ARG
    buf = np.zeros(4096, dtype=np.uint8)
    assert L.bear_fastx_encode_wide(str(fq).encode(), 1, 1, 21, 0, buf.size, buf.ctypes.data, None, ctypes.byref(n)) == INVALID_ARG
    assert L.bear_fastx_encode_wide(str(fq).encode(), 1, 0, 7, 0, buf.size, buf.ctypes.data, None, ctypes.byref(n)) == INVALID_ARG
    with pytest.raises(ValueError, match="reverse"):
        summarize.load_text(str(tmp_path / "missing.csv"), reverse=True, alphabet="prot")
    with pytest.raises(ValueError, match="reverse"):
        summarize.encode_sequences(["AR"], [0], reverse=True, alphabet="prot")
    with pytest.raises(ValueError):
        summarize.encode_sequences(["AR"], [0], alphabet="rna")


@pytest.mark.parametrize("reverse", [0, 1])
def test_width_5_reader_is_the_dna_reader(tmp_path, reverse):
    L = _lib.lib()
    seqs = ["ACGTNacgt", "", "TTTAT*", "GGGCCCAAATTT" * 9, "N"]
    for fastq, path in ((0, tmp_path / "d.fa"), (1, tmp_path / "d.fq")):
        if fastq:
            _write_fastq(path, seqs, "\r\n")
        else:
            _write_fasta(path, seqs, 10, "\n")
        n = ctypes.c_uint64()
        assert L.bear_fastx_size(str(path).encode(), fastq, reverse, ctypes.byref(n), None) == 0
        want_t, want_g = np.zeros(n.value, dtype=np.uint8), np.zeros(n.value, dtype=np.uint8)
        got = ctypes.c_uint64()
        assert L.bear_fastx_encode(str(path).encode(), fastq, reverse, 2, n.value, want_t.ctypes.data, want_g.ctypes.data,
                                   ctypes.byref(got)) == 0 and got.value == n.value
        st, text, grp = _encode_file(path, fastq, 5, 2, reverse)
        assert st == 0 and text.tobytes() == want_t.tobytes() and grp.tobytes() == want_g.tobytes()
        py_t, py_g = summarize.encode_sequences(seqs, [2] * len(seqs), reverse=bool(reverse))       # (a '*' is an "other" letter here)
        assert text.tobytes() == py_t.tobytes() and grp.tobytes() == py_g.tobytes()


def test_wide_writer_round_trip(tmp_path):
    kmers, counts = make_prot_table(seed=7, n=500, lag=4, num_ds=3)
    counts[1, 5, 20] = counts[0, 17, 0] = counts[2, 499, 11] = 2 ** 32 - 1
    counts[2, 0] = np.arange(21) * 204522252          # every digit count from 1 to 10
    want = tmp_path / "want.tsv"
    write_prot_tsv(want, kmers, counts)
    want_bytes = want.read_bytes()
    km = np.frombuffer("".join(kmers).encode(), dtype=np.uint8).reshape(len(kmers), 4).copy()
    L = _lib.lib()
    # several bins: rows row_begin, row_begin + n_bins, ...
    n_bins, lines = 4, want_bytes.splitlines(keepends=True)
    for b in range(n_bins):
        path = tmp_path / f"bin{b}.tsv"
        assert L.bear_write_counts_tsv_wide(str(path).encode(), km.ctypes.data, counts.ctypes.data, len(kmers), 4, 3, 21, b, n_bins, 0) == 0
        assert path.read_bytes() == b"".join(lines[b::n_bins])
        d = dataloader.dataloader(str(path), "prot", 64, 3)
        assert d.width == 21 and np.array_equal(d.counts, counts[:, b::n_bins]) and np.array_equal(d.kmers, km[b::n_bins])
    # append: the bins one after the other into one file
    whole = tmp_path / "whole.tsv"
    for b in range(n_bins):
        assert L.bear_write_counts_tsv_wide(str(whole).encode(), km.ctypes.data, counts.ctypes.data, len(kmers), 4, 3, 21, b, n_bins, int(b > 0)) == 0
    assert whole.read_bytes() == b"".join(b"".join(lines[b::n_bins]) for b in range(n_bins))
    # dataloader.write_counts_tsv, planar and row-major
    for form, c in (("planar", counts), ("rows", counts.transpose(1, 0, 2))):
        path = tmp_path / f"{form}.tsv"
        dataloader.write_counts_tsv(str(path), kmers, c)
        assert path.read_bytes() == want_bytes
        d = dataloader.dataloader(str(path), "prot", 128, 3)
        assert np.array_equal(d.counts, counts) and [bytes(r).decode() for r in d.kmers] == kmers
    # width 5 through the wide writer is the 5-wide writer
    c5 = np.ascontiguousarray(counts[:, :, :5])
    assert L.bear_write_counts_tsv_wide(str(tmp_path / "w5.tsv").encode(), km.ctypes.data, c5.ctypes.data, len(kmers), 4, 3, 5, 0, 1, 0) == 0
    assert L.bear_write_counts_tsv(str(tmp_path / "n5.tsv").encode(), km.ctypes.data, c5.ctypes.data, len(kmers), 4, 3, 0, 1, 0) == 0
    assert (tmp_path / "w5.tsv").read_bytes() == (tmp_path / "n5.tsv").read_bytes()
    # other widths stay refused
    assert L.bear_write_counts_tsv_wide(str(tmp_path / "w7.tsv").encode(), km.ctypes.data, counts.ctypes.data, len(kmers), 4, 3, 7, 0, 1, 0) == INVALID_ARG
    with pytest.raises(ValueError):
        dataloader.write_counts_tsv(str(tmp_path / "w7.tsv"), kmers, np.zeros((3, len(kmers), 7), dtype=np.uint32))


def test_refusals_without_a_device(tmp_path):
    L = _lib.lib()
    text = np.array([21, 0, 1, 20], dtype=np.uint8)       # host memory: a call that got past its checks would fail differently
    grp = np.zeros(4, dtype=np.uint8)
    h, n_rows = ctypes.c_void_p(), ctypes.c_uint64()

    def create(lag, width):
        return L.bear_kmer_sort_create_wide(text.ctypes.data, grp.ctypes.data, text.size, lag, width, ctypes.byref(h), ctypes.byref(n_rows), None)
    assert create(3, 7) == INVALID_ARG
    assert create(13, 21) == INVALID_ARG
    assert create(0, 21) == INVALID_ARG
    assert create(0, 5) == INVALID_ARG and create(22, 5) == INVALID_ARG
    assert h.value is None
    assert L.bear_kmer_sort_create_wide(None, None, 4, 3, 21, ctypes.byref(h), ctypes.byref(n_rows), None) == INVALID_ARG
    assert L.bear_kmer_sort_create_wide(text.ctypes.data, grp.ctypes.data, 4, 3, 21, None, ctypes.byref(n_rows), None) == INVALID_ARG
    # Python: the limit is named
    with pytest.raises(ValueError, match="12"):
        summarize.count_transitions(text, grp, 13, 1, alphabet="prot")
    with pytest.raises(ValueError, match="12"):
        summarize.count_tables(str(tmp_path / "missing.csv"), 13, alphabet="prot")
    with pytest.raises(ValueError):
        summarize.count_transitions(text, grp, 0, 1, alphabet="prot")
    with pytest.raises(ValueError):
        summarize.count_transitions(text, grp, 3, 1, alphabet="rna")
    # summarize -r -a prot: refused before any file is read (the list does not exist)
    args = types.SimpleNamespace(file=str(tmp_path / "missing.csv"), out_prefix=str(tmp_path / "out"), l=3, nf=False, r=True, mf=0.1, a="prot")
    with pytest.raises(ValueError, match="reverse"):
        summarize.main(args)
    with pytest.raises(ValueError, match="reverse"):
        summarize.run(args)
    assert not list(tmp_path.iterdir())
    # the counter: reverse defaults to True (the DNA callers' default) and has to be switched off for residues
    from bear_amd import get_var_probs
    with pytest.raises(ValueError, match="reverse=False"):
        get_var_probs.make_sequence_counter(["ARND"], 2, alphabet_name="prot")
    with pytest.raises(ValueError, match="reverse=False"):
        get_var_probs.make_sequence_counter(str(tmp_path / "missing.csv"), 2, no_end=True, alphabet_name="prot")
