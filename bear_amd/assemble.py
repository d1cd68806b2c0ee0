"""Sequence generation from seeds under a BEAR / BMM model: host mirror of ``bear_model/assemble.py``.

``assemble_no_ends`` (assemble.py:21-184) with the reference's arguments: for every seed and replicate a flank is grown
to the right of the seed and (through the reverse complement) to its left, one letter at a time; the transition
log-probabilities of the current end k-mer come from ``get_var_probs.get_pdf`` (posterior samples -- one AR model per
generated sequence -- or the MAP table), the letter from a Gumbel-max draw (:121).  The sampling of the tables runs on
the device (``bear_logdir_sample_f64``); the per-letter bookkeeping stays on the host as in the reference.

Differences: transition counts come from ``counter`` (e.g. ``get_var_probs.make_sequence_counter(...)``, the device-built
table look-up) instead of a KMC database (``kmc_path`` still works where ``py_kmc_api`` is installed); a BMM run
(``van=...``) does not need a trained-model folder; and a new k-mer's table row is stored under the index the k-mer
was given (the reference indexes k-mers in order of appearance but stores their rows in sorted order, assemble.py:96-99,
so that rows can be swapped between k-mers that first appear in the same step).

With a ``get_var_probs.DeviceCounter`` as ``counter=`` the flanks grow on the device instead (``kernels.generate_steps``,
kernels_generate.h): look-up, table values and Gumbel-max draws of every letter in one launch per direction for a BMM, one
launch per step behind the AR function for a trained model.  A table value is keyed by (seed, sequence, k-mer, letter), so the
sample a sequence sees is the same whenever it meets a k-mer again and ``batch_size`` has no effect; ``device_path=False``
keeps the host loop for such a counter.

``generate_sequences`` (no counterpart in the reference) samples WHOLE sequences from such a counter: from the start context or a
prompt, letter by letter until the stop symbol is drawn or ``max_len`` letters are written (``kernels.generate_whole``).
"""
import os

import numpy as np
from scipy.special import xlogy

from . import core, get_var_probs, summarize

_COMP = str.maketrans("ACGTUacgtu", "TGCAAtgcaa")


def reverse_complement(seq):
    return seq.translate(_COMP)[::-1]


def _host_flanks(counter, seqs_by_dir, lengths_by_dir, lag, alphabet, alphabet_name, h, ar_func, vans, train_col, get_map, batch_size,
                 rng, seed):
    """The reference's loop (assemble.py:60-130): letter by letter on the host, a sampled table row per new k-mer and live sequence."""
    flanks = []
    for seqs_all_b, length_all_b in zip(seqs_by_dir, lengths_by_dir):
        all_batch_new = []
        for lo in range(0, len(seqs_all_b), batch_size):
            seqs = seqs_all_b[lo:lo + batch_size]
            length_to_gen = length_all_b[lo:lo + batch_size]
            new_seq = len(seqs) * [""]
            new_len = np.zeros(len(seqs), dtype=int)
            inds = np.nonzero(new_len < length_to_gen)[0]
            end_kmers = np.array([s[-lag:] for s in seqs[inds]])
            kmer_row, all_pdf = {}, None                      # k-mer -> row of all_pdf [rows, letters, (live sequences)]
            step = 0
            while len(inds) > 0:
                new_kmers = np.unique([k for k in end_kmers if k not in kmer_row])
                if len(new_kmers) > 0:
                    counts = counter(new_kmers)[:, None, :]
                    for k in new_kmers:
                        kmer_row[k] = len(kmer_row)
                    pdf = get_var_probs.get_pdf(new_kmers, counts, h, ar_func, len(end_kmers), vans, train_col, alphabet_name,
                                                get_map, output="numpy", seed=None if seed is None else seed + 7919 * step,
                                                row_base=len(kmer_row))[:, :-1, 0, :]
                    all_pdf = pdf if all_pdf is None else np.concatenate([all_pdf, pdf])
                rows = np.array([kmer_row[k] for k in end_kmers])
                tlp = all_pdf[rows]                               # [live, letters, samples]
                tlp = tlp[:, :, 0] if get_map else tlp[np.arange(len(rows)), :, np.arange(len(rows))]
                new_letters = alphabet[np.argmax(rng.gumbel(size=tlp.shape) + tlp, axis=-1)]      # assemble.py:121
                keep = new_len[inds] + 1 < length_to_gen[inds]
                for j, ind in enumerate(inds):
                    new_seq[ind] += new_letters[j]
                    new_len[ind] += 1
                end_kmers = np.array([e[1:] + l for e, l, k in zip(end_kmers, new_letters, keep) if k])
                if not get_map:
                    all_pdf = all_pdf[:, :, keep]                 # one posterior sample per live sequence (assemble.py:126)
                inds = inds[keep]
                step += 1
            all_batch_new.append(new_seq)
        flanks.append(np.concatenate(all_batch_new) if all_batch_new else np.array([]))
    return flanks


def _require_letters(s, letters_en, what, alphabet_name):
    """Every character of a seed or a prompt is a letter of the alphabet, or ``ValueError``."""
    for ch in set(s):
        if ch not in letters_en:
            raise ValueError(f"character {ch!r} of {what} {s!r} is not a letter of the alphabet {alphabet_name!r}")


def _ar_step(generate, state, t, seed, ar_func, kmer_codes, W, h, get_map):
    """Step ``t`` of a trained model: the AR function's rows of the current end k-mers, then one launch of ``generate``
    (``kernels.generate_steps`` / ``generate_whole`` over its ``state``), which also writes the next end k-mers to ``kmer_codes``."""
    import torch
    with torch.no_grad():
        prior = ar_func(kmer_codes).to(torch.float64).expand(kmer_codes.shape[0], W).contiguous()
    generate(*state, t, 1, seed, prior=prior, h=None if get_map else float(h), get_map=get_map, codes=kmer_codes)


def _write_seqs_fa(save_folder, gen_seqs):
    """``seqs.fa`` in ``save_folder``: row i, replicate j as ``>seq{i}_rep{j}``."""
    os.makedirs(save_folder, exist_ok=True)
    with open(os.path.join(save_folder, "seqs.fa"), "w") as f:
        for i, seqs in enumerate(gen_seqs):
            for j, seq in enumerate(seqs):
                f.write(">seq{}_rep{}\n{}\n".format(i, j, seq))


def _device_flanks(counter, seqs_by_dir, lengths_by_dir, lag, alphabet_name, h, ar_func, vans, get_map, seed):
    """The flanks of both directions grown on the device (``kernels.generate_steps``, kernels_generate.h): no table, no dictionary
    and no host round trip per letter.  A BMM takes one launch per direction; a trained model one AR-function call and one launch
    per step, and nothing is synchronised before the letters of both directions are copied back.  The sample index of a sequence is
    ``direction * n_total + its index``: left and right flanks are different posterior samples, as in the reference."""
    import torch
    from . import kernels
    from .log_gamma import _next_seed
    if counter.lag != lag or counter.alphabet_name != alphabet_name:
        raise ValueError(f"counter: a lag-{counter.lag} table of {counter.alphabet_name!r}, asked for lag {lag} of {alphabet_name!r}")
    letters_en = [str(ch) for ch in core.alphabets_en[alphabet_name][:-1]]
    W, device = counter.width, counter.device
    n_total = len(seqs_by_dir[1])
    if alphabet_name == "prot" and n_total and np.any(np.asarray(lengths_by_dir[0]) > 0):
        raise ValueError("a left flank grows along the reverse complement: the protein alphabet has none, ask for left lengths of 0")
    ends = []
    for seqs in seqs_by_dir:                                   # every refusal comes before the first launch
        for s_ in seqs:
            s_ = str(s_)
            if len(s_) < lag:
                raise ValueError(f"seed {s_!r} is shorter than the lag {lag}")
            _require_letters(s_, letters_en, "seed", alphabet_name)
        raw = np.frombuffer("".join(str(s_)[-lag:] for s_ in seqs).encode("ascii"), dtype=np.uint8)
        ends.append(counter._lut[raw].reshape(len(seqs), lag))
    seed = _next_seed() if seed is None else seed
    char_of = np.frombuffer("".join(letters_en).encode("ascii"), dtype=np.uint8)
    grown = []
    with torch.cuda.device(device):
        for direction, (codes, lens) in enumerate(zip(ends, lengths_by_dir)):
            lens = np.maximum(np.asarray(lens, dtype=np.int64).reshape(-1), 0)
            n_steps = int(lens.max()) if lens.size else 0
            letters = torch.full((n_total, n_steps), 0xFF, dtype=torch.uint8, device=device)
            grown.append((letters, lens))
            if n_steps == 0:
                continue
            keys = counter._keys_of_codes(torch.from_numpy(np.ascontiguousarray(codes)).to(device))
            sample = torch.arange(n_total, dtype=torch.int64, device=device) + direction * n_total
            left = torch.from_numpy(lens.astype(np.int32)).to(device)
            common = (counter.keys, counter.counts_by_key, counter.rank, lag, keys, sample, left, letters)
            if ar_func is None:
                kernels.generate_steps(*common, 0, n_steps, seed, van=float(vans[0]), get_map=get_map)
            else:
                kmer_codes = counter.codes_of_keys(keys)
                for t in range(n_steps):
                    _ar_step(kernels.generate_steps, common, t, seed, ar_func, kmer_codes, W, None if get_map else h[0], get_map)
        flanks = []
        for letters, lens in grown:                            # the one copy back (and the first synchronisation)
            chars = char_of[np.minimum(letters.cpu().numpy(), W - 2)]
            flanks.append(np.array([chars[i, :int(l)].tobytes().decode("ascii") for i, l in enumerate(lens)]))
    return flanks


def assemble_no_ends(seqs_fa_file, lengths_to_gen, num_to_gen, bear_path, kmc_path,
                     h=None, reverse=True, save_folder=None, batch_size=100,
                     van=None, lag=None, alphabet_name=None, get_map=False, counter=None, seed=None, device_path=True):
    """assemble.assemble_no_ends (assemble.py:21-184) -> ``(gen_seqs [len(seqs), num_to_gen], sw_ent)``.  A ``DeviceCounter`` as
    ``counter`` takes the device path (``device_path=False``: the host loop); it refuses, with ``ValueError`` and before any launch, a
    seed shorter than ``lag`` or with a character outside the alphabet, a counter of another lag or alphabet, and a left flank for
    ``prot``."""
    if bear_path is not None:
        lag, alphabet_name, h_bear, ar_func, _ = get_var_probs.load_bear(bear_path)
        if h is None:
            h = h_bear
    else:
        assert van is not None, "without a trained model folder only a BMM (van=...) can generate"
        ar_func = None
    h = np.array([h]) if h is not None else None
    if van is not None:
        assert lag is not None and alphabet_name is not None
        vans, ar_func, h = van * np.ones(1), None, None
    else:
        vans = []
    train_col = 0
    alphabet = core.alphabets_en[alphabet_name][:-1]
    alphabet_size = len(alphabet)
    if counter is None:
        counter = get_var_probs.make_kmc_genome_counter(kmc_path, lag, reverse=reverse, no_end=True)
    rng = np.random if seed is None else np.random.RandomState(seed)

    with open(seqs_fa_file) as fh:
        fwd_seqs = np.array([s for _, s in summarize.load_input(fh, "fa")])
    n_seeds = len(fwd_seqs)
    fwd_seqs = np.repeat(fwd_seqs, num_to_gen)
    lengths = np.repeat(np.asarray(lengths_to_gen).reshape(n_seeds, 2), num_to_gen, axis=0)     # [:, 0] left, [:, 1] right
    rev_seqs = np.array([reverse_complement(s) for s in fwd_seqs])

    if isinstance(counter, get_var_probs.DeviceCounter) and device_path:
        flanks = _device_flanks(counter, [rev_seqs, fwd_seqs], [lengths[:, 0], lengths[:, 1]], lag, alphabet_name, h, ar_func, vans,
                                get_map, seed)
    else:
        flanks = _host_flanks(counter, [rev_seqs, fwd_seqs], [lengths[:, 0], lengths[:, 1]], lag, alphabet, alphabet_name, h, ar_func,
                              vans, train_col, get_map, batch_size, rng, seed)

    gen_seqs = [reverse_complement(left) + seed_seq + right for left, right, seed_seq in zip(flanks[0], flanks[1], fwd_seqs)]
    gen_seqs = np.array(gen_seqs).reshape([-1, num_to_gen])
    sw_ent = []
    for seqs in gen_seqs:
        probs = np.average(core.tf_one_hot(list(seqs), alphabet_name).cpu().numpy(), axis=0)
        sw_ent.append(-np.sum(xlogy(probs, probs), axis=-1))
    if save_folder is not None:
        _write_seqs_fa(save_folder, gen_seqs)
        try:
            import matplotlib
            matplotlib.use("Agg")
            from matplotlib import pyplot as plt
            plt.figure(figsize=[10, 5])
            plt.xlabel("entropy", fontsize=15)
            plt.ylabel("position", fontsize=15)
            for ent, ltg in zip(sw_ent, np.asarray(lengths_to_gen).reshape(n_seeds, 2)):
                plt.plot(np.arange(len(ent)) - ltg[0], ent, color="blue", linewidth=1, alpha=0.1)
            plt.savefig(os.path.join(save_folder, "entropy.png"), dpi=200)
            plt.close()
        except Exception:
            pass
    return gen_seqs, sw_ent


def _any_left(left):
    """Whether any sequence still has steps to take: the one synchronising look of the per-step path."""
    return bool(left.any().item())


def _generate_ref(model, counter, ref_counter, state, max_len, seed, h, get_map, stepwise):
    """``generate_sequences`` under a bear_ref model (``kernels.generate_whole_ref`` over ``state``, ``generate_whole``'s): the stop
    net function and the fused protein linear one in one launch, the mixing and the net function inside the kernel; otherwise (or
    ``stepwise``) the net function's rows and one launch per step, looking every 16 steps whether anything is left."""
    import torch
    from . import kernels
    table, counts, rank, lag, keys, sample, left = state[:7]
    W, device = counter.width, counter.device
    ref = (ref_counter.keys, ref_counter.counts_by_key if ref_counter.keys.numel() else None)
    args = (table, counts, *ref, *state[2:])
    kw = dict(h=h, get_map=get_map)
    net = model.net_func
    mat = getattr(net, "linear_mat", None)
    if not stepwise and net is None:
        kernels.generate_whole_ref(*args, 0, max_len, seed, model.tau, model.net_weight, **kw)
    elif not stepwise and mat is not None and getattr(net, "fused", False) and W == kernels.LINEAR_WIDE_WIDTH and mat.device == device:
        kernels.generate_whole_ref(*args, 0, max_len, seed, model.tau, model.net_weight, mat=mat.detach().contiguous(), **kw)
    else:
        kmer_codes = counter.codes_of_keys(keys)
        stop_rows = None
        if net is None:             # the stop net function as rows: the one-hot at the stop
            stop_rows = torch.zeros((keys.numel(), W), dtype=torch.float64, device=device)
            stop_rows[:, -1] = 1.0
        for t in range(max_len):
            g = stop_rows if net is None else model.net_rows(kmer_codes)
            kernels.generate_whole_ref(*args, t, 1, seed, model.tau, model.net_weight, net_rows=g, codes=kmer_codes, **kw)
            if (t + 1) % 16 == 0 and t + 1 < max_len and not _any_left(left):
                break


def generate_sequences(counter, num_to_gen, max_len, bear_path=None, ar_func=None, h=None, van=None, get_map=False, prompts=None,
                       seed=None, save_folder=None, stepwise=False, ref_model=None, ref_counter=None):
    """Whole sequences from the model over ``counter`` (a ``get_var_probs.DeviceCounter`` counted WITH ends; its lag and alphabet
    are the model's) -> ``(seqs, stopped)``, both ``[len(prompts), num_to_gen]``: every prompt (strings over the alphabet, shorter
    than the lag or empty if need be; default one empty prompt, the start of a sequence) continued ``num_to_gen`` times, the
    prompt included, and whether the stop symbol was drawn -- False: cut at ``max_len`` generated letters.  The model is ``van`` (a
    BMM), ``bear_path`` (``load_bear``) or ``ar_func`` with ``h``; with ``get_map`` a BMM / BEAR table is taken at its MAP value and a
    trained model generates at its AR function's.  The start key is the last ``lag`` symbols of ``'[' * lag + prompt``; the sample
    index of a sequence is ``prompt index * num_to_gen + replicate`` and steps count generated letters from 0, so equal seeds give
    equal strings.

    The device is the only path (``kernels.generate_whole``, kernels_generate.h).  A BMM takes one launch; a trained model one AR
    call and one launch per step, looking every 16 steps whether any sequence is still growing; the linear AR function of the
    protein alphabet (``make_ar_func_linear(lag, 20)``: ``linear_mat``, ``fused``) runs inside the kernel instead, one launch for
    everything, unless ``stepwise``.  ``ValueError`` before any launch: a ``no_end`` counter (its stop column is zeroed), a prompt
    character outside the alphabet, ``max_len < 0``, no model or more than one.  ``save_folder`` receives ``seqs.fa``.

    ``ref_model=`` (a ``get_var_probs.RefModel`` or a folder of ``train_bear_ref.py``) with ``ref_counter=`` (the ``DeviceCounter`` of
    the reference column) is a model trained by ``bear_ref``: the reference mixing runs inside the kernel
    (``kernels.generate_whole_ref``), so the stop net function -- the standard configuration -- and the protein linear one take one
    launch for everything; any other net function, or ``stepwise``, one net call and one launch per step.  ``h`` defaults to the
    model's.  ``ValueError`` before any launch: only one of the two, a counter of another lag or alphabet than the model's, a
    ``no_end`` reference counter, another model (``van``, ``bear_path``, ``ar_func``) beside them."""
    import torch
    from . import kernels
    from .log_gamma import _next_seed
    if not isinstance(counter, get_var_probs.DeviceCounter):
        raise TypeError("generate_sequences runs on the device only: counter must be a get_var_probs.DeviceCounter")
    if counter.no_end:
        raise ValueError("a no_end counter has its stop column zeroed: no sequence would ever end")
    ref_model = get_var_probs._ref_setup(ref_model, ref_counter, counter, dict(van=van, bear_path=bear_path, ar_func=ar_func))
    if (van is not None) + (bear_path is not None) + (ar_func is not None) + (ref_model is not None) != 1:
        raise ValueError("exactly one model: van=... (a BMM), bear_path=..., ar_func=... with h=... or ref_model=... with ref_counter=...")
    if ar_func is not None and h is None and not get_map:
        raise ValueError("ar_func needs h (the AR model alone is a table only at its MAP value: get_map=True)")
    num_to_gen, max_len = int(num_to_gen), int(max_len)
    if max_len < 0 or num_to_gen < 0:
        raise ValueError("max_len and num_to_gen count letters and sequences: not negative")
    lag, W, device, name = counter.lag, counter.width, counter.device, counter.alphabet_name
    letters_en = "".join(str(ch) for ch in core.alphabets_en[name][:-1])
    prompts = [""] if prompts is None else [str(p) for p in prompts]
    for p in prompts:
        _require_letters(p, letters_en, "prompt", name)
    if bear_path is not None:
        lag_b, name_b, h_b, ar_func, _ = get_var_probs.load_bear(bear_path)
        if (lag_b, name_b) != (lag, name):
            raise ValueError(f"counter: a lag-{lag} table of {name!r}, the model at {bear_path!r} has lag {lag_b} of {name_b!r}")
        h = h_b if h is None else h
    if ref_model is not None:
        h = ref_model.h if h is None else h
    n_total = len(prompts) * num_to_gen
    seed = _next_seed() if seed is None else seed
    starts = np.frombuffer("".join(("[" * lag + p)[-lag:] for p in prompts).encode("ascii"), dtype=np.uint8)
    with torch.cuda.device(device):
        keys = counter._keys_of_codes(torch.from_numpy(counter._lut[starts].reshape(len(prompts), lag)).to(device))
        keys = keys.repeat_interleave(num_to_gen).contiguous()
        sample = torch.arange(n_total, dtype=torch.int64, device=device)
        left = torch.full((n_total,), max_len, dtype=torch.int32, device=device)
        length = torch.zeros(n_total, dtype=torch.int32, device=device)
        stopped = torch.zeros(n_total, dtype=torch.uint8, device=device)
        letters = torch.full((n_total, max_len), 0xFF, dtype=torch.uint8, device=device)
        state = (counter.keys, counter.counts_by_key, counter.rank, lag, keys, sample, left, length, stopped, letters)
        mat = getattr(ar_func, "linear_mat", None)
        if n_total == 0:
            pass
        elif ref_model is not None:
            _generate_ref(ref_model, counter, ref_counter, state, max_len, seed, None if get_map else float(h), get_map, stepwise)
        elif ar_func is None:
            kernels.generate_whole(*state, 0, max_len, seed, van=float(van), get_map=get_map)
        elif not stepwise and mat is not None and getattr(ar_func, "fused", False) and W == kernels.LINEAR_WIDE_WIDTH and mat.device == device:
            # (a protein key holds at most 12 letters, SCORE_MAX_LAG: every lag of such a counter fits the kernel's LDS image of mat)
            kernels.generate_whole(*state, 0, max_len, seed, mat=mat.detach().contiguous(), h=None if get_map else float(h),
                                   get_map=get_map)
        else:
            kmer_codes = counter.codes_of_keys(keys)
            for t in range(max_len):
                _ar_step(kernels.generate_whole, state, t, seed, ar_func, kmer_codes, W, h, get_map)
                if (t + 1) % 16 == 0 and t + 1 < max_len and not _any_left(left):
                    break
        # the one copy back: letters | length as four bytes | stopped, a row per sequence
        back = torch.cat([letters, length.view(torch.uint8).reshape(n_total, 4), stopped[:, None]], 1).cpu().numpy()
    chars = np.frombuffer(letters_en.encode("ascii"), dtype=np.uint8)[np.minimum(back[:, :max_len], W - 2)]
    lens = np.ascontiguousarray(back[:, max_len:max_len + 4]).view(np.int32).reshape(-1)
    seqs = [prompts[i // num_to_gen] + chars[i, :int(l)].tobytes().decode("ascii") for i, l in enumerate(lens)]
    seqs = np.array(seqs, dtype=str).reshape(len(prompts), num_to_gen)
    if save_folder is not None:
        _write_seqs_fa(save_folder, seqs)
    return seqs, back[:, max_len + 4].astype(bool).reshape(len(prompts), num_to_gen)
