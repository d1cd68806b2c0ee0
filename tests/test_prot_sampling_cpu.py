"""CPU tests of the posterior-sampling oracle at the protein width (rows of 21: 20 letters + stop): the MAP table against its
closed form, the mean of the sampled log-probabilities against the digamma expectation, and the normalisation of every draw.
The GPU tests of bear_logdir_sample_wide_f64 hold the kernel against this oracle."""
import numpy as np
from scipy.special import digamma, logsumexp

import bear_oracle as o
from test_prot_cpu import make_prot_table

W = 21


def _inputs(seed=0, K=40):
    _, counts = make_prot_table(seed=seed, n=K, num_ds=1)
    counts = counts[0].astype(np.float64)
    counts[0] = 0
    counts[1, -1] = 4294967295.0
    rng = np.random.default_rng(seed + 1)
    ar = rng.dirichlet(np.full(W, 0.4), size=K) + 1e-7
    ar[2, 3] = 1e-300
    return counts, ar


def test_oracle_map_is_the_closed_form():
    counts, ar = _inputs()
    h = np.array([1e-3, 1.0, 30.0])
    vans = np.array([0.1, 1.0, 10.0])
    got = o.get_pdf_numpy(counts, ar, h, vans, 1, True)
    assert got.shape == (len(counts), W, 1 + len(h) + len(vans), 1)
    concs = [ar] + [ar / hh + counts for hh in h] + [v + counts for v in vans]
    for m, a in enumerate(concs):
        want = np.log(a) - np.log(a.sum(-1, keepdims=True))
        assert np.allclose(got[:, :, m, 0], want, rtol=1e-13, atol=1e-13), m
    # vanilla models only, unseen k-mers
    got = o.get_pdf_numpy(np.zeros((3, W)), None, None, vans, 1, True)
    for m, v in enumerate(vans):
        assert np.allclose(got[:, :, m, 0], -np.log(W))


def test_oracle_sample_means_match_digamma():
    row = np.zeros((1, W))
    row[0, :6] = [0, 1, 3, 17, 250, 4000]
    vans = np.array([0.1, 1.0, 10.0])
    mc = 20000
    lp = o.get_pdf_numpy(row, None, None, vans, mc, False, seed=3, row_base=11)   # [1, W, M, mc]
    assert lp.shape == (1, W, len(vans), mc)
    for m, v in enumerate(vans):
        a = row[0] + v
        x = lp[0, :, m, :]
        mean, se = x.mean(-1), x.std(-1) / np.sqrt(mc)
        want = digamma(a) - digamma(a.sum())
        assert np.all(np.abs(mean - want) < 5 * se), (v, (mean - want) / se)


def test_oracle_samples_are_normalised():
    counts, ar = _inputs(seed=2, K=25)
    lp = o.get_pdf_numpy(counts, ar, np.array([0.05, 1e3]), np.array([0.1, 10.0]), 9, False, seed=5, row_base=2 ** 40 + 3)
    assert lp.shape == (25, W, 4, 9) and np.isfinite(lp).all()
    assert np.abs(logsumexp(lp, axis=1)).max() < 1e-12
