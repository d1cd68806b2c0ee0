"""CPU tests of the training host path's pure pieces (bear_amd/_train.py): the resident / streamed / refused decision, the
parameter vector's packing, and the rows-of-the-live-contexts helper.  No device is touched."""
import itertools

import pytest
import torch

from bear_amd import _train

EPOCH, WINDOW = 1365, 900

# (asked, epoch fits, shuffled, n_pieces) -> per "window fits" in (True, False): (status, why is set, rows asked of `check`).
# Written out by hand from the rules: streaming asked -> 1, else 0 if the epoch fits; an epoch that does not fit -> 2 when shuffled
# or fewer than two pieces, else 1; status 1 and not shuffled -> the window is checked, and a window that does not fit -> 2.  The
# epoch is checked only when streaming was not asked, the window only in that last case.
E, W = EPOCH, WINDOW
TABLE = {
    # asked: the epoch is never checked; unshuffled, the window is
    (1, True, 0, 1): {True: (1, False, [W]), False: (2, True, [W])},
    (1, True, 0, 2): {True: (1, False, [W]), False: (2, True, [W])},
    (1, False, 0, 1): {True: (1, False, [W]), False: (2, True, [W])},
    (1, False, 0, 2): {True: (1, False, [W]), False: (2, True, [W])},
    # asked and shuffled: nothing is checked (the caller refuses a shuffled streamed epoch)
    (1, True, 1, 1): {True: (1, False, []), False: (1, False, [])},
    (1, True, 1, 2): {True: (1, False, []), False: (1, False, [])},
    (1, False, 1, 1): {True: (1, False, []), False: (1, False, [])},
    (1, False, 1, 2): {True: (1, False, []), False: (1, False, [])},
    # not asked, the epoch fits: resident, whatever else
    (0, True, 0, 1): {True: (0, False, [E]), False: (0, False, [E])},
    (0, True, 0, 2): {True: (0, False, [E]), False: (0, False, [E])},
    (0, True, 1, 1): {True: (0, False, [E]), False: (0, False, [E])},
    (0, True, 1, 2): {True: (0, False, [E]), False: (0, False, [E])},
    # not asked, the epoch refused: one piece or a shuffled epoch cannot be streamed
    (0, False, 0, 1): {True: (2, True, [E]), False: (2, True, [E])},
    (0, False, 1, 1): {True: (2, True, [E]), False: (2, True, [E])},
    (0, False, 1, 2): {True: (2, True, [E]), False: (2, True, [E])},
    # ... two pieces in file order can: streamed if the window fits
    (0, False, 0, 2): {True: (1, True, [E, W]), False: (2, True, [E, W])},
}


@pytest.mark.parametrize("asked, epoch_fits, window_fits, shuffled, n_pieces",
                         list(itertools.product((0, 1), (True, False), (True, False), (0, 1), (1, 2))))
def test_residency_status(asked, epoch_fits, window_fits, shuffled, n_pieces):
    calls, refused = [], []

    def check(rows):
        calls.append(rows)
        if not {EPOCH: epoch_fits, WINDOW: window_fits}[rows]:
            refused.append(rows)
            raise MemoryError(f"{rows} rows do not fit")
    status, why = _train.residency_status(check, EPOCH, WINDOW, asked, shuffled, n_pieces)
    want_status, want_why, want_calls = TABLE[(asked, epoch_fits, shuffled, n_pieces)][window_fits]
    assert status == want_status
    assert (why is not None) == want_why
    assert calls == want_calls
    if why is not None:                         # the message of the LAST refusal travels to the warning / the MemoryError
        assert why == f"{refused[-1]} rows do not fit"


def test_residency_table_is_complete():
    assert len(TABLE) == 16 and all(set(v) == {True, False} for v in TABLE.values())


def test_pack_and_unpack_theta_round_trip():
    g = torch.Generator().manual_seed(3)
    shapes = [(), (3, 5, 5), (7,), (2, 1, 4), (1,)]
    params = [torch.randn(s, generator=g, dtype=torch.float32 if i == 2 else torch.float64).requires_grad_() for i, s in enumerate(shapes)]
    theta = _train.pack_theta(params, torch.device("cpu"))
    want = torch.cat([p.detach().reshape(-1).to(torch.float64) for p in params])
    assert theta.dtype == torch.float64 and theta.is_contiguous() and not theta.requires_grad
    assert theta.shape == (sum(p.numel() for p in params),) and torch.equal(theta, want)
    # three scalars (bear_ref's stop path): the values of a stack, in order
    assert torch.equal(_train.pack_theta(params[:1] * 3, torch.device("cpu")), torch.stack([params[0].detach()] * 3))
    # theta is a copy: the update of the vector reaches the parameters only through unpack_theta
    before = [p.detach().clone() for p in params]
    theta += torch.arange(1, theta.numel() + 1, dtype=torch.float64)
    assert all(torch.equal(p.detach(), b) for p, b in zip(params, before))
    _train.unpack_theta(theta, params)
    k = 0
    for p, b in zip(params, before):
        assert p.requires_grad and p.shape == b.shape and p.dtype == b.dtype
        assert torch.equal(p.detach(), theta[k:k + p.numel()].reshape(p.shape).to(p.dtype))
        assert not torch.equal(p.detach(), b)
        k += p.numel()
    assert k == theta.numel()


def live_entry(n=12, live=(0, 2, 3, 7, 11)):
    counts = torch.zeros((n, 5), dtype=torch.int32)
    for j, i in enumerate(live):
        counts[i, j % 5] = j + 1
    return {"rows": n, "train": counts, "codes": (torch.arange(n * 3, dtype=torch.int8) % 5).reshape(n, 3),
            "ref_in": torch.arange(n * 5, dtype=torch.float64).reshape(n, 5)}, list(live)


def row_fn(codes, ref_in=None):
    """A stand-in for an AR function: a row per context that depends on the context's own columns only."""
    out = codes.to(torch.float64).sum(dim=1, keepdim=True) + torch.arange(5, dtype=torch.float64) + 1.0
    return out if ref_in is None else out * ref_in


def test_rows_on_live_scatters_the_live_rows(monkeypatch):
    monkeypatch.delenv("BEAR_AMD_ALL_ROWS", raising=False)
    e, live = live_entry()
    want = torch.zeros((12, 5), dtype=torch.float64)
    want[live] = row_fn(e["codes"])[live]
    seen = []
    got = _train.rows_on_live(e, lambda codes: seen.append(codes.shape[0]) or row_fn(codes))
    assert seen == [5] and torch.equal(got, want)
    # a second gathered column (bear_ref's reference rows), and the width given
    want2 = torch.zeros((12, 5), dtype=torch.float64)
    want2[live] = row_fn(e["codes"], e["ref_in"])[live]
    assert torch.equal(_train.rows_on_live(e, row_fn, columns=("codes", "ref_in")), want2)
    assert torch.equal(_train.rows_on_live(e, row_fn, width=5), want)
    # by another column: its own live rows
    e["test"] = torch.zeros((12, 5), dtype=torch.int32)
    e["test"][[1, 4], 0] = 9
    want3 = torch.zeros((12, 5), dtype=torch.float64)
    want3[[1, 4]] = row_fn(e["codes"])[[1, 4]]
    assert torch.equal(_train.rows_on_live(e, row_fn, by="test", width=5), want3)
    # differentiable: the gradient reaches the parameters through the live rows only
    w = torch.ones(5, dtype=torch.float64, requires_grad=True)
    _train.rows_on_live(e, lambda codes: row_fn(codes) * w).sum().backward()
    assert torch.equal(w.grad, row_fn(e["codes"])[live].sum(dim=0))


def test_rows_on_live_all_rows_live_returns_the_function_value():
    e, _ = live_entry(live=range(12))
    made = []
    got = _train.rows_on_live(e, lambda codes: made.append(row_fn(codes)) or made[-1])
    assert got is made[0] and made[0].shape == (12, 5) and torch.equal(got, row_fn(e["codes"]))
    assert _train.live_rows(e, "codes") is None


def test_rows_on_live_all_rows_switch(monkeypatch):
    monkeypatch.setenv("BEAR_AMD_ALL_ROWS", "1")
    e, _ = live_entry()
    seen = []
    got = _train.rows_on_live(e, lambda codes: seen.append(codes) or row_fn(codes))
    assert seen[0] is e["codes"] and torch.equal(got, row_fn(e["codes"]))          # every row, the empty contexts' too


@pytest.mark.parametrize("all_live", [False, True])
def test_rows_on_live_single_row_is_expanded(monkeypatch, all_live):
    monkeypatch.delenv("BEAR_AMD_ALL_ROWS", raising=False)
    e, _ = live_entry(live=range(12) if all_live else (0, 2, 3, 7, 11))
    one = torch.tensor([[0.1, 0.2, 0.3, 0.4, 0.0]], dtype=torch.float64)
    got = _train.rows_on_live(e, lambda codes: one, width=5)
    assert got.shape == (12, 5) and got.is_contiguous() and torch.equal(got, one.expand(12, 5))


def test_loss_scales_and_zero_reduce():
    class Res:
        batches = [{"global_rows": 300}, {"global_rows": 165}]
    assert _train.loss_scales(Res, 1365) == [-(1365 / 300), -(1365 / 165)]
    packed = torch.ones(4, dtype=torch.float64)
    _train.zero_reduce(packed)
    assert not packed.any()
