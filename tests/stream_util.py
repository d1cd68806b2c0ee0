"""The harness of tests/test_stream_contract_gpu.py: what it takes to see that an entry of the C ABI keeps the stream contract of
include/bear_hip.h (launches are asynchronous on `stream`, outputs are valid once that stream is synchronised) when the stream
is NOT the default one.  Every other GPU test runs on torch's default stream -- the legacy null stream, on which everything
serialises with everything -- so a launch on stream 0 instead of `s`, a device-wide wait, or a wrapper that hands over the wrong
stream cannot show there.

Gates.  A gate is a chain of public torch ops (fp64 ``mm`` on a 2048 x 2048 buffer of its own) that occupies a stream for a known
time and touches none of the test's tensors.
  * the SIDE gate runs on the side stream in front of ``inp.copy_(true)`` and the entry: until it is through, the entry's inputs
    hold DECOY values (valid inputs with another answer), so an entry that reads them from another stream, or before its stream
    gets there, computes the decoy's answer;
  * the NULL gate runs on the default stream, with an event behind it: work that the entry wrongly puts on stream 0 queues behind
    it and is missing when the side stream has drained (the outputs still hold the sentinel bytes), and a device-wide wait
    inside the entry shows as that event being complete.
Spy.  ``Spy`` wraps the loaded library and records every ``bear_*`` call with its last argument; for the entries whose declaration
ends in ``void *stream`` that value must be the side stream's handle.
``judge`` runs one case and returns the list of its failures, each starting with the letter of the condition it misses -- the
controls of the test module go through the same function and must fail in the right way."""
import math
import time

import numpy as np
import torch

from util import stream_entries

SENTINEL_BYTE = 0xA5          # every byte of a tensor the wrappers allocate: float64 -1.6e-129, int32 -1515870811, uint8 165
GATE_N = 2048
MIN_GATE_MS = 10.0
HOST_FACTOR = 20              # the side gate lasts at least this many host enqueue times of the entry
NULL_FACTOR = 3               # the null gate: this many times the side stream's work (the two share the device while both run)
STREAM_ENTRIES = stream_entries()


class Gate:
    """``reps`` fp64 products of a 2048 x 2048 matrix with itself into a second buffer, on the current stream."""

    def __init__(self, device):
        self.a = torch.full((GATE_N, GATE_N), 1.0 / GATE_N, dtype=torch.float64, device=device)
        self.b = torch.empty_like(self.a)
        self.ms_per_rep = None

    def measure(self, reps=40):
        """Device milliseconds of one product, timed with events over ``reps`` of them (after a warm-up)."""
        for _ in range(5):
            torch.mm(self.a, self.a, out=self.b)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            torch.mm(self.a, self.a, out=self.b)
        e1.record()
        torch.cuda.synchronize()
        self.ms_per_rep = e0.elapsed_time(e1) / reps
        return self.ms_per_rep

    def run(self, ms):
        """Occupies the current stream for about ``ms`` milliseconds; the event recorded behind the chain."""
        for _ in range(max(1, int(math.ceil(ms / self.ms_per_rep)))):
            torch.mm(self.a, self.a, out=self.b)
        e = torch.cuda.Event()
        e.record()
        return e


class Harness:
    """One side stream, a gate per stream (each with buffers of its own) and the measured time of a gate product."""

    def __init__(self, device):
        self.device = device
        self.side = torch.cuda.Stream(device)
        self.side2 = torch.cuda.Stream(device)     # the second side stream of the re-entrancy test: three streams in all, with the default one
        self.side_gate, self.null_gate = Gate(device), Gate(device)
        self.null_gate.ms_per_rep = self.side_gate.measure()
        with torch.cuda.stream(self.side):
            self.side_gate.run(1.0)
        torch.cuda.synchronize()
        self.records = []        # one dict per judged case: what profiles/stream_contract.md tabulates


def _handle(arg):
    """A call's last argument as the integer a stream handle is (NULL: 0); None for what is no handle."""
    if arg is None:
        return 0
    if isinstance(arg, int):
        return arg
    v = getattr(arg, "value", False)
    return (v or 0) if v is not False and (v is None or isinstance(v, int)) else None


class Spy:
    """Recording proxy of the loaded library: ``calls`` = [(entry, last argument as an integer)] of every ``bear_*`` call."""

    def __init__(self, real):
        self._real = real
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("bear_"):
            return fn

        def recorded(*args):
            self.calls.append((name, _handle(args[-1]) if args else None))
            return fn(*args)
        return recorded


def install_spy(monkeypatch):
    from bear_amd import _lib
    spy = Spy(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", spy)
    return spy


class _SentinelTorch:
    """``torch`` as the wrapper modules see it during a case: ``empty`` / ``empty_like`` hand out device tensors whose every byte is
    SENTINEL_BYTE (filled on the current stream, so in front of the entry's launch there) -- the wrappers allocate their outputs."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        return getattr(self._real, name)

    @staticmethod
    def _fill(t):
        if t.is_cuda and t.numel() and t.is_contiguous():
            t.view(-1).view(torch.uint8).fill_(SENTINEL_BYTE)
        return t

    def empty(self, *args, **kw):
        return self._fill(self._real.empty(*args, **kw))

    def empty_like(self, *args, **kw):
        return self._fill(self._real.empty_like(*args, **kw))


def install_sentinel(monkeypatch):
    from bear_amd import kernels, summarize
    for mod in (kernels, summarize):
        monkeypatch.setattr(mod, "torch", _SentinelTorch(torch))


def _host(outs):
    """The outputs of a call (a tensor, or a tuple / list / dict of tensors and Nones) as a flat list of NumPy arrays, copied on the
    CURRENT stream and waited for on that stream alone."""
    if isinstance(outs, torch.Tensor):
        outs = [outs]
    elif isinstance(outs, dict):
        outs = list(outs.values())
    return [o.detach().cpu().numpy() for o in outs if o is not None]


def distance(got, want):
    """Largest ``|got - want| / max|want|`` over the outputs of a call (each array scaled by its own largest magnitude; integer and
    byte outputs: 0.0 when equal, inf otherwise).  NaN counts as infinitely far."""
    worst = 0.0
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype, (g.dtype, w.dtype)
        if g.shape != w.shape:                   # (a table of another number of rows)
            return math.inf
        if not g.size:
            continue
        if g.dtype.kind != "f":
            d = 0.0 if np.array_equal(g, w) else math.inf
        elif g.tobytes() == w.tobytes():
            d = 0.0
        elif not (np.isfinite(g).all() and np.isfinite(w).all()):
            d = math.inf
        else:
            d = float(np.abs(g - w).max() / max(float(np.abs(w).max()), np.finfo(np.float64).tiny))
        worst = max(worst, d)
    return worst


def _copy_in(inp, true):
    for k, v in true.items():
        if isinstance(v, torch.Tensor):
            inp[k].copy_(v)
        else:
            inp[k] = v


def judge(h, name, cls, true, decoy, call, tol, spy, tol_from=""):
    """One case.  ``true`` / ``decoy``: {name: value input} -- device tensors of equal shape and dtype, or host values the entry takes
    by value; ``call(inputs)`` runs the entry on the current stream and returns its outputs; ``cls``: "A" (asynchronous on the
    stream: conditions a, b, c, d and the spy) or "B" (a set-up path that may wait or allocate: a, b and the spy); ``tol``: the bound
    of ``distance`` to the default-stream run (0: equal bits).  Returns the failures, [] when the case holds."""
    assert cls in "AB" and set(true) == set(decoy)
    side, fails = h.side, []
    call(true)                                                      # (first use: code objects, workspaces, lazy buffers)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    ref_dev = call(true)
    e1.record()
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1)
    ref = _host(ref_dev)
    dec = _host(call(decoy))
    torch.cuda.synchronize()
    gap = distance(dec, ref)
    if not all(np.isfinite(d).all() for d in dec if d.dtype.kind == "f"):
        fails.append("b: the decoy's answer is not finite: a decoy is a valid input")
    if not (gap >= 1000.0 * tol and gap > 0.0):
        fails.append(f"b: the decoy's answer is {gap:.3e} from the true one, the case needs >= {1000.0 * tol:.1e} and > 0")
    inp = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in decoy.items()}
    with torch.cuda.stream(side):                                   # this stream's first use of the entry (its own workspace)
        call(inp)
    torch.cuda.synchronize()
    gate_ms = max(MIN_GATE_MS, HOST_FACTOR * host_ms, dev_ms) if cls == "A" else MIN_GATE_MS
    null_event = None
    if cls == "A":
        null_event = h.null_gate.run(NULL_FACTOR * (gate_ms + dev_ms))
    spy.calls.clear()
    with torch.cuda.stream(side):
        side_event = h.side_gate.run(gate_ms)
        _copy_in(inp, true)
        out_dev = call(inp)
        side_busy = not side_event.query()
    seen = list(spy.calls)
    side.synchronize()
    null_busy = null_event is not None and not null_event.query()
    with torch.cuda.stream(side):
        got = _host(out_dev)                                        # (copied on the side stream: the default one is behind its gate)
    torch.cuda.synchronize()
    dist = distance(got, ref)
    if not dist <= tol:
        sentinel = any(g.size and (g.view(np.uint8) == SENTINEL_BYTE).all() for g in got)
        fails.append(f"a: {dist:.3e} from the default-stream run (bound {tol:.1e}; the decoy's answer is {distance(got, dec):.3e} away"
                     + ("; an output still holds the sentinel bytes" if sentinel else "") + ")")
    if cls == "A" and not side_busy:
        fails.append(f"c: the side gate ({gate_ms:.1f} ms) was through when the call returned ({host_ms:.3f} ms of host time on the "
                     "default stream): the entry waited for its stream, or the gate is too short")
    if cls == "A" and not null_busy:
        fails.append(f"d: the null gate ({NULL_FACTOR * (gate_ms + dev_ms):.1f} ms) was through when the side stream had drained: "
                     "something waited for the whole device, or the gate is too short")
    wrong = [(n, s) for n, s in seen if n in STREAM_ENTRIES and s != side.cuda_stream]
    if wrong:
        fails.append(f"spy: stream arguments other than the side stream's {side.cuda_stream}: {wrong}")
    h.records.append(dict(name=name, cls=cls, tol=tol, tol_from=tol_from, gap=gap, dist=dist, host_ms=host_ms, dev_ms=dev_ms,
                          gate_ms=gate_ms, entries=sorted({n for n, _ in seen if n in STREAM_ENTRIES})))
    return fails
