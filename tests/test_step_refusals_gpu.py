"""The statuses of the planned step entries for a bad call: every entry that takes a plan, one faulty argument at a time, straight
through the C ABI.  Each must come back BEAR_ERR_INVALID_ARG from the host-side checks -- no launch in this file is made with a
bad pointer -- and a refused call must leave the workspace usable: afterwards a one-launch train step still equals its reduce +
apply form (the workspace's arrival epoch is consumed by launches only)."""
import ctypes

import numpy as np
import pytest
import torch

from util import dense_table

pytestmark = pytest.mark.gpu

INVALID_ARG = -1       # BEAR_ERR_INVALID_ARG (include/bear_hip.h)
N, LAG, FW = 64, 3, 2
SLACK = 8              # rows behind every buffer: an entry that let "n_rows off by one" through would still stay in bounds


class _Case:
    """The valid arguments of one entry, in ABI order (by name), and the faults that apply to it."""

    def __init__(self, name, args, plan_ncol, rows, out, theta=(), adam=(), refuses_empty=False, takes_dense=False):
        self.name, self.args, self.plan_ncol, self.rows, self.out = name, args, plan_ncol, rows, out
        self.theta, self.adam, self.refuses_empty, self.takes_dense = theta, adam, refuses_empty, takes_dense

    def call(self, L, **override):
        a = dict(self.args)
        assert set(override) <= set(a), (self.name, override)
        a.update(override)
        return getattr(L, self.name)(*a.values())


@pytest.fixture(scope="module")
def env():
    from bear_amd import _lib, kernels
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    tr, rf = dense_table(N + SLACK, 17)
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)      # noqa: E731
    e = {"dev": dev, "L": L, "kernels": kernels}
    e["tr_all"], e["rf_all"] = (torch.from_numpy(a.view(np.int32)).to(dev) for a in (tr, rf))
    e["tr"], e["rf"] = e["tr_all"][:N], e["rf_all"][:N]
    e["other"] = e["tr_all"].clone()                         # another tensor with the same rows
    e["plan5"] = kernels.Plan(e["tr"], 5)
    e["plan4"] = kernels.Plan(e["tr"], 4)
    e["dense"] = kernels.Plan(e["tr"], 5, rows_if_dense=True)
    assert e["dense"].rowwise
    e["prior"] = torch.full((N + SLACK, 5), 0.2, dtype=torch.float64, device=dev)
    e["grad"], e["grad2"] = f64(N + SLACK, 5), f64(N + SLACK, 5)
    e["t1"] = f64(N + SLACK, 16)
    codes = kernels.synth_kmer_codes(3, 0, N, LAG, dev, sort=True)
    e["packed_kmers"] = torch.cat([kernels.pack_kmers(codes), torch.zeros(SLACK, dtype=torch.int64, device=dev)])
    e["index"] = torch.cat([kernels.linear_index(e["packed_kmers"][:N], LAG), torch.zeros(SLACK, dtype=torch.int64, device=dev)])
    e["n_cnn"] = kernels.cnn_param_count(LAG, FW)
    e["scalars"] = f64(3)                                    # h_signed, tau_signed, net_weight_signed
    e["out"] = f64(16)
    e["theta_ref"], e["theta_lin"], e["theta_cnn"] = f64(3), f64(1 + LAG * 25), f64(1 + e["n_cnn"])
    e["packed_lin"], e["packed_cnn"] = f64(2 + LAG * 25 + 2), f64(2 + e["n_cnn"] + 2)
    e["adam"] = [f64(1 + LAG * 25) for _ in range(2)] + [f64(1)]
    e["ws"] = e["plan5"].ws.handle
    return e


def _cases(e):
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)      # noqa: E731
    ws, tr, n, eps = e["ws"], p(e["tr"]), N, 1e-32
    P5, P4 = e["plan5"]._h, e["plan4"]._h
    sc = e["scalars"]
    m, v, t = (p(x) for x in e["adam"])
    return [
        _Case("bear_dm_prior_plan_f64", dict(ws=ws, plan=P5, counts=tr, prior=p(e["prior"]), n=n, h=-0.3, eps=eps, ar=0, norm=0, out=p(e["out"]),
                                             stream=None), 5, ["prior"], "out", takes_dense=True),
        _Case("bear_dm_prior_plan_grad_f64", dict(ws=ws, plan=P5, counts=tr, prior=p(e["prior"]), n=n, h=-0.3, eps=eps, ar=0, norm=0,
                                                  out=p(e["out"]), grad=p(e["grad"]), stream=None), 5, ["prior", "grad"], "out", takes_dense=True),
        _Case("bear_dm_prior_plan_dev_f64", dict(ws=ws, plan=P5, counts=tr, prior=p(e["prior"]), n=n, h_dev=p(sc), eps=eps, ar=0, norm=0,
                                                 out=p(e["out"]), grad=p(e["grad"]), stream=None), 5, ["prior", "grad"], "out", theta=["h_dev"],
              takes_dense=True),
        _Case("bear_dm_refmix_plan_grad_f64", dict(ws=ws, plan=P5, counts=tr, net_rows=p(e["prior"]), ref_rows=p(e["grad2"]), n=n, h_dev=p(sc),
                                                   tau_dev=p(sc, 8), nw_dev=p(sc, 16), eps=eps, ar=0, out=p(e["out"]), grad=p(e["grad"]),
                                                   stream=None), 5, ["net_rows", "ref_rows", "grad"], "out", theta=["h_dev", "tau_dev", "nw_dev"]),
        _Case("bear_dm_ref_plan_f64", dict(ws=ws, plan=P4, counts=tr, ref=p(e["rf"]), n=n, h=0.0, tau=-3.4, nu=-4.6, eps=eps, ar=0, out=p(e["out"]),
                                           stream=None), 4, ["ref"], "out"),
        _Case("bear_ref_train_reduce_f64", dict(ws=ws, plan=P4, counts=tr, ref=p(e["rf"]), n=n, theta=p(e["theta_ref"]), eps=eps, ar=0,
                                                packed=p(e["out"]), stream=None), 4, ["ref"], "packed", theta=["theta"], refuses_empty=True),
        _Case("bear_ref_train_step_f64", dict(ws=ws, plan=P4, counts=tr, ref=p(e["rf"]), n=n, theta=p(e["theta_ref"]), m=m, v=v, t=t, eps=eps, ar=0,
                                              lr=0.01, scale=1.0, out=p(e["out"]), loss_buf=None, loss_cap=0, stream=None), 4, ["ref"], "out",
              theta=["theta"], adam=["m", "v", "t"], refuses_empty=True),
        _Case("bear_dm_linear_f64", dict(ws=ws, plan=P5, counts=tr, kmer=p(e["index"]), mat=p(e["theta_lin"], 8), lag=LAG, n=n, h=-0.3, eps=eps, ar=0,
                                         out=p(e["out"]), grad_mat=p(e["packed_lin"], 16), stream=None), 5, ["kmer"], "out", theta=["mat"]),
        _Case("bear_net_linear_train_reduce_f64", dict(ws=ws, plan=P5, counts=tr, kmer=p(e["index"]), lag=LAG, n=n, theta=p(e["theta_lin"]), eps=eps,
                                                       ar=0, packed=p(e["packed_lin"]), stream=None), 5, ["kmer"], "packed", theta=["theta"],
              refuses_empty=True),
        _Case("bear_net_linear_train_step_f64", dict(ws=ws, plan=P5, counts=tr, kmer=p(e["index"]), lag=LAG, n=n, theta=p(e["theta_lin"]), m=m, v=v, t=t,
                                                     packed=p(e["packed_lin"]), eps=eps, ar=0, lr=0.01, scale=1.0, loss_buf=None, loss_cap=0,
                                                     stream=None), 5, ["kmer"], "packed", theta=["theta"], adam=["m", "v", "t"], refuses_empty=True),
        _Case("bear_net_cnn_train_reduce_f64", dict(ws=ws, plan=P5, counts=tr, kmer=p(e["packed_kmers"]), n=n, lag=LAG, fw=FW, nf=e["kernels"].CNN_NUM_FILTERS,
                                                    l1=e["kernels"].CNN_LAYER1_WIDTH, theta=p(e["theta_cnn"]), prior=p(e["prior"]), t1=p(e["t1"]),
                                                    grad=p(e["grad"]), eps=eps, ar=0, packed=p(e["packed_cnn"]), stream=None), 5,
              ["prior", "t1", "grad"], "packed", theta=["theta"], refuses_empty=True),
    ]


def _shift(arg, nbytes):
    return ctypes.c_void_p(arg.value + nbytes)


def test_every_plan_entry_refuses_a_bad_call(env):
    e = env
    L = e["L"]
    cases = _cases(e)
    assert len(cases) == 11
    empty = {}
    for ncol in (4, 5):       # plans of no rows over the same buffer: "n_rows = 0" with nothing else wrong
        h = ctypes.c_void_p()
        assert L.bear_plan_create(e["ws"], ctypes.c_void_p(e["tr"].data_ptr()), 0, ncol, ctypes.byref(h)) == 0
        empty[ncol] = h
    try:
        with torch.cuda.device(e["dev"]):
            for c in cases:
                bad = [("NULL plan", dict(plan=None)),
                       ("n_rows off by one", dict(n=N + 1)),
                       ("n_rows short by one", dict(n=N - 1)),
                       ("another tensor's counts", dict(counts=ctypes.c_void_p(e["other"].data_ptr()))),
                       ("plan of the wrong ncol", dict(plan=(e["plan4"] if c.plan_ncol == 5 else e["plan5"])._h)),
                       (c.out + " offset by 4 bytes", {c.out: _shift(c.args[c.out], 4)})]
                if not c.takes_dense:
                    bad.append(("dense-form plan", dict(plan=e["dense"]._h)))
                bad += [(k + " offset by 8 bytes", {k: _shift(c.args[k], 8)}) for k in c.rows]
                bad += [("NULL " + k, {k: None}) for k in list(c.theta) + list(c.adam)]
                if c.refuses_empty:
                    bad.append(("n_rows = 0", dict(plan=empty[c.plan_ncol], n=0)))
                for what, override in bad:
                    assert c.call(L, **override) == INVALID_ARG, (c.name, what)
    finally:
        for h in empty.values():
            L.bear_plan_destroy(h)
    _steps_still_match(e)


def test_a_plan_of_another_device_is_refused(env):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    e = env
    kernels = e["kernels"]
    dev1 = torch.device("cuda", 1)
    far = {ncol: kernels.Plan(e["tr"].to(dev1), ncol, ws=kernels.Workspace(dev1)) for ncol in (4, 5)}
    with torch.cuda.device(e["dev"]):
        for c in _cases(e):
            # (the counts pointer is the other device's too: the plan's own buffer, so only the device differs)
            override = dict(plan=far[c.plan_ncol]._h, counts=ctypes.c_void_p(far[c.plan_ncol].counts.data_ptr()))
            assert c.call(e["L"], **override) == INVALID_ARG, c.name


def _steps_still_match(e):
    """One valid bear_ref_train_step_f64 and one bear_net_linear_train_step_f64 == their reduce + bear_train_apply_f64 form, as
    tests/test_train_gpu.py::test_one_launch_step_matches_the_two_launch_step compares the two."""
    kernels, dev = e["kernels"], e["dev"]

    def run(step, reduce, theta0, n_packed):
        res = []
        for one_launch in (True, False):
            theta = theta0.clone()
            m, v, t = torch.zeros_like(theta), torch.zeros_like(theta), torch.zeros(1, dtype=torch.float64, device=dev)
            packed, loss = torch.zeros(n_packed, dtype=torch.float64, device=dev), torch.zeros(4, dtype=torch.float64, device=dev)
            for _ in range(3):
                if one_launch:
                    step(theta, m, v, t, packed, loss)
                else:
                    reduce(theta, packed)
                    kernels.train_apply(theta, packed, m, v, t, 0.01, 1.0 / N, loss_buf=loss)
            res.append((loss[:3].cpu().numpy(), theta.cpu().numpy()))
        (l1, p1), (l2, p2) = res
        assert np.all(np.isfinite(l1)) and np.all(l1 != 0.0)
        assert np.allclose(l1, l2, rtol=1e-12, atol=0)
        assert np.allclose(p1, p2, rtol=1e-9, atol=1e-12)

    theta_ref = torch.tensor([0.0, np.log(1 / 30), -np.log(100)], dtype=torch.float64, device=dev)
    run(lambda th, m, v, t, pk, ls: kernels.ref_train_step(e["plan4"], e["rf"], th, m, v, t, 0.01, 1.0 / N, pk, loss_buf=ls),
        lambda th, pk: kernels.ref_train_reduce(e["plan4"], e["rf"], th, pk), theta_ref, 4)
    g = torch.Generator().manual_seed(5)
    theta_lin = torch.cat([torch.tensor([-0.3], dtype=torch.float64), 0.1 * torch.randn(LAG * 25, dtype=torch.float64, generator=g)]).to(dev)
    index = e["index"][:N]
    run(lambda th, m, v, t, pk, ls: kernels.net_linear_train_step(e["plan5"], index, LAG, th, m, v, t, pk, 0.01, 1.0 / N, loss_buf=ls),
        lambda th, pk: kernels.net_linear_train_reduce(e["plan5"], index, LAG, th, pk), theta_lin, 2 + LAG * 25)
