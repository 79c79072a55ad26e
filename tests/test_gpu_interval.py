"""Interval-censored rows (side 2: the truth lies in [y, upper]) on the device: the pointwise functions against a 600-digit
fixture, ``laplace_fit_step(..., upper=)`` against the dense restatement of tests/interval_helpers.py, a ragged batch against its
sites one by one, the gradient against central differences, the two limits (very wide and very narrow brackets), the
no-regression identities and the error rules of ``dgp_laplace_interval_*``.

Bounds.  Pointwise: those of the one-sided test (test_gpu_censored.py), 1e-13 for log P and sigma g, 1e-11 for W v, 1e-9 for
sigma^3 d3, each relative to max(1, |reference|).  Dense restatement: ``_check_against`` of test_gpu_censored.py, as it stands
there.  A site in a batch against its single-site plan: the bounds of test_gpu_censored_batched.py (NLL 1e-11, gradients / dr 1e-9
of their largest entry, f 1e-9 absolute).  Central differences with step 1e-4 in theta: the truncation error is h^2 / 6 |NLL'''|
~ 1e-8 of the gradient's scale and the rounding error eps |NLL| / h ~ 1e-10, so the bound is 1e-6 of the largest entry.
The narrow limit's constant: a bracket of width w_i (model space) around y_i has log P = log N(y_i | f_i, v_i) + log w_i +
O(Delta^2), so NLL(brackets) = NLL(plain) - sum log w_i = NLL(plain) - sum log(w_i / sigma_i) - sum log sigma_i: the second sum
is the Gaussian density's own normalisation, which the plain NLL carries and log P does not.

Measured on an MI355X (EXPERIMENTS.md, "Interval-censored observations").  Pointwise, worst over the fixture's 1266 bounded
points: log P 4.0e-16, sigma g 7.3e-16, W v 1.2e-12, sigma^3 d3 4.5e-11 (the last two in the tail regime).  Dense restatement, worst
over the twenty cases: |f - f_ref| 7.2e-15, NLL 5.6e-16, dtheta 1.1e-14, dr 1.2e-13.  Ragged batch against single sites: bitwise.
Central differences 4.7e-7.  Wide limit 3.6e-16 / 1.2e-16 / 1.1e-15; narrow limit 2.7e-11 / 1.5e-11, NLL constant to 7.4e-12."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from oracle import gp_oracle as orc
from tests import censored_helpers as ch
from tests import interval_helpers as ih
from tests import test_gpu_censored as base

pytestmark = pytest.mark.gpu

TOL = base.TOL
NFAR = 24  # the far points (za = -100, -300, -1000, every Delta) at the end of the fixture


def _theta(d):
    theta = torch.full((orc.loadest_ntheta(d),), base.LN2, dtype=torch.float64)
    return theta * torch.linspace(0.8, 1.3, theta.numel(), dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _case(n, d, frac, seed):
    """-> (model, X, y, side, v, m, theta, upper) of a loadest fixture with the three censored kinds; shared, never modified."""
    X = torch.tensor(orc.synth_loadest(n, d, seed=seed)[0])
    y, side, v, m, upper = ih.synth(X.numpy(), frac, seed)
    for a in (y, side, v, m, upper):
        a.setflags(write=False)
    return "loadest", X, y, side, v, m, _theta(d), upper


@functools.lru_cache(maxsize=None)
def _reference(n, d, frac, seed):
    model, X, y, side, v, m, theta, upper = _case(n, d, frac, seed)
    return ih.laplace(model, X, y, side, v, m, theta, upper=upper, tol=TOL)


def _dev(dev, *arrays):
    return base._dev(dev, *arrays)


def _fit_step(plan, dev, case, tol=TOL, upper="case", side=None):
    _model, X, y, side0, v, m, theta, up = case
    plan.set_inputs(X.to(dev).contiguous())
    yd, vd, md, sd = _dev(dev, y, v, m, side0 if side is None else side)
    ud = _dev(dev, up)[0] if isinstance(upper, str) else upper
    out, dr, f_hat, stat = plan.laplace_fit_step(theta, yd, md, vd, sd, tol=tol, upper=ud)
    return out.cpu(), dr.cpu(), f_hat.cpu(), stat


def test_pointwise_functions_against_the_600_digit_fixture(gpu_device):
    data = np.load(os.path.join(os.path.dirname(__file__), "golden", "interval_terms.npy"))  # rows: za, Delta, the four functions
    za, delta, ref = data[0], data[1], data[2:]
    plan = base._plan("loadest", 8, 2, gpu_device)
    got = plan.interval_terms(torch.tensor(za).to(gpu_device), torch.tensor(delta).to(gpu_device)).cpu().numpy()
    near, far = slice(0, len(za) - NFAR), slice(len(za) - NFAR, len(za))
    assert za[near].min() == -40.0 and za[near].max() == 38.0 and (za[near] + delta[near]).max() <= 40.0
    assert sorted(set(delta.tolist())) == [1e-6, 1e-4, 1e-3, 1e-2, 0.1, 1.0, 5.0, 30.0]
    assert sorted(set(za[far].tolist())) == [-1000.0, -300.0, -100.0]
    err = [np.abs(got[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k])) for k in range(4)]
    h, c = 0.5 * delta, np.abs(za + 0.5 * delta)
    narrow = (h <= ih.NARROW_H) & (c * h <= ih.NARROW_A)
    tail = ~narrow & ((za + delta <= 0) | (za >= 0))
    index = np.arange(len(za))
    for name, mask in (("narrow", narrow), ("tail", tail), ("straddle", ~narrow & ~tail)):
        mask = mask & (index < len(za) - NFAR)
        print(f"interval terms, {name} ({int(mask.sum())} points): log P {err[0][mask].max():.2e}, sigma g {err[1][mask].max():.2e}, "
              f"W v {err[2][mask].max():.2e}, sigma^3 d3 {err[3][mask].max():.2e}")
    print(f"interval terms, far ({NFAR} points): log P {err[0][far].max():.2e}, sigma g {err[1][far].max():.2e}, "
          f"W v {err[2][far].max():.2e}, sigma^3 d3 {err[3][far].max():.2e}")
    assert np.all(np.isfinite(got))
    assert np.all((got[2] > 0) & (got[2] <= 1))
    assert err[0][near].max() <= 1e-13 and err[1][near].max() <= 1e-13 and err[2][near].max() <= 1e-11 and err[3][near].max() <= 1e-9
    # the far points: log P and the mean do not cancel anywhere
    assert err[0][far].max() <= 1e-13 and err[1][far].max() <= 1e-13


CASES = [(n, d, frac, 100 * d + n) for n in (1, 2, 65, 129, 257) for d in (2, 3) for frac in (0.2, 1.0)]


@pytest.mark.parametrize("n,d,frac,seed", CASES, ids=[f"n{c[0]}-d{c[1]}-{c[2]}" for c in CASES])
def test_fit_step_against_the_dense_restatement(gpu_device, n, d, frac, seed):
    case = _case(n, d, frac, seed)
    ref = _reference(n, d, frac, seed)
    side = case[3]
    assert ref["converged"] and ref["capped"] == 0 and ref["iterations"] <= 30
    assert (side == 2).any() and side[0] != 0 and side[-1] != 0
    if n > 2:
        assert (side == -1).any() and (side == 1).any()
    if frac == 1.0:
        assert (side != 0).all()
    plan = base._plan(case[0], n, d, gpu_device)
    out, dr, f_hat, stat = _fit_step(plan, gpu_device, case)
    base._check_against(out, dr, f_hat, stat, ref, plan.ntheta, f"interval n={n} d={d} frac={frac}")
    assert stat[3] == 0
    if n == 1:  # the mode solves a scalar equation
        root = ih.scalar_mode(float(ref["K"][0, 0]), float(case[2][0]), float(case[7][0]), float(case[4][0]), float(case[5][0]))
        assert abs(float(f_hat[0]) - root) <= 1e-11
    # a second call repeats bitwise; the value-only entry: same mode, same NLL, no gradient
    out2, dr2, f2, stat2 = _fit_step(plan, gpu_device, case)
    assert torch.equal(out, out2) and torch.equal(dr, dr2) and torch.equal(f_hat, f2) and stat == stat2
    _m, X, y, side, v, m, theta, upper = case
    yd, vd, md, sd, ud = _dev(gpu_device, y, v, m, side, upper)
    outf, ff, statf = plan.laplace_factorize(theta, yd, md, vd, sd, tol=TOL, upper=ud)
    outf = outf.cpu()
    assert abs(float(outf[_lib.OUT_NLL]) - ref["nll"]) <= base.NLL_BOUND * abs(ref["nll"]) and statf[0] == stat[0]
    assert torch.all(outf[_lib.OUT_DTHETA:] == 0) and float((ff.cpu() - f_hat).abs().max()) <= base.F_BOUND


def test_ragged_batch_against_its_sites_one_by_one(gpu_device):
    from discontinuum_amd.backend import GPPlan

    d = 2
    sites = [(5, d, 1.0, 41), (129, d, 0.2, 42), (200, d, 0.5, 43)]
    cases = [_case(*s) for s in sites]
    B, n = len(sites), max(s[0] for s in sites)
    X = torch.full((B, n, d), float("nan"), dtype=torch.float64)
    y, m, v, up = (torch.full((B, n), float("nan"), dtype=torch.float64) for _ in range(4))
    side = torch.full((B, n), 7, dtype=torch.int32)  # the unused tails may hold anything
    for b, (c, s) in enumerate(zip(cases, sites)):
        nb = s[0]
        X[b, :nb], y[b, :nb], m[b, :nb], v[b, :nb], up[b, :nb] = c[1], torch.tensor(c[2]), torch.tensor(c[5]), torch.tensor(c[4]), torch.tensor(c[7])
        side[b, :nb] = torch.tensor(c[3])
    theta = torch.stack([c[6] for c in cases])
    plan = GPPlan("loadest", n, d, dtype=torch.float64, device=gpu_device, lookahead=1, batch=B)
    plan.set_site_sizes([s[0] for s in sites])
    to = lambda t: t.to(gpu_device).contiguous()  # noqa: E731
    plan.set_inputs(to(X))
    args = (theta, to(y), to(m), to(v), to(side))
    out, dr, f_hat, stat = plan.laplace_fit_step(*args, tol=TOL, upper=to(up))
    out, dr, f_hat = out.cpu(), dr.cpu(), f_hat.cpu()
    again = plan.laplace_fit_step(*args, tol=TOL, upper=to(up))
    assert torch.equal(out, again[0].cpu()) and torch.equal(dr, again[1].cpu()) and stat == again[3]
    nt = orc.loadest_ntheta(d)
    for b, (c, s) in enumerate(zip(cases, sites)):
        nb = s[0]
        one = base._plan("loadest", nb, d, gpu_device)
        o1, d1, f1, s1 = _fit_step(one, gpu_device, c)
        enll = abs(float(out[b, 0]) - float(o1[0])) / abs(float(o1[0]))
        g1 = o1[_lib.OUT_DTHETA:_lib.OUT_DTHETA + nt]
        edth = float((out[b, _lib.OUT_DTHETA:_lib.OUT_DTHETA + nt] - g1).abs().max() / g1.abs().max())
        edr = float((dr[b, :nb] - d1).abs().max() / d1.abs().max())
        ef = float((f_hat[b, :nb] - f1).abs().max())
        print(f"interval ragged batch, site {b} n={nb}: NLL {enll:.2e}, dtheta {edth:.2e}, dr {edr:.2e}, f {ef:.2e}, iterations {stat[b][0]:.0f}")
        assert enll <= 1e-11 and edth <= 1e-9 and edr <= 1e-9 and ef <= 1e-9
        assert stat[b][0] == s1[0] and stat[b][3] == 0 and int(out[b, _lib.OUT_INFO]) == 0
        ref = _reference(*s)
        assert abs(float(out[b, 0]) - ref["nll"]) <= 1e-10 * abs(ref["nll"]) and float(np.abs(f_hat[b, :nb].numpy() - ref["f"]).max()) <= 1e-9


def test_gradient_against_central_differences(gpu_device):
    n, d, frac, seed = 65, 2, 1.0, 265
    model, X, y, side, v, m, theta, upper = case = _case(n, d, frac, seed)
    plan = base._plan(model, n, d, gpu_device)
    out, _dr, _f, _stat = _fit_step(plan, gpu_device, case)
    got = out[_lib.OUT_DTHETA:_lib.OUT_DTHETA + plan.ntheta].numpy()
    h = 1e-4
    fd = np.zeros(plan.ntheta)
    for p in range(plan.ntheta):
        e = torch.zeros_like(theta)
        e[p] = h
        fd[p] = (ih.nll_of_theta(model, X, y, side, v, m, theta + e, upper) - ih.nll_of_theta(model, X, y, side, v, m, theta - e, upper)) / (2 * h)
    err = float(np.abs(got - fd).max() / np.abs(fd).max())
    print(f"interval gradient against central differences of the dense NLL (n = {n}): {err:.2e} of the largest entry")
    assert err <= 1e-6


def test_very_wide_brackets_are_one_sided_rows(gpu_device):
    """[l - 1e3 sigma, l] is "below l" and [l, l + 1e3 sigma] is "above l": Phi of the far end is exactly 0 or 1."""
    n, d = 129, 2
    X = torch.tensor(orc.synth_loadest(n, d, seed=51)[0])
    y, side, v, m = ch.synth(X.numpy(), 0.2, 51)
    assert (side == -1).any() and (side == 1).any()
    sg = np.sqrt(v)
    lo = np.where(side == -1, y - 1e3 * sg, y)
    up = np.where(side == -1, y, np.where(side == 1, y + 1e3 * sg, np.nan))
    theta = _theta(d)
    plan = base._plan("loadest", n, d, gpu_device)
    one = _fit_step(plan, gpu_device, ("loadest", X, y, side, v, m, theta, None), upper=None)
    two = _fit_step(plan, gpu_device, ("loadest", X, lo, np.where(side != 0, 2, 0).astype(np.int32), v, m, theta, up))
    nt = plan.ntheta
    ef = float((one[2] - two[2]).abs().max())
    enll = abs(float(one[0][0]) - float(two[0][0])) / abs(float(one[0][0]))
    g1 = one[0][_lib.OUT_DTHETA:_lib.OUT_DTHETA + nt]
    edth = float((two[0][_lib.OUT_DTHETA:_lib.OUT_DTHETA + nt] - g1).abs().max() / g1.abs().max())
    print(f"interval, brackets 1e3 sigma wide against one-sided rows: f {ef:.2e}, NLL {enll:.2e}, dtheta {edth:.2e}")
    assert ef <= 1e-12 and enll <= 1e-12 and edth <= 1e-12 and one[3][0] == two[3][0]


def test_very_narrow_brackets_are_observations(gpu_device):
    """Every row bracketed, 1e-4 sigma wide around y: the plain fit step on y up to Delta^2 / 12, the NLL shifted by -sum log w."""
    n, d = 129, 2
    X = torch.tensor(orc.synth_loadest(n, d, seed=52)[0])
    y, _side, v, m = ch.synth(X.numpy(), 0.2, 52)
    w = 1e-4 * np.sqrt(v)
    theta = _theta(d)
    plan = base._plan("loadest", n, d, gpu_device)
    plan.set_inputs(X.to(gpu_device).contiguous())
    yd, vd, md = _dev(gpu_device, y, v, m)
    out0, dr0, _dn = plan.fit_step(theta, (yd - md).contiguous(), vd)
    out0, f0 = out0.cpu().clone(), (yd - vd * dr0).cpu()
    out, _dr, f_hat, stat = _fit_step(plan, gpu_device, ("loadest", X, y - 0.5 * w, np.full(n, 2, dtype=np.int32), v, m, theta, y + 0.5 * w))
    nt = plan.ntheta
    ef = float((f_hat - f0).abs().max() / f0.abs().max())
    g0 = out0[_lib.OUT_DTHETA:_lib.OUT_DTHETA + nt]
    edth = float((out[_lib.OUT_DTHETA:_lib.OUT_DTHETA + nt] - g0).abs().max() / g0.abs().max())
    shift = float(out[_lib.OUT_NLL]) - float(out0[_lib.OUT_NLL])
    const = -float(np.log(w / np.sqrt(v)).sum()) - float(np.log(np.sqrt(v)).sum())
    enll = abs(shift - const) / abs(float(out0[_lib.OUT_NLL]))
    print(f"interval, brackets 1e-4 sigma wide against the plain fit step: f {ef:.2e}, dtheta {edth:.2e}, NLL shift {shift:.6f} "
          f"(-sum log w = {const:.6f}: {enll:.2e} of the NLL), iterations {stat[0]:.0f}, capped {stat[3]:.0f}")
    assert ef <= 1e-7 and edth <= 1e-7 and enll <= 1e-7 and stat[3] == 0


def test_no_bracketed_row_is_the_existing_entry_bitwise(gpu_device):
    n, d = 257, 3
    model, X, y, side, v, m, theta = base._case("loadest", n, d, 0.2, 12)
    plan = base._plan(model, n, d, gpu_device)
    plan.set_inputs(X.to(gpu_device).contiguous())
    yd, vd, md, sd = _dev(gpu_device, y, v, m, side)
    junk = torch.full((n,), float("nan"), dtype=torch.float64, device=gpu_device)  # read on rows of side 2 only
    bufs = (_lib.BUF_ALPHA, _lib.BUF_A, _lib.BUF_T, _lib.BUF_S, _lib.BUF_Z)
    o0, d0, f0, s0 = plan.laplace_fit_step(theta, yd, md, vd, sd, tol=TOL)
    keep0 = [t.clone() for t in (o0, d0, f0)] + [plan.buffer(b).clone() for b in bufs]
    o1, d1, f1, s1 = plan.laplace_fit_step(theta, yd, md, vd, sd, tol=TOL, upper=junk)
    keep1 = [o1, d1, f1] + [plan.buffer(b) for b in bufs]
    assert all(torch.equal(a, b) for a, b in zip(keep0, keep1)) and s0 == s1 and s0[0] >= 2
    # nothing censored at all: the plain step
    zero = torch.zeros(n, dtype=torch.int32, device=gpu_device)
    p0, pd0, _dn = plan.fit_step(theta, (yd - md).contiguous(), vd)
    p0, pd0 = p0.clone(), pd0.clone()
    p1, pd1, _f, st = plan.laplace_fit_step(theta, yd, md, vd, zero, tol=TOL, upper=junk)
    assert torch.equal(p0, p1) and torch.equal(pd0, pd1) and st == (0.0, 0.0, 0.0, 0.0)
    of0, ff0, _s = plan.laplace_factorize(theta, yd, md, vd, sd, tol=TOL)
    of0, ff0 = of0.clone(), ff0.clone()
    of1, ff1, _s = plan.laplace_factorize(theta, yd, md, vd, sd, tol=TOL, upper=junk)
    assert torch.equal(of0, of1) and torch.equal(ff0, ff1)


def _raw(plan, dev, case, side=None, upper="case", batched_ws=True):
    """``dgp_laplace_interval_fit_step`` through ctypes, as it is: -> (return code, error text)."""
    _model, _X, y, side0, v, m, theta, up = case
    lib = plan.lib
    yd, vd, md, sd = _dev(dev, y, v, m, side0 if side is None else side)
    ud = _dev(dev, up)[0] if isinstance(upper, str) else upper
    fd = md.clone()
    th = (C.c_double * len(theta))(*theta.tolist())
    need = max(int(lib.dgp_laplace_batched_workspace_bytes(plan._h)), 1 << 16)
    work = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    basep = work.data_ptr() + (-work.data_ptr()) % 256
    out = torch.zeros(_lib.OUT_LEN, dtype=torch.float64, device=dev)
    dr = torch.zeros(len(y), dtype=torch.float64, device=dev)
    stat = (C.c_double * 4)()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    with torch.cuda.device(dev):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.dgp_laplace_interval_fit_step(plan._h, th, ptr(yd), ptr(md), ptr(vd), ptr(sd), ptr(ud), ptr(fd), 50, TOL,
                                               C.c_void_p(basep), need, ptr(out), ptr(dr), stat, s)
        torch.cuda.synchronize(dev)
    return rc, lib.dgp_last_error().decode()


def test_error_rules(gpu_device):
    n, d = 129, 2
    case = _case(n, d, 0.2, 100 * d + n)
    plan = base._plan("loadest", n, d, gpu_device)
    plan.set_inputs(case[1].to(gpu_device).contiguous())
    rc, msg = _raw(plan, gpu_device, case)
    assert rc == 0, msg
    rc, msg = _raw(plan, gpu_device, case, upper=None)  # a row of side 2 and no upper_dev
    assert rc == _lib.E_ARG and "upper_dev" in msg
    row = int(np.flatnonzero(case[3] == 2)[0])
    for bad in (case[2][row], case[2][row] - 1.0, float("nan"), float("inf")):
        up = case[7].copy()
        up[row] = bad
        rc, msg = _raw(plan, gpu_device, case, upper=_dev(gpu_device, up)[0])
        assert rc == _lib.E_ARG and "bracket" in msg, (bad, rc, msg)
    side = case[3].copy()
    side[3] = 3
    rc, msg = _raw(plan, gpu_device, case, side=side)
    assert rc == _lib.E_ARG and "side" in msg
    rc, msg = _raw(base._plan("loadest", n, d, gpu_device, dtype=torch.float32), gpu_device, case)
    assert rc == _lib.E_ARG and "float64" in msg
    # the existing entries are unchanged: for them 2 is a bad side value
    yd, vd, md, sd = _dev(gpu_device, case[2], case[4], case[5], case[3])
    with pytest.raises(_lib.DGPError) as err:
        plan.laplace_fit_step(case[6], yd, md, vd, sd, tol=TOL)
    assert err.value.code == _lib.E_ARG
    # and the plan stays usable
    out, dr, f_hat, stat = _fit_step(plan, gpu_device, case)
    base._check_against(out, dr, f_hat, stat, _reference(n, d, 0.2, 100 * d + n), plan.ntheta, "interval after the errors")


def test_engine_fit_and_fit_many_with_brackets(gpu_device):
    """``LoadestGP.fit(censored=codes, target_upper=u)`` and ``fit_many(..., target_upper=[...])`` on the device: the products of
    the held factorisation equal those of the CPU engine over the dense restatement at the fitted hyperparameters (restored from
    the checkpoint, which carries the codes and the brackets; the bound of the one-sided engine test, 1e-8), and the batch lands
    where the solo fits land (the bound of the one-sided batched test, 1e-6 in the parameters)."""
    import io

    from discontinuum_amd import multisite_fit
    from discontinuum_amd.loadest_gp import LoadestGP, censoring_from_bounds
    from tests.flux_helpers import FluxOraclePlan, daily_loadest

    class RefPlan(ih.IntervalOraclePlan, FluxOraclePlan):
        pass

    class CpuRef(LoadestGP):
        _plan_factory = staticmethod(RefPlan)
        device = "cpu"

    def bounds(target, seed):
        vals = np.asarray(target.values, dtype=np.float64)
        rng = np.random.default_rng(seed)
        order = np.argsort(vals)
        low, high = vals.copy(), vals.copy()
        low[order[:6]], high[order[:6]] = 0.0, vals[order[6]]  # "< limit"
        for i in rng.choice(order[6:], size=12, replace=False):  # brackets of 10 % .. 60 % relative width
            w = rng.uniform(0.1, 0.6)
            low[i], high[i] = vals[i] * (1 - 0.4 * w), vals[i] * (1 + 0.6 * w)
        return censoring_from_bounds(low, type(target)(high, dims=target.dims, coords=target.coords, name=target.name, attrs=target.attrs))

    sites = [daily_loadest(n_obs=n, end="2014-01-01", seed=s) for n, s in ((80, 5), (61, 6))]
    args = [bounds(target, s) for s, (_cov, target, _daily) in enumerate(sites)]
    solos = []
    for (cov, _t, daily), (tgt, codes, upper) in zip(sites, args):
        m = LoadestGP()
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(len(solos))
            m.fit(cov, tgt, iterations=8, censored=codes, target_upper=upper)
        assert m._censor.upper is not None and m.laplace_status_[1] <= m.laplace_tol and (codes == 2).sum() == 12
        solos.append(m)
    (cov, _t, daily), (tgt, codes, upper), m = sites[0], args[0], solos[0]
    got = (m.predict(daily)[0].values, m.annual_flux(daily)["mean"].values)
    buf = io.BytesIO()
    m.save(buf)
    buf.seek(0)
    cpu = CpuRef.load(buf, cov, tgt)
    assert cpu._censor.side.tolist() == codes.tolist()
    ref = (cpu.predict(daily)[0].values, cpu.annual_flux(daily)["mean"].values)
    plain = LoadestGP()
    plain.fit(cov, tgt, iterations=8, censored=np.where(codes == 2, 0, codes))
    sub = (plain.predict(daily)[0].values, plain.annual_flux(daily)["mean"].values)
    for name, g, r, s in zip(("predict", "annual_flux"), got, ref, sub):
        err, moved = float(np.max(np.abs(g - r) / np.abs(r))), float(np.max(np.abs(g - s) / np.abs(s)))
        print(f"interval engine {name}: against the dense restatement {err:.2e}, against dropping the brackets {moved:.2e}")
        assert err <= 1e-8 and moved > 1e-4
    models = [LoadestGP() for _ in sites]
    multisite_fit.fit_many(models, [(c, a[0]) for (c, _t, _d), a in zip(sites, args)], iterations=8, site_seeds=[0, 1],
                           censored=[a[1] for a in args], target_upper=[a[2] for a in args])
    flat = lambda e: torch.cat([p.detach().reshape(-1).double() for _, p in sorted(e.model.named_parameters())])  # noqa: E731
    many = multisite_fit.predict_many(models, [d for _c, _t, d in sites])
    for b, (mb, solo) in enumerate(zip(models, solos)):
        diff = float((flat(mb) - flat(solo)).abs().max())
        mu1 = mb.predict(sites[b][2])[0].values
        pm = float(np.max(np.abs(many[b][0].values - mu1) / np.abs(mu1)))
        print(f"interval fit_many site {b}: parameters against the solo fit {diff:.2e}, predict_many against predict {pm:.2e}")
        assert diff <= 1e-6 and pm <= 1e-9 and mb._censor.upper is not None
