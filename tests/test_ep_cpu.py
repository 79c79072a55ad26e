"""Expectation propagation for censored fits, on the CPU: the dense restatement of tests/ep_helpers.py against itself (the two forms
of the value, the gradient against central differences of the re-converged value, a two-point case against quadrature, the
degenerate records) and the engine -- ``fit(approximation="ep")``, the products, the refusals, checkpoints -- over ``EPOraclePlan``.

Bounds.  The two forms of the value are the same number in exact arithmetic: 1e-12.  Central differences with step 1e-5 of a value
re-converged to 1e-13: truncation h^2 / 6 |NLL'''| ~ 1e-10 and rounding eps |NLL| / h ~ 1e-9 of the gradient's scale; the bound is
1e-6 of the largest entry.  The two-point case: what EP is known to deliver there (mean within 0.02 sd, sd within 5 %, -log Z
within 0.01), while Laplace's mean is more than half a standard deviation off."""
import io
import math
import os

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib, multisite_fit
from discontinuum_amd.loadest_gp import LoadestGP
from oracle import gp_oracle as orc
from tests import censored_helpers as ch
from tests import ep_helpers as eh
from tests import interval_helpers as ih
from tests.flux_helpers import daily_loadest
from tests.window_helpers import WindowOraclePlan

LN2 = 0.6931471805599453


def _record(n, d, frac, seed):
    X = torch.tensor(orc.synth_loadest(n, d, seed=seed)[0])
    y, side, v, m, upper = ih.synth(X.numpy(), frac, seed)
    theta = torch.full((orc.loadest_ntheta(d),), LN2, dtype=torch.float64) * torch.linspace(0.8, 1.3, orc.loadest_ntheta(d), dtype=torch.float64)
    return X, y, side, v, m, upper, theta


def test_abi_declares_the_ep_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "dgp_hip.h")).read()
    lib = _lib.load()
    for name in ("dgp_ep_workspace_bytes", "dgp_ep_fit_step", "dgp_ep_factorize", "dgp_ep_diag"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header, name
    step, fac = _lib.SIGNATURES["dgp_ep_fit_step"][1], _lib.SIGNATURES["dgp_ep_factorize"][1]
    assert len(step) == 22 and fac == step[:16] + step[17:]  # the same arguments without dr_dev


@pytest.mark.parametrize("n,frac,seed", [(40, 0.3, 1), (64, 0.6, 2), (128, 0.9, 3)])
def test_the_two_forms_of_the_value_agree(n, frac, seed):
    X, y, side, v, m, upper, theta = _record(n, 2, frac, seed)
    res = eh.ep_fit("loadest", X, y, side, v, m, theta, upper=upper, tol=1e-12)
    sweeps, d_mu, d_tau, _capped, held, ncens = res["stat"]
    assert res["converged"] and sweeps <= 40 and held == 0 and ncens == (side != 0).sum() and max(d_mu, d_tau) <= 1e-12
    assert (side == 2).any() and (side == -1).any() and (side == 1).any()
    assert abs(res["nll"] - res["nll_long"]) <= 1e-12 * abs(res["nll"])
    assert abs(res["nll_engine"] - res["nll_engine_oracle"]) <= 1e-12 * abs(res["nll_engine"])
    assert np.all(res["cav_var"] > 0) and np.all(res["nt"][side != 0] >= v[side != 0] * (1 - 1e-12))
    # k of the oracle's explicit gradient: 2 dnoise + alpha^2
    assert float(np.max(np.abs(2.0 * res["dnoise"] + res["dr"] ** 2 - res["k"]) / res["k"])) <= 1e-10
    # damped sweeps reach the same fixed point
    damped = eh.ep_fit("loadest", X, y, side, v, m, theta, upper=upper, tol=1e-12, damping=0.8, with_grad=False)
    assert damped["converged"] and damped["stat"][0] >= sweeps and float(np.max(np.abs(damped["mu"] - res["mu"]))) <= 1e-9


def test_gradient_against_central_differences_of_the_reconverged_value():
    n, d = 40, 2
    X, y, side, v, m, upper, theta = _record(n, d, 0.3, 5)
    assert (side == 2).any() and (side == -1).any() and (side == 1).any() and 10 <= (side != 0).sum() <= 14
    res = eh.ep_fit("loadest", X, y, side, v, m, theta, upper=upper, tol=1e-13, maxit=400)
    assert res["converged"]
    h = 1e-5
    fd = np.zeros(len(theta))
    for p in range(len(theta)):
        e = torch.zeros_like(theta)
        e[p] = h
        fd[p] = (eh.nll_of("loadest", X, y, side, v, m, theta + e, upper) - eh.nll_of("loadest", X, y, side, v, m, theta - e, upper)) / (2 * h)
    err = float(np.abs(res["dtheta"] - fd).max() / np.abs(fd).max())
    # the constant mean: d NLL / d c = -sum dr
    fdm = (eh.nll_of("loadest", X, y, side, v, m + h, theta, upper) - eh.nll_of("loadest", X, y, side, v, m - h, theta, upper)) / (2 * h)
    errm = abs(-res["dr"].sum() - fdm) / max(abs(fdm), np.abs(res["dr"]).max())
    print(f"EP gradient against central differences (n = {n}): dtheta {err:.2e}, mean {errm:.2e}")
    assert err <= 1e-6 and errm <= 1e-6


def test_two_points_against_quadrature():
    from scipy import integrate, stats

    K = np.array([[1.0, 0.8], [0.8, 1.0]])
    lim, v, m = np.array([-1.0, -1.5]), np.full(2, 0.01), np.zeros(2)
    side = np.array([-1, -1], dtype=np.int32)
    prior = stats.multivariate_normal(mean=m, cov=K)
    sg = np.sqrt(v)

    def moment(p):
        f = lambda f1, f0: f0 ** p * prior.pdf([f0, f1]) * stats.norm.cdf((lim[0] - f0) / sg[0]) * stats.norm.cdf((lim[1] - f1) / sg[1])  # noqa: E731
        return integrate.dblquad(f, -8.0, 4.0, -8.0, 4.0, epsabs=1e-12, epsrel=1e-10)[0]

    Z = moment(0)
    mean = moment(1) / Z
    sd = math.sqrt(moment(2) / Z - mean * mean)
    res = eh.ep(K, lim, side, v, m, tol=1e-12)
    Sigma = K - K @ np.linalg.solve(K + np.diag(res["nt"]), K)
    ep_mean, ep_sd = float(res["mu"][0]), float(np.sqrt(Sigma[0, 0]))
    f_lap = ch.newton(K, lim, side, v, m, tol=1e-12)[0]
    print(f"two points: quadrature mean {mean:.4f} sd {sd:.4f} -log Z {-math.log(Z):.4f}; EP {ep_mean:.4f} {ep_sd:.4f} {res['nll']:.4f}; "
          f"Laplace mean {f_lap[0]:.4f}")
    assert abs(mean + 1.7857) <= 2e-4 and abs(sd - 0.5286) <= 2e-4 and abs(-math.log(Z) - 2.9363) <= 2e-4  # the quadrature itself
    assert res["converged"] and abs(ep_mean - mean) <= 0.02 * sd and abs(ep_sd - sd) <= 0.05 * sd and abs(res["nll"] + math.log(Z)) <= 0.01
    assert abs(res["nll"] - res["nll_long"]) <= 1e-12
    assert abs(f_lap[0] - mean) > 0.5 * sd


def test_degenerate_records():
    X, y, side, v, m, upper, theta = _record(40, 2, 1.0, 7)
    assert (side != 0).all()
    res = eh.ep_fit("loadest", X, y, side, v, m, theta, upper=upper, tol=1e-12)
    assert res["converged"] and res["stat"][5] == 40 and res["stat"][4] == 0 and abs(res["nll"] - res["nll_long"]) <= 1e-12 * abs(res["nll"])
    # no censored row: no sweep, the plain NLL, the sites are the data
    none = np.zeros(40, dtype=np.int32)
    res = eh.ep_fit("loadest", X, y, none, v, m, theta, upper=upper)
    plain = orc.nll_data_and_grads("loadest", X, torch.tensor(y - m), torch.tensor(v), theta)
    assert res["stat"] == (0.0,) * 6 and res["converged"] and np.array_equal(res["yt"], y) and np.array_equal(res["nt"], v)
    assert abs(res["nll"] - float(plain[0])) <= 1e-12 * abs(float(plain[0])) and np.allclose(res["dtheta"], plain[1].numpy(), rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match="damping"):
        eh.ep(np.eye(2), np.zeros(2), np.array([-1, 0]), np.ones(2), np.zeros(2), damping=0.0)


class _Plan(eh.EPOraclePlan, WindowOraclePlan):
    pass


@pytest.fixture()
def cpu_engine(monkeypatch):
    monkeypatch.setattr(LoadestGP, "_plan_factory", staticmethod(_Plan))
    monkeypatch.setattr(LoadestGP, "device", "cpu")
    monkeypatch.setattr(multisite_fit, "GPPlan", ih.BatchedIntervalOraclePlan)
    return LoadestGP


def _non_detects(target, k):
    vals = np.asarray(target.values, dtype=np.float64)
    order = np.argsort(vals)
    mask = np.zeros(len(vals), dtype=bool)
    mask[order[:k]] = True
    reported = vals.copy()
    reported[mask] = vals[order[k]]
    return type(target)(reported, dims=target.dims, coords=target.coords, name=target.name, attrs=target.attrs), mask


def test_engine_fit_products_refusals_and_checkpoint(cpu_engine):
    cov_obs, target, daily = daily_loadest(n_obs=40, end="2014-01-01", seed=5)
    reported, mask = _non_detects(target, 16)
    with pytest.raises(ValueError, match="approximation"):
        cpu_engine().fit(cov_obs, reported, iterations=1, censored=mask, approximation="vb")
    m = cpu_engine()
    values = []
    real = m.__class__._record_censor_status

    def spy(self):
        real(self)
        values.append(self._plan.ep_stat)

    m.__class__._record_censor_status, keep = spy, real
    try:
        m.fit(cov_obs, reported, iterations=12, censored=mask, approximation="ep", scheduler=False)
    finally:
        m.__class__._record_censor_status = keep
    assert m._censor.approximation == "ep" and m._plan.ep_calls == 12 and getattr(m._plan, "laplace_calls", 0) == 0
    sweeps, d_mu, d_tau, _capped, held, ncens = m.ep_status_
    assert ncens == 16 and held == 0 and max(d_mu, d_tau) <= m.laplace_tol and m.laplace_status_ is None
    assert len(values) == 12 and all(1 <= st[0] <= m.ep_maxit for st in values) and m._censor.sites is not None  # (warm-started)
    # the objective falls
    with torch.no_grad():
        theta = m._theta_fn().detach()
        mean = m.model.prior_mean(m._train_x).numpy()
    fresh = cpu_engine()
    fresh.fit(cov_obs, reported, iterations=1, censored=mask, approximation="ep", scheduler=False)
    with torch.no_grad():
        theta0, mean0 = fresh._theta_fn().detach(), fresh.model.prior_mean(fresh._train_x).numpy()
    args = (m._train_x, m._train_y.numpy(), m._censor.side.numpy(), np.full(40, 0.01))
    nll_end = eh.ep_fit("loadest", *args, mean, theta, with_grad=False)["nll"]
    nll_start = eh.ep_fit("loadest", *args, mean0, theta0, with_grad=False)["nll"]
    assert nll_end < nll_start - 1e-3
    # the products read the EP posterior: one ep_factorize builds the cache, then nothing more
    calls = m._plan.ep_calls
    mu_d, se_d = m.predict(daily)
    flux = m.annual_flux(daily)
    tau = float(np.quantile(np.asarray(target.values), 0.6))
    exc = m.exceedance(daily, threshold=tau)
    roll = m.rolling_mean(daily, window=30)
    assert m._plan.ep_calls == calls + 1 and getattr(m._plan, "laplace_calls", 0) == 0
    for out in (mu_d.values, se_d.values, flux["mean"].values, exc["mean"].values, roll["mean"].values):
        assert np.all(np.isfinite(np.asarray(out, dtype=np.float64)))
    Xs = torch.tensor(m.dm.Xnew(cov_obs), dtype=torch.float64)
    mu, var = m._model_space_predict(Xs)
    res = eh.ep_fit("loadest", *args, mean, theta, tol=1e-12, with_grad=False)
    ref_mu, ref_var = eh.posterior("loadest", m._train_x, res, Xs)
    assert torch.allclose(mu, ref_mu + float(mean[0]), rtol=0, atol=1e-8)
    assert torch.allclose(var, ref_var + m.likelihood.predictive_noise(40, Xs.device, torch.float64), rtol=0, atol=1e-8)
    # ... which is not the Laplace posterior at the same hyperparameters: the EP means of the non-detects lie further below the limit
    lap = ih.laplace("loadest", *args, mean, theta, tol=1e-12, with_grad=False)
    cens = m._censor.side.numpy() != 0
    gap = lap["f"][cens] - res["mu"][cens]
    assert float(np.max(gap)) > 0.1 and float(np.mean(gap)) > 0.05 and float(np.min(gap)) > -0.01
    # refusals
    refused = {
        "cross_validate": lambda: m.cross_validate(),
        "cross_validate cavity": lambda: m.cross_validate(laplace="cavity"),
        "flux_bias cavity": lambda: m.flux_bias(laplace="cavity"),
        "influence": lambda: m.influence(cov_obs, np.ones(40)),
        "hyperparameter_uncertainty": lambda: m.hyperparameter_uncertainty(),
        "predict_marginalized": lambda: m.predict_marginalized(cov_obs),
        "annual_flux": lambda: m.annual_flux(daily, hyperparameters=True),
    }
    for name, call in refused.items():
        with pytest.raises(NotImplementedError, match="censored|approximation"):
            call()
    with pytest.raises(NotImplementedError, match="Laplace MODE"):
        m.cross_validate(laplace="cavity")
    with pytest.raises(NotImplementedError, match="single-site"):
        multisite_fit.fit_many([cpu_engine()], [(cov_obs, reported)], iterations=1, censored=[mask], approximation="ep")
    with pytest.raises(NotImplementedError, match="single-site"):
        multisite_fit.fit_many_distributed([cpu_engine()], [(cov_obs, reported)], iterations=1, censored=[mask], approximation="ep")
    with pytest.raises(NotImplementedError, match="EP hyperparameters"):
        multisite_fit.predict_many([m], [cov_obs])
    # a checkpoint carries the approximation; one written before it existed loads as Laplace
    buf = io.BytesIO()
    m.save(buf)
    buf.seek(0)
    back = cpu_engine.load(buf, cov_obs, reported)
    assert back._censor.approximation == "ep" and back._censor.side.tolist() == m._censor.side.tolist()
    b = back._model_space_predict(Xs)
    assert back._plan.ep_calls == 1 and torch.allclose(mu, b[0], rtol=0, atol=1e-8) and torch.allclose(var, b[1], rtol=0, atol=1e-8)
    buf.seek(0)
    record = torch.load(buf, weights_only=True)
    assert record.pop("approximation") == "ep"
    old = io.BytesIO()
    torch.save(record, old)
    old.seek(0)
    legacy = cpu_engine.load(old, cov_obs, reported)
    assert legacy._censor.approximation == "laplace"
    legacy._model_space_predict(Xs)
    assert legacy._plan.laplace_calls == 1 and getattr(legacy._plan, "ep_calls", 0) == 0
    buf.seek(0)
    assert cpu_engine.load(buf, cov_obs, reported, approximation="laplace")._censor.approximation == "laplace"


def test_without_the_keyword_nothing_changes(cpu_engine):
    """``fit(censored=...)`` without the keyword (and with "laplace" / None) makes exactly the calls it made before; "ep" without a
    censored row is the plain fit."""
    cov_obs, target, _daily = daily_loadest(n_obs=40, end="2014-01-01", seed=5)
    reported, mask = _non_detects(target, 8)
    params = []
    for kw in ({}, {"approximation": "laplace"}, {"approximation": None}):
        torch.manual_seed(0)
        m = cpu_engine()
        m.fit(cov_obs, reported, iterations=6, censored=mask, **kw)
        assert m._plan.laplace_calls == 6 and getattr(m._plan, "ep_calls", 0) == 0 and m._censor.approximation == "laplace"
        assert m.ep_status_ is None and m.laplace_status_ is not None
        m.predict(cov_obs)
        assert m._plan.laplace_calls == 7 and getattr(m._plan, "ep_calls", 0) == 0
        params.append(torch.cat([p.detach().reshape(-1) for p in m.model.parameters()]))
    assert torch.equal(params[0], params[1]) and torch.equal(params[0], params[2])
    plain = []
    for kw in ({}, {"approximation": "ep"}):
        torch.manual_seed(0)
        m = cpu_engine()
        m.fit(cov_obs, reported, iterations=4, **kw)
        assert m._censor is None and getattr(m._plan, "ep_calls", 0) == 0 and getattr(m._plan, "laplace_calls", 0) == 0
        plain.append(torch.cat([p.detach().reshape(-1) for p in m.model.parameters()]))
    assert torch.equal(plain[0], plain[1])
