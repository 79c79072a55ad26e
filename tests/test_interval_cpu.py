"""Interval-censored observations without a GPU: the dense restatement of tests/interval_helpers.py against the 600-digit
fixture and against central differences, the C ABI's declarations, ``censoring_from_bounds``, and the engine's host side --
``fit(censored=codes, target_upper=u)``, predict, annual_flux, checkpointing, the pipeline / swap / midpoint rules,
``fit_many(target_upper=)`` and the unchanged refusals -- over the interval-aware oracle plan."""
import io
import os

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from discontinuum_amd.engines.hip import MIDPOINT_WIDTH, bracket_ends, censor_sides
from discontinuum_amd.loadest_gp import LoadestGP, censoring_from_bounds
from oracle import gp_oracle as orc
from tests import censored_helpers as ch
from tests import interval_helpers as ih
from tests.flux_helpers import FluxOraclePlan, daily_loadest
from tests.helpers import loadest_dataset

LN2 = 0.6931471805599453
NFAR = 24


def test_helper_pointwise_against_the_600_digit_fixture():
    """The bounds of the device test: 1e-13 (log P, sigma g), 1e-11 (W v), 1e-9 (sigma^3 d3), relative to max(1, |reference|)."""
    data = np.load(os.path.join(os.path.dirname(__file__), "golden", "interval_terms.npy"))
    za, delta, ref = data[0], data[1], data[2:]
    got = ih.interval_pointwise(za, delta)
    near = slice(0, len(za) - NFAR)
    err = [float(np.max((np.abs(got[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k])))[near])) for k in range(4)]
    assert err[0] <= 1e-13 and err[1] <= 1e-13 and err[2] <= 1e-11 and err[3] <= 1e-9, err
    assert np.all(np.isfinite(np.array(got))) and np.all((got[2] > 0) & (got[2] <= 1))
    # the derivative chain of the four functions, by central differences in f (za -> za - s, Delta fixed)
    z, d, s = np.array([-3.0, -0.4, 0.2, 2.5, -6.0]), np.array([0.3, 1.0, 5.0, 0.01, 8.0]), 1e-5
    lo, mid, hi = ih.interval_pointwise(z + s, d), ih.interval_pointwise(z, d), ih.interval_pointwise(z - s, d)
    assert np.allclose((hi[0] - lo[0]) / (2 * s), mid[1], rtol=0, atol=1e-8)    # d log P / d f = g
    assert np.allclose(-(hi[1] - lo[1]) / (2 * s), mid[2], rtol=0, atol=1e-8)   # -d g / d f = W
    assert np.allclose(-(hi[2] - lo[2]) / (2 * s), mid[3], rtol=0, atol=1e-8)   # -d W / d f = d3


def _fixture(n=40, d=2, seed=3):
    X, _y = orc.synth_loadest(n, d, seed=seed)
    y, side, v, m, upper = ih.synth(X, 0.3, seed)
    assert (side == -1).any() and (side == 1).any() and (side == 2).any()
    theta = torch.full((orc.loadest_ntheta(d),), LN2, dtype=torch.float64)
    theta = theta * torch.linspace(0.8, 1.3, theta.numel(), dtype=torch.float64)
    return torch.tensor(X), y, side, v, m, theta, upper


def test_helper_gradients_against_central_differences():
    X, y, side, v, m, theta, upper = _fixture()
    res = ih.laplace("loadest", X, y, side, v, m, theta, upper=upper, tol=1e-12)
    assert res["converged"] and res["capped"] == 0 and 2 <= res["iterations"] <= 30
    # the mode is a stationary point: grad log p = K^-1 (f - m) = a
    assert np.max(np.abs(res["terms"]["g"] - res["alpha"])) < 1e-8
    step = 1e-5
    for p in range(theta.numel()):
        e = torch.zeros_like(theta)
        e[p] = step
        fd = (ih.nll_of_theta("loadest", X, y, side, v, m, theta + e, upper) - ih.nll_of_theta("loadest", X, y, side, v, m, theta - e, upper)) / (2 * step)
        assert abs(fd - res["dtheta"][p]) <= 1e-6 * max(1.0, abs(fd)), (p, fd, res["dtheta"][p])
    # without a bracketed row the helper is censored_helpers' own
    one = np.where(side == 2, -1, side)
    a, b = ih.laplace("loadest", X, y, one, v, m, theta, upper=upper), ch.laplace("loadest", X, y, one, v, m, theta)
    assert a["nll"] == b["nll"] and np.array_equal(a["f"], b["f"])


def test_scalar_mode_by_bisection():
    X = torch.tensor([[0.3, -0.2]])
    theta = torch.full((orc.loadest_ntheta(2),), LN2, dtype=torch.float64)
    for lo, hi in ((-0.4, -0.35), (0.2, 0.9), (0.05, 0.0501)):
        res = ih.laplace("loadest", X, np.array([lo]), np.array([2]), np.array([0.01]), np.array([0.1]), theta, upper=np.array([hi]), tol=1e-13)
        ref = ih.scalar_mode(float(res["K"][0, 0]), lo, hi, 0.01, 0.1)
        assert res["converged"] and abs(res["f"][0] - ref) < 1e-11, (res["f"], ref)


def test_abi_declares_the_interval_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "dgp_hip.h")).read()
    lib = _lib.load()
    for name in ("dgp_laplace_interval_fit_step", "dgp_laplace_interval_factorize", "dgp_debug_interval_terms"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header, name
    vp = _lib.SIGNATURES["dgp_laplace_batched_fit_step"][1][0]
    batched, interval = _lib.SIGNATURES["dgp_laplace_batched_fit_step"][1], _lib.SIGNATURES["dgp_laplace_interval_fit_step"][1]
    assert interval == batched[:6] + [vp] + batched[6:]  # dgp_laplace_batched_*'s arguments plus upper_dev after side_dev
    batched, interval = _lib.SIGNATURES["dgp_laplace_batched_factorize"][1], _lib.SIGNATURES["dgp_laplace_interval_factorize"][1]
    assert interval == batched[:6] + [vp] + batched[6:]


def test_censoring_from_bounds():
    nan, inf = float("nan"), float("inf")
    low = np.array([nan, 0.0, -1.0, 2.0, 3.0, 1.5, 0.5])
    high = np.array([0.7, 0.8, 0.9, nan, inf, 1.5, 0.9])
    target, censored, upper = censoring_from_bounds(low, high)
    assert censored.tolist() == [-1, -1, -1, 1, 1, 0, 2] and censored.dtype == np.int32
    assert target.tolist() == [0.7, 0.8, 0.9, 2.0, 3.0, 1.5, 0.5]
    assert np.isnan(upper[:6]).all() and upper[6] == 0.9
    # no bracketed row: no upper ends; labelled arrays keep their metadata
    _cov, tgt = loadest_dataset(5)
    vals = np.asarray(tgt.values)
    t2, c2, u2 = censoring_from_bounds(np.where(np.arange(5) == 1, 0.0, vals), tgt)
    assert u2 is None and c2.tolist() == [0, -1, 0, 0, 0] and type(t2) is type(tgt) and t2.dims == tgt.dims and np.array_equal(t2.values, vals)
    with pytest.raises(ValueError, match="neither"):
        censoring_from_bounds([nan], [nan])
    with pytest.raises(ValueError, match="low > high"):
        censoring_from_bounds([2.0], [1.0])
    with pytest.raises(ValueError, match="align"):
        censoring_from_bounds([1.0, 2.0], [1.0])


def test_code_two_needs_target_upper():
    assert censor_sides([0, 2, -1], 3, bracketed=True).tolist() == [0, 2, -1]
    with pytest.raises(ValueError, match="target_upper"):
        censor_sides([0, 2, 0], 3)
    with pytest.raises(ValueError, match="-1"):
        censor_sides([0, 3, 0], 3, bracketed=True)


def test_bracket_ends_sorts_and_applies_the_midpoint_rule():
    side = np.array([2, 2, 2, -1, 0], dtype=np.int32)
    y = np.array([0.5, 1.0, 0.2, 0.3, 0.4])
    up = np.array([0.1, 1.0 + 0.5e-6 * 0.1, 0.6, np.nan, np.nan])
    s, yy, u = bracket_ends(side, y, up, np.full(5, 0.1))
    assert s.tolist() == [2, 0, 2, -1, 0]
    assert yy[0] == 0.1 and u[0] == 0.5                      # a decreasing transform's ends, sorted
    assert yy[1] == 0.5 * (1.0 + (1.0 + 0.5e-6 * 0.1)) and np.isnan(u[1])  # narrower than 1e-6 sigma: its midpoint, observed
    assert yy[2] == 0.2 and u[2] == 0.6 and np.isnan(u[3:]).all() and np.array_equal(yy[3:], y[3:])
    s, yy, u = bracket_ends(np.array([2, 0]), np.array([1.0, 2.0]), np.array([1.0, np.nan]), np.full(2, 0.1))
    assert s.tolist() == [0, 0] and u is None and yy.tolist() == [1.0, 2.0]
    assert MIDPOINT_WIDTH == 1e-6
    with pytest.raises(ValueError, match="finite"):
        bracket_ends(np.array([2]), np.array([1.0]), np.array([np.nan]), np.full(1, 0.1))


class _Plan(ih.IntervalOraclePlan, FluxOraclePlan):
    pass


@pytest.fixture()
def cpu_engine(monkeypatch):
    from discontinuum_amd import multisite_fit

    monkeypatch.setattr(LoadestGP, "_plan_factory", staticmethod(_Plan))
    monkeypatch.setattr(LoadestGP, "device", "cpu")
    monkeypatch.setattr(multisite_fit, "GPPlan", ih.BatchedIntervalOraclePlan)
    monkeypatch.setattr(ih.BatchedIntervalOraclePlan, "laplace_calls_total", 0)
    return LoadestGP


def _bounds(target, seed=1, k2=6, kminus=3, kplus=2):
    """EGRET-style (low, high) from a record: ``k2`` samples reported as brackets of 20 % .. 60 % relative width, the ``kminus``
    smallest as "< limit" (low = 0), ``kplus`` of the largest as "> limit" (high missing), the rest observed."""
    vals = np.asarray(target.values, dtype=np.float64)
    rng = np.random.default_rng(seed)
    order = np.argsort(vals)
    low, high = vals.copy(), vals.copy()
    low[order[:kminus]], high[order[:kminus]] = 0.0, vals[order[kminus]]
    low[order[-kplus:]], high[order[-kplus:]] = vals[order[-kplus - 1]], np.nan
    for i in rng.choice(order[kminus:-kplus], size=k2, replace=False):
        w = rng.uniform(0.2, 0.6)
        low[i], high[i] = vals[i] * (1 - 0.4 * w), vals[i] * (1 + 0.6 * w)
    wrap = lambda a: type(target)(a, dims=target.dims, coords=target.coords, name=target.name, attrs=getattr(target, "attrs", {}))  # noqa: E731
    return wrap(low), wrap(high)


def test_engine_fit_with_brackets_predicts_the_laplace_posterior(cpu_engine):
    cov, target = loadest_dataset(40, seed=2)
    low, high = _bounds(target)
    tgt, codes, upper = censoring_from_bounds(low, high)
    assert sorted(set(codes.tolist())) == [-1, 0, 1, 2] and (codes == 2).sum() == 6
    with pytest.raises(ValueError, match="target_upper"):
        cpu_engine().fit(cov, tgt, iterations=1, censored=codes)
    with pytest.raises(ValueError, match="align"):
        cpu_engine().fit(cov, tgt, iterations=1, censored=codes, target_upper=upper[:-1])
    m = cpu_engine()
    m.fit(cov, tgt, iterations=10, censored=codes, target_upper=upper)
    assert m._censor is not None and m._censor.upper is not None and m._plan.interval_calls >= 10
    assert m._censor.side.tolist() == codes.tolist() and m._prior().upper is m._censor.upper
    it, dmax, _halvings, capped = m.laplace_status_
    assert 1 <= it <= 30 and dmax <= m.laplace_tol and capped == 0
    # the upper ends went through the target pipeline as fitted on the target
    br = codes == 2
    ref_upper = np.asarray(m.dm.target_pipeline.transform(high)).reshape(-1)
    assert np.array_equal(m._censor.upper.numpy()[br], ref_upper[br]) and np.all(m._censor.upper.numpy()[br] > m._train_y.numpy()[br])
    assert np.array_equal(m._train_y.numpy(), m.dm.y)
    # predict: the helper's Laplace posterior at the fitted hyperparameters, in model space
    Xs = torch.tensor(m.dm.Xnew(cov), dtype=torch.float64)
    mu, var = m._model_space_predict(Xs)
    with torch.no_grad():
        theta = m._theta_fn().detach()
        mean = m.model.prior_mean(m._train_x).numpy()
    res = ih.laplace("loadest", m._train_x, m._train_y.numpy(), codes, np.full(40, 0.01), mean, theta, upper=m._censor.upper.numpy(), tol=1e-12)
    ref_mu, ref_var = ch.posterior("loadest", m._train_x, res, Xs)
    assert torch.allclose(mu, ref_mu + float(mean[0]), rtol=0, atol=1e-8)
    assert torch.allclose(var, ref_var + m.likelihood.predictive_noise(40, Xs.device, torch.float64), rtol=0, atol=1e-8)
    # ... which is not the fit that takes the lower ends for samples and drops the brackets
    plain = cpu_engine()
    plain.fit(cov, tgt, iterations=10, censored=np.where(br, 0, codes))
    assert float((plain._model_space_predict(Xs)[0] - mu).abs().max()) > 1e-3
    mu_d, se_d = m.predict(cov)
    assert np.all(np.isfinite(mu_d.values)) and np.all(np.isfinite(se_d.values))
    # a checkpoint carries the codes and the brackets
    buf = io.BytesIO()
    m.save(buf)
    buf.seek(0)
    back = cpu_engine.load(buf, cov, tgt)
    assert back._censor.side.tolist() == codes.tolist() and np.array_equal(back._censor.upper.numpy()[br], m._censor.upper.numpy()[br])
    b = back._model_space_predict(Xs)
    assert torch.allclose(mu, b[0], rtol=0, atol=1e-9) and torch.allclose(var, b[1], rtol=0, atol=1e-9)
    buf.seek(0)
    other = upper.copy()
    other[br] *= 1.5
    wider = cpu_engine.load(buf, cov, tgt, target_upper=other)  # an explicit argument outranks the saved brackets
    assert np.all(wider._censor.upper.numpy()[br] > back._censor.upper.numpy()[br])


def test_annual_flux_reads_the_laplace_posterior(cpu_engine):
    cov_obs, target, daily = daily_loadest(n_obs=40, end="2014-01-01", seed=5)
    low, high = _bounds(target, seed=2)
    tgt, codes, upper = censoring_from_bounds(low, high)
    m = cpu_engine()
    m.fit(cov_obs, tgt, iterations=6, censored=codes, target_upper=upper)
    calls = m._plan.interval_calls
    flux = m.annual_flux(daily)
    assert m._plan.interval_calls == calls + 1  # the cache build: one laplace_factorize with the brackets
    assert np.all(np.isfinite(flux["mean"].values)) and np.all(flux["mean"].values > 0)
    plain = cpu_engine()
    plain.fit(cov_obs, tgt, iterations=6, censored=np.where(codes == 2, 0, codes))
    other = plain.annual_flux(daily)["mean"].values
    assert float(np.max(np.abs(flux["mean"].values - other) / other)) > 1e-4
    # the refusals stay exactly as they are
    refused = {
        "cross_validate": lambda: m.cross_validate(),
        "influence": lambda: m.influence(cov_obs, np.ones(40)),
        "hyperparameter_uncertainty": lambda: m.hyperparameter_uncertainty(),
        "predict_marginalized": lambda: m.predict_marginalized(cov_obs),
        "annual_flux": lambda: m.annual_flux(daily, hyperparameters=True),
    }
    for name, call in refused.items():
        with pytest.raises(NotImplementedError, match="censored"):
            call()


def test_midpoint_rule(cpu_engine):
    """Brackets narrower than 1e-6 sigma are observations at their midpoints: no Laplace call, the plain fit on the midpoints."""
    cov, target = loadest_dataset(30, seed=7)
    vals = np.asarray(target.values, dtype=np.float64)
    codes = np.zeros(30, dtype=np.int32)
    codes[[2, 11, 20]] = 2
    low = np.where(codes == 2, vals * (1 - 1e-9), vals)
    high = np.where(codes == 2, vals * (1 + 1e-9), np.nan)
    wrap = lambda a: type(target)(a, dims=target.dims, coords=target.coords, name=target.name, attrs=getattr(target, "attrs", {}))  # noqa: E731
    m = cpu_engine()
    m.fit(cov, wrap(low), iterations=4, censored=codes, target_upper=high)
    assert m._censor is None and getattr(m._plan, "laplace_calls", 0) == 0
    mid = m._train_y.numpy()
    lo_m = np.asarray(m.dm.target_pipeline.transform(wrap(low))).reshape(-1)
    hi_m = np.asarray(m.dm.target_pipeline.transform(wrap(np.where(codes == 2, high, low)))).reshape(-1)
    assert np.array_equal(mid, np.where(codes == 2, 0.5 * (lo_m + hi_m), lo_m)) and np.array_equal(m.model_space_targets(), mid)
    # one bracket wide enough keeps its code; the narrow ones still become observations
    high2 = high.copy()
    high2[11] = vals[11] * 1.3
    m2 = cpu_engine()
    m2.fit(cov, wrap(low), iterations=2, censored=codes, target_upper=high2)
    assert m2._censor.side.tolist() == np.where(np.arange(30) == 11, 2, 0).tolist() and m2._plan.interval_calls >= 2


def test_decreasing_transform_swaps_the_ends(cpu_engine):
    from discontinuum_amd import pipeline as pl

    class Negate(pl._Step):
        def transform(self, X):
            return -X

        inverse_transform = transform

    class NegLogPipeline(pl.Pipeline):
        def __init__(self):
            super().__init__([("metadata", pl.MetadataManager()), ("log", pl.LogTransformer()), ("negate", Negate()),
                              ("scale", pl.StandardScaler())])

    cov, target = loadest_dataset(30, seed=8)
    low, high = _bounds(target, seed=3, k2=5, kminus=1, kplus=1)
    tgt, codes, upper = censoring_from_bounds(low, high)
    br = codes == 2
    codes = np.where(br, 2, 0)  # (one-sided codes keep their meaning in DATA space; here only the brackets matter)
    m = cpu_engine()
    m.dm.target_pipeline = NegLogPipeline
    m.fit(cov, tgt, iterations=3, censored=codes, target_upper=upper)
    lo_m = np.asarray(m.dm.target_pipeline.transform(tgt)).reshape(-1)
    hi_m = np.asarray(m.dm.target_pipeline.transform(high)).reshape(-1)
    assert np.all(hi_m[br] < lo_m[br])  # the pipeline decreases
    assert np.array_equal(m._train_y.numpy()[br], hi_m[br]) and np.array_equal(m._censor.upper.numpy()[br], lo_m[br])
    assert np.array_equal(m._train_y.numpy()[~br], lo_m[~br]) and m._plan.interval_calls >= 3
    assert m.laplace_status_[1] <= m.laplace_tol


def _flat(m):
    return torch.cat([p.detach().reshape(-1).double() for _, p in sorted(m.model.named_parameters())])


def test_fit_many_with_brackets_equals_the_per_site_fits(cpu_engine):
    from discontinuum_amd import multisite_fit

    sizes, data, codes, uppers = (30, 24, 36), [], [], []
    for i, n in enumerate(sizes):
        cov, target = loadest_dataset(n, seed=20 + i)
        if i == 1:  # a site without a censored row rides along
            data.append((cov, target))
            codes.append(None)
            uppers.append(None)
            continue
        low, high = _bounds(target, seed=i, k2=4, kminus=2, kplus=1)
        tgt, c, u = censoring_from_bounds(low, high)
        data.append((cov, tgt))
        codes.append(c)
        uppers.append(u)
    seeds = [0, 1, 2]
    models = [cpu_engine() for _ in sizes]
    multisite_fit.fit_many(models, data, iterations=6, site_seeds=seeds, censored=codes, target_upper=uppers)
    assert ih.BatchedIntervalOraclePlan.laplace_calls_total == 6
    for b, (m, (cov, tgt)) in enumerate(zip(models, data)):
        solo = cpu_engine()
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seeds[b])
            solo.fit(cov, tgt, iterations=6, censored=codes[b], target_upper=uppers[b])
        assert float((_flat(m) - _flat(solo)).abs().max()) <= 1e-6, b  # the bound of the one-sided batched test
        if codes[b] is None:
            assert m._censor is None
            continue
        br = codes[b] == 2
        assert m._censor.side.tolist() == codes[b].tolist() and m._censor.f is not None
        assert np.array_equal(m._censor.upper.numpy()[br], solo._censor.upper.numpy()[br])
        mu, se = m.predict(cov)
        mu1, se1 = solo.predict(cov)
        assert np.allclose(mu.values, mu1.values, rtol=1e-5, atol=0) and np.allclose(se.values, se1.values, rtol=1e-5, atol=0)
    # predict_many builds ONE batched cache with the brackets and agrees with the models' own predictions
    calls = ih.BatchedIntervalOraclePlan.laplace_calls_total
    got = multisite_fit.predict_many(models, [cov for cov, _ in data])
    assert ih.BatchedIntervalOraclePlan.laplace_calls_total == calls + 1
    for m, (cov, _), (mu, se) in zip(models, data, got):
        mu1, se1 = m.predict(cov)
        assert np.allclose(mu.values, mu1.values, rtol=1e-9, atol=0) and np.allclose(se.values, se1.values, rtol=1e-9, atol=0)
    with pytest.raises(ValueError, match="one entry per site"):
        multisite_fit.fit_many([cpu_engine() for _ in sizes], data, iterations=1, censored=codes, target_upper=uppers[:1])
    with pytest.raises(ValueError, match="target_upper"):
        multisite_fit.fit_many([cpu_engine() for _ in sizes], data, iterations=1, censored=codes)


def test_fit_many_distributed_passes_the_brackets_on(cpu_engine):
    """Without a process group ``fit_many_distributed`` is ``fit_many`` plus the table: the same bits with ``target_upper``; and a
    site handed back from the table alone (a rank that does not own it) carries its brackets too."""
    from discontinuum_amd import multisite_fit

    data, codes, uppers = [], [], []
    for i, n in enumerate((26, 31)):
        cov, target = loadest_dataset(n, seed=30 + i)
        tgt, c, u = censoring_from_bounds(*_bounds(target, seed=i, k2=4, kminus=2, kplus=1))
        data.append((cov, tgt))
        codes.append(c)
        uppers.append(u)
    a = [cpu_engine() for _ in data]
    oa = multisite_fit.fit_many(a, data, iterations=3, site_seeds=[0, 1], censored=codes, target_upper=uppers)
    b = [cpu_engine() for _ in data]
    ob, _table = multisite_fit.fit_many_distributed(b, data, iterations=3, seed=0, censored=codes, target_upper=uppers)
    assert torch.equal(oa, ob) and all(torch.equal(_flat(x), _flat(y)) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="target_upper"):
        multisite_fit.fit_many_distributed([cpu_engine() for _ in data], data, iterations=1, censored=codes, target_upper=uppers[:1])
    # the hand-back of a site this process did not train
    other = cpu_engine()
    tx, ty, _ = other._attach(*data[0], None)
    other._fresh_model(tx, ty, None)
    other._pending_device = (tx, ty)
    multisite_fit._hand_back_censoring(other, codes[0], tx.shape[0], None, 0, uppers[0], ty)
    br = codes[0] == 2
    assert other._censor.side.tolist() == codes[0].tolist()
    assert np.array_equal(other._censor.upper.numpy()[br], a[0]._censor.upper.numpy()[br])
    assert torch.equal(other._pending_device[1], a[0]._pending_device[1] if a[0]._pending_device is not None else a[0]._train_y)
