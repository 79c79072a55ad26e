"""Threshold excess without a GPU: the references of tests/excess_helpers.py against 30-digit quadrature, Price's integral,
the closed-form limits and draws; the host product through the oracle-backed plan; the C entries' host-side checks."""
from __future__ import annotations

import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch
from scipy.integrate import IntegrationWarning, quad
from scipy.special import ndtr

from discontinuum_amd import _lib
from discontinuum_amd import excess as xs
from discontinuum_amd.engines.base import ModelConfig
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.loads import flux_weights, period_groups, target_transform
from discontinuum_amd.rating_gp import RatingGP
from tests.exceedance_helpers import bvn_excess_ref
from tests.excess_helpers import ExcessOraclePlan, dense_excess_moments, pair_cov_ref
from tests.flux_helpers import daily_loadest, daily_rating, dense_period_moments, gaussian_draws, one_hot

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "excess_pairs.npy")


class SpyPlan(ExcessOraclePlan):
    """Records what the product hands to ``excess_moments``."""

    calls: list = []

    def excess_moments(self, cov, m, mu, scale2, thresh, w, groups, ngroups, above=True, extra_var=None):
        host = lambda v: torch.as_tensor(v).detach().cpu().numpy().copy()  # noqa: E731
        SpyPlan.calls.append(dict(cov=host(cov), mu=host(mu), scale2=float(scale2), thresh=host(thresh), w=host(w), groups=host(groups), above=above,
                                  extra_var=None if extra_var is None else host(extra_var)))
        return super().excess_moments(cov, m, mu, scale2, thresh, w, groups, ngroups, above, extra_var)


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(SpyPlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)
    SpyPlan.calls = []


_MODELS = {}
SPAN = dict(start="2012-06-01", end="2013-06-01")  # one year of days in two calendar years: m = 365, two periods


def _loadest(transform="log"):
    key = ("loadest", transform)
    if key not in _MODELS:
        cov_obs, target, daily = daily_loadest(n_obs=40, **SPAN)
        model = LoadestGP() if transform == "log" else LoadestGP(model_config=ModelConfig(transform=transform))
        model.fit(cov_obs, target, iterations=10)
        _MODELS[key] = (model, daily)
    return _MODELS[key]


def _rating():
    if "rating" not in _MODELS:
        cov_obs, target, unc, daily = daily_rating(n_obs=30, **SPAN)
        model = RatingGP()
        model.fit(cov_obs, target, target_unc=unc, iterations=10)
        _MODELS["rating"] = (model, daily)
    return _MODELS["rating"]


def _posterior(model, daily, pred_noise=False):
    """Model-space posterior mean, covariance and predictive noise at the daily points, as the engine sees them."""
    model._ensure_factor()
    x = torch.tensor(model.dm.Xnew(daily), dtype=torch.float64)
    kmean, cov = model._plan.posterior_cov(model._factor_theta, x)
    mu = (kmean + model.model.prior_mean(x)).detach().numpy()
    noise = model.likelihood.predictive_noise(x.shape[0], x.device, torch.float64).detach().numpy() if pred_noise else None
    return mu, cov.numpy().copy(), noise


def _handed(call):
    """(mapped mean, symmetric model-space covariance, s^2) exactly as the product handed them to the plan."""
    m = call["mu"].shape[0]
    C = call["cov"][:m, :m]
    return call["mu"], np.tril(C) + np.tril(C, -1).T, call["scale2"]


# ------------------------------------------------------------------------------------------------ the references
def test_reference_pair_covariance_against_the_quadrature_fixture():
    """``pair_cov_ref`` vs 30-digit quadrature of the conditional Black-Scholes mean (tests/golden/make_excess_pairs.py),
    280 pairs, both ``above``: <= 1e-14 rms_i rms_j, rms = exp(m + v)."""
    g = np.load(GOLDEN)
    assert g.shape == (280, 9) and set(g[:, 7]) == {0.0, 1.0}
    worst = 0.0
    for above in (True, False):
        r = g[g[:, 7] == float(above)]
        ref = pair_cov_ref(r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], r[:, 5], r[:, 6], above)
        err = np.abs(ref - r[:, 8]) / (np.exp(r[:, 0] + r[:, 1]) * np.exp(r[:, 3] + r[:, 4]))
        print(f"above={above}: max |ref - quadrature| / (rms_i rms_j) = {err.max():.3e} at row {err.argmax()}")
        worst = max(worst, err.max())
    assert worst <= 1e-14


def test_reference_pair_covariance_against_prices_integral():
    """Cov(e_i, e_j) = exp(M_i + M_j) int_0^c exp(c') Phi2((m_i + v_i + c' - a_i) / sigma_i, (m_j + v_j + c' - a_j) / sigma_j;
    c' / (sigma_i sigma_j)) dc' (Price's theorem; excess) by adaptive quadrature on a dozen pairs: the same bound."""
    g = np.load(GOLDEN)
    g = g[(g[:, 7] == 1.0) & (np.abs(g[:, 6]) / np.sqrt(g[:, 1] * g[:, 4]) < 0.995)][::10][:12]
    assert len(g) == 12
    worst = 0.0
    for mi, vi, ai, mj, vj, aj, c, _above, _cov in g:
        si, sj = np.sqrt(vi), np.sqrt(vj)

        def f(cp):
            h, k, r = (mi + vi + cp - ai) / si, (mj + vj + cp - aj) / sj, cp / (si * sj)
            return np.exp(cp) * float(bvn_excess_ref(h, k, r) + ndtr(h) * ndtr(k))

        with warnings.catch_warnings():
            warnings.simplefilter("ignore", IntegrationWarning)
            val, _err = quad(f, 0.0, c, epsabs=1e-16, epsrel=1e-14, limit=400)
        ref = pair_cov_ref(mi, vi, ai, mj, vj, aj, c, True)[0]
        worst = max(worst, abs(np.exp(mi + vi / 2 + mj + vj / 2) * val - ref) / (np.exp(mi + vi) * np.exp(mj + vj)))
    print("max |Price - four-term| / (rms_i rms_j) =", worst)
    assert worst <= 1e-14


def _toy(seed=0, m=60, P=3):
    rng = np.random.default_rng(seed)
    t = np.arange(m)
    C = 0.8 * np.exp(-np.abs(t[:, None] - t[None, :]) / 6.0) + 0.05 * np.eye(m)
    mu = 0.4 * rng.standard_normal(m)
    w = rng.uniform(0.5, 2.0, m)
    g = (t // (m // P)).astype(np.int32)
    return C, mu, w, g


def test_limits_of_the_dense_reference():
    """tau -> 0 is the lognormal period moments (1e-13 relative), tau = +inf gives zeros, a v = 0 point is deterministic and
    uncorrelated with every other, an excluded point adds nothing."""
    C, mu, w, g = _toy()
    m, P, s2 = len(mu), 3, 0.49
    mapped = 0.7 * mu + 0.2
    ev = np.linspace(0.0, 0.1, m)
    zero = np.full((1, m), -np.inf)
    for extra in (None, ev):
        mean, cov, total = dense_excess_moments(C, mapped, s2, zero, w, g, P, True, extra)
        pm, pc = (x.numpy() for x in dense_period_moments(C, mapped, s2, w, g, P, 1, extra))
        assert np.allclose(mean[0], pm, rtol=1e-13, atol=0) and np.allclose(total, pm, rtol=1e-13, atol=0)
        assert np.allclose(cov[0], pc, rtol=0, atol=1e-13 * np.sqrt(np.outer(np.diag(pc), np.diag(pc))).max())
        dmean, dcov, _ = dense_excess_moments(C, mapped, s2, zero, w, g, P, False, extra)
        assert np.all(dmean == 0) and np.all(dcov == 0)
    mean, cov, total = dense_excess_moments(C, mapped, s2, np.full((1, m), np.inf), w, g, P, True)
    assert np.all(mean == 0) and np.all(cov == 0) and np.all(total > 0)
    # a deterministic point: (exp(m) - tau)^+ in the mean, nothing in the covariance
    Cd = C.copy()
    Cd[10, :] = Cd[:, 10] = 0.0
    a = np.full((1, m), np.log(1.1))
    a[0, 10] = mapped[10] - 0.3
    mean, cov, _ = dense_excess_moments(Cd, mapped, s2, a, w, g, P, True)
    gd = g.copy()
    gd[10] = -1
    mean_x, cov_x, _ = dense_excess_moments(Cd, mapped, s2, a, w, gd, P, True)
    assert np.allclose(cov, cov_x, rtol=1e-14, atol=0)
    fixed = w[10] * (np.exp(mapped[10]) - np.exp(a[0, 10]))
    assert fixed > 0 and np.allclose(mean[0] - mean_x[0], [fixed, 0, 0], rtol=0, atol=1e-14 * mean[0].max())
    a[0, 10] = mapped[10] + 0.3  # the fixed value below the threshold: a deficit, no excess
    assert np.allclose(dense_excess_moments(Cd, mapped, s2, a, w, g, P, True)[0], mean_x, rtol=1e-14, atol=0)
    dmean = dense_excess_moments(Cd, mapped, s2, a, w, g, P, False)[0] - dense_excess_moments(Cd, mapped, s2, a, w, gd, P, False)[0]
    assert np.allclose(dmean[0], [w[10] * (np.exp(a[0, 10]) - np.exp(mapped[10])), 0, 0], rtol=0, atol=1e-13)


def test_dense_reference_against_draws_on_a_toy():
    """60 points, 3 periods, 200 000 joint draws: every mean and covariance entry of the dense reference within 4 Monte
    Carlo standard errors, excess and deficit, a per-point threshold beside a constant one."""
    C, mu, w, g = _toy(seed=1)
    m, P, s, t = len(mu), 3, 0.7, 0.2
    rng = np.random.default_rng(5)
    a = np.stack([np.full(m, np.log(1.2)), 0.2 + 0.4 * rng.standard_normal(m)])
    g[33] = -1
    A = one_hot(g, P) * w[:, None]
    c = np.concatenate([np.exp(s * f + t) for f in gaussian_draws(mu, C, 200_000, seed=2)])
    for above in (True, False):
        mean, cov, total = dense_excess_moments(C, s * mu + t, s * s, a, w, g, P, above)
        for l in range(2):
            tau = np.exp(a[l])[None, :]
            sums = np.clip(c - tau if above else tau - c, 0.0, None) @ A
            n = sums.shape[0]
            z = np.abs(mean[l] - sums.mean(axis=0)) / (sums.std(axis=0, ddof=1) / np.sqrt(n))
            assert np.all(z < 4), (above, l, z)
            d = sums - sums.mean(axis=0)
            for p in range(P):
                for q in range(p, P):
                    prod = d[:, p] * d[:, q]
                    assert abs(cov[l, p, q] - prod.mean()) < 4 * prod.std(ddof=1) / np.sqrt(n), (above, l, p, q)
        assert np.all(np.abs(total - (c @ A).mean(axis=0)) < 4 * (c @ A).std(axis=0, ddof=1) / np.sqrt(c.shape[0]))


# ------------------------------------------------------------------------------------------------ the host product
def test_excess_dataset_and_the_dense_reference():
    model, daily = _loadest()
    m = len(daily.coords["time"].values)
    tau = [0.9, 1.2]
    ds, pcov = model.excess(daily, threshold=tau, return_cov=True)
    assert set(ds) == {"mean", "se", "lower", "upper", "total", "share", "n_points"}
    assert ds["mean"].dims == ("level", "time") and ds["mean"].values.shape == (2, 2) and pcov.shape == (2, 2, 2)
    assert ds["total"].dims == ("time",) and list(ds["n_points"].values) == [214, 151]
    assert ds.attrs["above"] is True and ds.attrs["freq"] == "YE" and ds["lower"].attrs["ci"] == 0.95
    assert "ratio of expectations" in ds["share"].attrs["long_name"].lower()
    assert np.array_equal(ds.coords["level"].values, tau)
    call = SpyPlan.calls[-1]
    mu, cov, _ = _posterior(model, daily)
    _mode, s, t = target_transform(model.dm)
    assert call["scale2"] == s * s and np.array_equal(call["thresh"], np.log(np.broadcast_to(np.array(tau)[:, None], (2, m))))
    # (the oracle's posterior repeats to 1e-10 only: the mean is compared loosely, the numbers below use what was handed over)
    assert np.allclose(call["mu"], s * mu + t, rtol=1e-8, atol=0) and call["extra_var"] is None and call["above"] is True
    assert np.allclose(call["cov"][:m, :m], cov[:m, :m], rtol=0, atol=1e-8 * np.abs(cov).max())
    _o, groups, _labels, _n, _d = period_groups(daily.coords["time"].values, np.ones(m), "YE")
    mapped, sym, s2 = _handed(call)
    rmean, rcov, rtotal = dense_excess_moments(sym, mapped, s2, np.log(np.array(tau))[:, None] * np.ones((1, m)), np.ones(m), groups, 2)
    assert np.allclose(ds["mean"].values, rmean, rtol=1e-12, atol=0) and np.allclose(pcov, rcov, rtol=1e-10, atol=0)
    assert np.allclose(ds["total"].values, rtotal, rtol=1e-13, atol=0)
    assert np.allclose(ds["se"].values, np.sqrt(np.diagonal(rcov, axis1=1, axis2=2)), rtol=1e-10, atol=0)
    assert np.array_equal(ds["share"].values, ds["mean"].values / ds["total"].values[None, :])
    assert np.all((ds["share"].values > 0) & (ds["share"].values < 1)) and np.all(np.diff(ds["mean"].values, axis=0) < 0)
    lo, hi = ds["lower"].values, ds["upper"].values
    assert np.all((lo > 0) & (lo < ds["mean"].values) & (ds["mean"].values < hi))
    # the deficit, and put-call parity of the means: excess - deficit = total - sum w tau
    below = model.excess(daily, threshold=tau, above=False)
    assert below.attrs["above"] is False and SpyPlan.calls[-1]["above"] is False
    n = ds["n_points"].values
    assert np.allclose(ds["mean"].values - below["mean"].values, ds["total"].values[None, :] - np.outer(tau, n), rtol=0, atol=1e-10)
    # a constant series is the scalar threshold; tau <= 0 is the total
    ser = model.excess(daily, threshold_series=np.stack([np.full(m, 0.9), np.full(m, 1.2)]))
    assert np.array_equal(ser["mean"].values, ds["mean"].values)
    whole = model.excess(daily, threshold=0.0)
    assert np.allclose(whole["mean"].values[0], ds["total"].values, rtol=1e-13, atol=0) and np.allclose(whole["share"].values, 1.0)
    with pytest.raises(ValueError, match="exactly one"):
        model.excess(daily)
    with pytest.raises(ValueError, match="shape"):
        model.excess(daily, threshold_series=np.ones(m - 1))
    with pytest.raises(RuntimeError, match="hasn't been fitted"):
        LoadestGP().excess(daily, threshold=1.0)


def test_excess_load_by_limit_and_by_criterion():
    model, daily = _loadest()
    m = len(daily.coords["time"].values)
    wf = flux_weights(daily, {"units": "mg/l"})
    limit = float(np.median(wf)) * 1.1  # kg per day
    ds, pcov = model.excess_load(daily, limit=limit, return_cov=True)
    assert ds["mean"].attrs["units"] == "kilograms" and np.array_equal(ds.coords["level"].values, [limit])
    _o, groups, _labels, _n, _d = period_groups(daily.coords["time"].values, np.ones(m), "YE")
    mapped, sym, s2 = _handed(SpyPlan.calls[-1])
    rmean, rcov, rtotal = dense_excess_moments(sym, mapped, s2, np.log(limit / wf)[None, :], wf, groups, 2)
    assert np.allclose(ds["mean"].values, rmean, rtol=1e-12, atol=0) and np.allclose(pcov, rcov, rtol=1e-10, atol=0)
    assert np.allclose(ds["total"].values, rtotal, rtol=1e-13, atol=0)
    flux = model.annual_flux(daily)
    assert np.allclose(ds["total"].values, flux["mean"].values, rtol=1e-8, atol=0)  # the period's expected load
    # a concentration criterion is excess(threshold, weights = flux weights); per-day series and lists of levels
    crit, ccov = model.excess_load(daily, criterion=[0.9, 1.2], return_cov=True)
    gen, gcov = model.excess(daily, threshold=[0.9, 1.2], weights=wf, return_cov=True)
    assert np.array_equal(crit["mean"].values, gen["mean"].values) and np.array_equal(ccov, gcov)
    series = limit * (1 + 0.1 * np.sin(np.arange(m)))
    per_day = model.excess_load(daily, limit=series)
    assert np.array_equal(SpyPlan.calls[-1]["thresh"], np.log(series / wf)[None, :]) and per_day["mean"].values.shape == (1, 2)
    below = model.excess_load(daily, limit=limit, above=False)
    assert np.allclose(ds["mean"].values - below["mean"].values, ds["total"].values[None, :] - limit * ds["n_points"].values,
                       rtol=0, atol=1e-9 * ds["total"].values.max())
    # a day without flow is excluded, like flux_exceedance excludes it
    from discontinuum_amd.xr_compat import Dataset

    q = np.array(daily["flow"].values, dtype=np.float64)
    q[100], q[300] = np.nan, 0.0
    holed = Dataset({"flow": ("time", q, {"units": "cubic meters per second"})}, coords={"time": daily.coords["time"].values})
    part = model.excess_load(holed, limit=limit)
    assert list(part["n_points"].values) == [213, 150] and SpyPlan.calls[-1]["thresh"].shape == (1, m - 2)
    for kw in ({}, {"criterion": 1.0, "limit": limit}):
        with pytest.raises(ValueError, match="exactly one"):
            model.excess_load(daily, **kw)


def test_rating_deficit_volume_with_seconds_as_weights():
    model, daily = _rating()
    m = len(daily.coords["time"].values)
    seconds = np.full(m, 86400.0)
    mu, cov, _ = _posterior(model, daily)
    _mode, s, t = target_transform(model.dm)
    low = float(np.exp(np.quantile(s * mu + t, 0.3)))
    ds, pcov = model.excess(daily, threshold=low, weights=seconds, above=False, return_cov=True)
    _o, groups, _labels, _n, _d = period_groups(daily.coords["time"].values, seconds, "YE")
    mapped, sym, s2 = _handed(SpyPlan.calls[-1])
    rmean, rcov, _total = dense_excess_moments(sym, mapped, s2, np.full((1, m), np.log(low)), seconds, groups, 2, above=False)
    assert np.allclose(ds["mean"].values, rmean, rtol=1e-12, atol=0) and np.allclose(pcov, rcov, rtol=1e-10, atol=0)
    assert np.all(ds["mean"].values > 0) and np.all(ds["mean"].values < low * 86400.0 * ds["n_points"].values)
    # predictive noise goes into the variances (model space), never into the covariances: a larger deficit
    noisy = model.excess(daily, threshold=low, weights=seconds, above=False, pred_noise=True)
    extra = SpyPlan.calls[-1]["extra_var"]
    assert extra is not None and extra.shape == (m,) and np.all(extra > 0) and np.all(noisy["mean"].values > ds["mean"].values)
    mapped, sym, s2 = _handed(SpyPlan.calls[-1])
    nmean = dense_excess_moments(sym, mapped, s2, np.full((1, m), np.log(low)), seconds, groups, 2, above=False, extra_var=extra)[0]
    assert np.allclose(noisy["mean"].values, nmean, rtol=1e-12, atol=0)
    wts = seconds.copy()
    wts[7] = np.nan  # a non-finite weight drops the point
    assert list(model.excess(daily, threshold=low, weights=wts)["n_points"].values) == [213, 151]


def test_refusals_say_why():
    model, daily = _loadest()
    with pytest.raises(NotImplementedError, match=r"footprint of \d+ bytes.*max_bytes = 1000000.*no streamed form"):
        model.excess(daily, threshold=1.0, max_bytes=1_000_000)
    with pytest.raises(NotImplementedError, match=r"footprint of \d+ bytes"):
        model.excess_load(daily, criterion=1.0, max_bytes=1_000_000)
    assert not SpyPlan.calls
    linear, daily = _loadest("standard")
    with pytest.raises(NotImplementedError, match="log targets only"):
        linear.excess(daily, threshold=1.0)
    with pytest.raises(NotImplementedError, match="log targets only"):
        linear.excess_load(daily, limit=10.0)
    assert not SpyPlan.calls


# ------------------------------------------------------------------------------------------------ the C entries
def test_excess_abi_without_a_device():
    """Both symbols are exported and bound through ``EXT_SIGNATURES``, declared in include/dgp_hip_ext.h and nowhere in
    ``SIGNATURES``; sizes and every refusal with null device addresses: each call is refused before a launch."""
    import re

    lib = _lib.load()
    names = {"dgp_excess_moments_workspace_bytes", "dgp_excess_moments"}
    assert set(_lib.EXT_SIGNATURES) == names and not names & set(_lib.SIGNATURES) and len(_lib.SIGNATURES) == 114
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    ext = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "dgp_hip_ext.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(dgp_[a-z_0-9]+)\s*\(", ext)) == names
    assert open(os.path.join(inc, "dgp_hip.h")).read().count('#include "dgp_hip_ext.h"') == 1
    for name in names:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.EXT_SIGNATURES[name][1] and fn.restype == _lib.EXT_SIGNATURES[name][0]
    q = lib.dgp_excess_moments_workspace_bytes
    need = q(1000, 3, 2, 2)
    M = lib.dgp_padded_n(1000)
    assert need == 2 * 8 * (M * (3 + 6 * 2 + 3 * 2) + 3) and need == 2 * xs._work_bytes(1000, 3, 2)
    assert q(1000, 3, 64, 1) == 8 * (M * (3 + 6 * 64 + 3 * 2) + 3) == xs._work_bytes(1000, 3, 64)  # Y holds one chunk of levels
    assert q(1, 1, 1, 1) == xs._work_bytes(1, 1, 1) and q(11323, 31, 8, 1) == xs._work_bytes(11323, 31, 8)
    for bad in ((0, 3, 1, 1), (-5, 3, 1, 1), ((1 << 20) + 1, 3, 1, 1), (10, 0, 1, 1), (10, 65536, 1, 1), (10, 3, 0, 1), (10, 3, 65, 1),
                (10, 3, 1, 0), (10, 3, 1, 1025)):
        assert q(*bad) == 0, bad
    p, work = C.c_void_p(16), C.c_void_p(4096)  # never dereferenced: every call below fails its host-side checks

    def args(**kw):
        return [kw.get("dtype", 0), kw.get("cov", p), kw.get("m", 1000), kw.get("batch", 2), kw.get("mu", p), kw.get("s2", p),
                kw.get("thresh", p), kw.get("w", p), kw.get("g", p), kw.get("ng", 3), kw.get("nl", 2), None, kw.get("above", 1),
                kw.get("work", work), kw.get("wb", need), kw.get("mean", p), kw.get("out", p), kw.get("total", p), None]

    call = lib.dgp_excess_moments
    assert call(*args(dtype=2)) == -1 and b"dgp_excess_moments: dtype" in lib.dgp_last_error()
    for name in ("cov", "mu", "s2", "thresh", "w", "g", "mean", "out", "total"):
        assert call(*args(**{name: None})) == -1 and b"null" in lib.dgp_last_error(), name
    for kw in ({"m": 0}, {"m": (1 << 20) + 1}, {"ng": 0}, {"ng": 65536}, {"nl": 0}, {"nl": 65}, {"batch": 0}, {"batch": 1025}):
        assert call(*args(**kw)) == -1 and b"size" in lib.dgp_last_error(), kw
    for above in (-1, 2):
        assert call(*args(above=above)) == -1 and b"above" in lib.dgp_last_error()
    assert call(*args(wb=need - 1)) == -3 and b"workspace" in lib.dgp_last_error()
    assert call(*args(work=None)) == -3 and b"workspace" in lib.dgp_last_error()
    assert call(*args(work=C.c_void_p(4096 + 128))) == -1 and b"256-byte aligned" in lib.dgp_last_error()
