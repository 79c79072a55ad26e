"""Exact exceedance statistics (``MarginalHIP.exceedance`` / ``duration_curve`` / ``exceedance_probability``,
``LoadestGP.exceedance(kind="flux")``) on CPU: the references of tests/exceedance_helpers.py pinned against scipy; the host
logic -- grouping, threshold mapping, complement, fraction, intervals -- against a seeded Monte Carlo of the reference
workflow (posterior draws, compared with the threshold and counted per period), with the device plan replaced by an
oracle-backed double; and the new C entries' argument checks without a device."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch
from scipy.integrate import IntegrationWarning, quad
from scipy.special import ndtr
from scipy.stats import multivariate_normal

from discontinuum_amd import _lib
from discontinuum_amd import exceedance as ex
from discontinuum_amd.engines.base import ModelConfig
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.loads import flux_weights, period_groups, target_transform
from discontinuum_amd.rating_gp import RatingGP
from discontinuum_amd.xr_compat import Dataset
from tests.exceedance_helpers import ExceedOraclePlan, bvn_excess_ref, dense_exceedance_moments, design_set
from tests.flux_helpers import daily_loadest, daily_rating, gaussian_draws, one_hot

NDRAW = 200_000


class SpyPlan(ExceedOraclePlan):
    """Records what the product hands to ``exceedance_moments``."""

    calls: list = []

    def exceedance_moments(self, cov, m, mu, thresh, w, groups, ngroups, extra_var=None):
        host = lambda v: torch.as_tensor(v).detach().cpu().numpy().copy()  # noqa: E731
        SpyPlan.calls.append(dict(cov=cov.clone(), mu=mu.clone(), thresh=host(thresh), w=host(w), groups=host(groups),
                                  extra_var=None if extra_var is None else extra_var.clone()))
        return super().exceedance_moments(cov, m, mu, thresh, w, groups, ngroups, extra_var)


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(SpyPlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)
    SpyPlan.calls = []


_MODELS = {}


def _loadest(transform="log", seed=0):
    key = ("loadest", transform, seed)
    if key not in _MODELS:
        cov_obs, target, daily = daily_loadest(seed=seed)
        model = LoadestGP() if transform == "log" else LoadestGP(model_config=ModelConfig(transform=transform))
        model.fit(cov_obs, target, iterations=10)
        _MODELS[key] = (model, daily)
    return _MODELS[key]


def _rating():
    if "rating" not in _MODELS:
        cov_obs, target, unc, daily = daily_rating()
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


# ------------------------------------------------------------------------------------------------ the references
def test_reference_pair_function_against_scipy_and_plackett():
    """Owen's-T form vs ``multivariate_normal.cdf`` on the design set (2000 pairs) and, on a subset, vs adaptive quadrature
    of Plackett's integral D = int_0^asin(rho) exp(-(h^2 - 2 h k sin t + k^2) / (2 cos^2 t)) dt / (2 pi): 1e-13."""
    h, k, r = design_set(100, seed=3)
    ref = bvn_excess_ref(h, k, r)
    inner = np.abs(r) < 1
    worst = 0.0
    for i in np.nonzero(inner)[0]:
        phi2 = multivariate_normal.cdf([h[i], k[i]], mean=[0.0, 0.0], cov=[[1.0, r[i]], [r[i], 1.0]])
        worst = max(worst, abs(phi2 - ndtr(h[i]) * ndtr(k[i]) - ref[i]))
    print("max |Owen - scipy| =", worst)
    assert worst <= 1e-13
    edge = ~inner
    ph, pk = ndtr(h[edge]), ndtr(k[edge])
    closed = np.where(r[edge] > 0, np.minimum(ph, pk), np.maximum(0.0, ph + pk - 1.0)) - ph * pk
    assert np.array_equal(ref[edge], closed)
    worst_q = 0.0
    for i in np.nonzero(inner)[0][::7]:
        f = lambda t, a=h[i], b=k[i]: np.exp(-(a * a - 2 * a * b * np.sin(t) + b * b) / (2 * np.cos(t) ** 2)) / (2 * np.pi)  # noqa: E731
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", IntegrationWarning)  # (the requested 1e-15 sits at the rounding floor)
            val, _err = quad(f, 0.0, np.arcsin(r[i]), epsabs=1e-15, epsrel=1e-14, limit=400)
        worst_q = max(worst_q, abs(val - ref[i]))
    print("max |Owen - quad| =", worst_q)
    assert worst_q <= 1e-13
    assert bvn_excess_ref(np.inf, 0.3, 0.5) == 0.0 and bvn_excess_ref(0.1, -np.inf, 0.99) == 0.0
    assert np.isnan(bvn_excess_ref(np.nan, 0.3, 0.5)) and np.isnan(bvn_excess_ref(0.1, 0.3, np.nan))


def test_dense_reference_against_draws_on_a_toy():
    """60 points, 3 periods, 400 000 draws: every mean and covariance entry of the dense reference within 5 Monte Carlo
    standard errors; decided points (zero variance, infinite thresholds) and an excluded one included."""
    rng = np.random.default_rng(0)
    m, P = 60, 3
    t = np.arange(m)
    C = 0.8 * np.exp(-np.abs(t[:, None] - t[None, :]) / 6.0) + 0.05 * np.eye(m)
    C[10, :] = C[:, 10] = 0.0  # a zero-variance point
    mu = 0.4 * rng.standard_normal(m)
    u = np.stack([np.full(m, 0.2), 0.5 * rng.standard_normal(m)])
    u[0, 20], u[0, 21] = np.inf, -np.inf
    w = rng.uniform(0.5, 2.0, m)
    g = (t // 20).astype(np.int32)
    g[33] = -1
    mean, cov = dense_exceedance_moments(C, mu, u, w, g, P)
    A = one_hot(g, P) * w[:, None]
    counts = [np.concatenate([(f > u[l][None, :]) @ A for f in gaussian_draws(mu, C, 400_000, seed=1)]) for l in range(2)]
    for l in range(2):
        n = counts[l].shape[0]
        z = np.abs(mean[l] - counts[l].mean(axis=0)) / (counts[l].std(axis=0, ddof=1) / np.sqrt(n))
        assert np.all(z < 5), z
        d = counts[l] - counts[l].mean(axis=0)
        for a in range(P):
            for b in range(a, P):
                prod = d[:, a] * d[:, b]
                assert abs(cov[l, a, b] - prod.mean()) < 5 * prod.std(ddof=1) / np.sqrt(n), (l, a, b)


# ------------------------------------------------------------------------------------------------ the C entries
def test_exceedance_abi_without_a_device():
    lib = _lib.load()
    q = lib.dgp_exceedance_moments_workspace_bytes
    need = q(1000, 3, 2, 2)
    M = lib.dgp_padded_n(1000)
    assert need == 2 * 8 * (2 * M + 2 * 2 * M + 2 * M * 3 + 3)
    assert q(2000, 3, 2, 2) > need and q(1000, 4, 2, 2) > need and q(1000, 3, 3, 2) > need
    assert q(1000, 3, 64, 1) == 8 * (2 * M + 2 * 64 * M + 8 * M * 3 + 3)  # Y holds one chunk of levels: nothing of order L M P
    for bad in ((0, 3, 1, 1), (1 << 21, 3, 1, 1), (10, 0, 1, 1), (10, 65536, 1, 1), (10, 3, 0, 1), (10, 3, 65, 1), (10, 3, 1, 0),
                (10, 3, 1, 1025)):
        assert q(*bad) == 0, bad
    p = C.c_void_p(16)  # never dereferenced: every call below fails its host-side checks

    def args(**kw):
        return [kw.get("dtype", 0), kw.get("cov", p), kw.get("m", 1000), kw.get("batch", 2), kw.get("mu", p), kw.get("thresh", p),
                kw.get("nl", 2), kw.get("w", p), kw.get("group", p), kw.get("ng", 3), None, kw.get("work", p), kw.get("wb", need),
                kw.get("mean", p), kw.get("covo", p), None]

    f = lib.dgp_exceedance_moments
    assert f(*args(dtype=2)) == -1 and b"dtype" in lib.dgp_last_error()
    for name in ("cov", "mu", "thresh", "w", "group", "mean", "covo"):
        assert f(*args(**{name: None})) == -1 and b"null" in lib.dgp_last_error(), name
    for kw in (dict(m=0), dict(m=(1 << 20) + 1), dict(batch=0), dict(batch=1025), dict(ng=0), dict(ng=65536), dict(nl=0), dict(nl=65)):
        assert f(*args(**kw)) == -1 and b"size" in lib.dgp_last_error(), kw
    assert f(*args(wb=need - 1)) == -3 and b"workspace" in lib.dgp_last_error()
    assert f(*args(work=None)) == -3 and b"workspace" in lib.dgp_last_error()
    g = lib.dgp_debug_bvn_excess
    assert g(None, p, p, 4, p, None) == -1 and b"dgp_debug_bvn_excess" in lib.dgp_last_error()
    assert g(p, p, p, 0, p, None) == -1 and g(p, p, p, 4, None, None) == -1


# ------------------------------------------------------------------------------------------------ the product layer
def _mc_check(ds, pcov, counts, name):
    """Means within 5 Monte Carlo standard errors; covariance entries within 5 standard errors of the sample covariance,
    that standard error estimated from the draws' own centred products."""
    n = counts.shape[0]
    mean = np.asarray(ds["mean"].values)
    sd = counts.std(axis=0, ddof=1)
    live = sd > 0
    z = np.abs(mean - counts.mean(axis=0))[live] / (sd[live] / np.sqrt(n))
    assert np.all(z < 5), (name, z)
    assert np.allclose(mean[~live], counts.mean(axis=0)[~live], atol=1e-6), name
    d = counts - counts.mean(axis=0)
    P = counts.shape[1]
    for a in range(P):
        for b in range(a, P):
            prod = d[:, a] * d[:, b]
            tol = 5 * prod.std(ddof=1) / np.sqrt(n) + 1e-9
            assert abs(pcov[a, b] - prod.mean()) <= tol, (name, a, b, pcov[a, b], prod.mean(), tol)
    assert np.allclose(np.sqrt(np.diag(pcov)), ds["se"].values)
    assert np.all(ds["lower"].values <= ds["upper"].values), name


def test_loadest_exceedance_matches_the_sampling_workflow():
    model, daily = _loadest()
    _mode, s, t = target_transform(model.dm)
    mu, cov, _ = _posterior(model, daily)
    conc_mean = np.exp(s * mu + t)
    levels = np.quantile(conc_mean, [0.3, 0.7])
    ds, pcov = model.exceedance(daily, threshold=levels, freq="YE", return_cov=True)
    assert ds["mean"].values.shape == (2, 3) and pcov.shape == (2, 3, 3)
    assert list(ds["n_points"].values) == [366, 365, 365] and np.array_equal(ds.coords["level"].values, levels)
    assert np.all(np.diff(ds["mean"].values, axis=0) <= 1e-12)  # a higher level is exceeded less often
    time = daily.coords["time"].values
    _o, groups, labels, _n, _d = period_groups(time, np.ones(len(time)), "YE")
    A = one_hot(groups, len(labels))
    counts = [[], []]
    for f in gaussian_draws(mu, cov, NDRAW, seed=1):
        conc = np.exp(s * f + t)
        for l in range(2):
            counts[l].append((conc > levels[l]).astype(np.float64) @ A)
    for l in range(2):
        one = Dataset({k: ("time", ds[k].values[l]) for k in ("mean", "se", "lower", "upper")}, coords={"time": labels})
        _mc_check(one, pcov[l], np.concatenate(counts[l]), f"loadest level {l}")


def test_rating_exceedance_with_predictive_noise_matches_the_sampling_workflow():
    model, daily = _rating()
    _mode, s, t = target_transform(model.dm)
    mu, cov, noise = _posterior(model, daily, pred_noise=True)
    q_mean = np.exp(s * mu + t)
    level = float(np.quantile(q_mean, 0.6))
    latent = model.exceedance(daily, threshold=level, freq="YE")
    ds, pcov = model.exceedance(daily, threshold=level, freq="YE", pred_noise=True, return_cov=True)
    assert not np.allclose(latent["mean"].values, ds["mean"].values)
    # pred_noise changes sigma and leaves rho's numerator unchanged: the same covariance buffer, the noise beside it
    a, b = SpyPlan.calls[-2], SpyPlan.calls[-1]
    assert a["extra_var"] is None and torch.equal(a["cov"], b["cov"])
    assert np.allclose(b["extra_var"].numpy(), noise) and np.all(noise > 0)
    time = daily.coords["time"].values
    _o, groups, labels, _n, _d = period_groups(time, np.ones(len(time)), "YE")
    A = one_hot(groups, len(labels))
    full = cov + np.diag(noise)
    counts = np.concatenate([(np.exp(s * f + t) > level).astype(np.float64) @ A for f in gaussian_draws(mu, full, NDRAW, seed=2)])
    one = Dataset({k: ("time", ds[k].values[0]) for k in ("mean", "se", "lower", "upper")}, coords={"time": labels})
    _mc_check(one, pcov[0], counts, "rating pred_noise")


@pytest.mark.parametrize("transform", ["log", "standard"])
def test_thresholds_map_exactly_to_model_space(transform):
    model, daily = _loadest(transform, seed=3)
    mode, s, t = target_transform(model.dm)
    assert mode == (1 if transform == "log" else 0)
    mu, cov, _ = _posterior(model, daily)
    tau = np.array([0.9, 1.4])
    u = (np.log(tau) - t) / s if transform == "log" else (tau - t) / s
    m = len(mu)
    _o, groups, labels, _n, _d = period_groups(daily.coords["time"].values, np.ones(m), "ME")
    rmean, rcov = dense_exceedance_moments(cov, mu, np.broadcast_to(u[:, None], (2, m)), np.ones(m), groups, len(labels))
    ds, pcov = model.exceedance(daily, threshold=tau, freq="ME", return_cov=True)
    assert np.allclose(ds["mean"].values, rmean, rtol=0, atol=1e-10) and np.allclose(pcov, rcov, rtol=0, atol=1e-10)
    assert np.allclose(SpyPlan.calls[-1]["thresh"], np.broadcast_to(u[:, None], (2, m)), rtol=1e-15, atol=0)
    if transform == "log":  # a non-positive level of a log target is always exceeded
        always = model.exceedance(daily, threshold=[0.0, -1.0], freq="YE")
        assert np.array_equal(always["mean"].values, np.broadcast_to(always["n_points"].values, (2, 3)))
        assert np.all(always["se"].values == 0) and np.array_equal(always["lower"].values, always["mean"].values)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="finite"):
            model.exceedance(daily, threshold=bad)


def test_complement_fraction_series_and_levels():
    model, daily = _loadest()
    m = len(daily.coords["time"].values)
    tau = [0.8, 1.1, 1.5]
    ds, pcov = model.exceedance(daily, threshold=tau, return_cov=True)
    n = ds["n_points"].values.astype(np.float64)
    below, bcov = model.exceedance(daily, threshold=tau, above=False, return_cov=True)
    assert np.array_equal(below["mean"].values, n[None, :] - ds["mean"].values) and np.array_equal(bcov, pcov)
    assert np.array_equal(below["se"].values, ds["se"].values)
    frac, fcov = model.exceedance(daily, threshold=tau, fraction=True, return_cov=True)
    assert np.allclose(frac["mean"].values, ds["mean"].values / n, rtol=1e-15, atol=0)
    assert np.allclose(frac["se"].values, ds["se"].values / n, rtol=1e-15, atol=0)
    assert np.allclose(fcov, pcov / (n[:, None] * n[None, :]), rtol=1e-15, atol=0)
    assert np.all((frac["mean"].values >= 0) & (frac["mean"].values <= 1))
    assert np.all(np.diff(ds["mean"].values, axis=0) <= 1e-12)
    # a constant per-point series is the scalar threshold
    one = model.exceedance(daily, threshold=1.1)
    ser = model.exceedance(daily, threshold_series=np.full(m, 1.1))
    assert np.array_equal(one["mean"].values, ser["mean"].values) and np.array_equal(one["se"].values, ser["se"].values)
    assert np.allclose(one["mean"].values[0], ds["mean"].values[1], rtol=0, atol=1e-10)
    two = model.exceedance(daily, threshold_series=np.stack([np.full(m, 0.8), np.full(m, 1.5)]))
    assert np.allclose(two["mean"].values, ds["mean"].values[[0, 2]], rtol=0, atol=1e-10)
    lo, hi = ds["lower"].values, ds["upper"].values
    # (a central interval of a count pressed against its bound need not contain the mean)
    assert np.all(lo <= hi) and np.all(lo >= 0) and np.all(hi <= n[None, :]) and np.all(hi[2] > ds["mean"].values[2])
    with pytest.raises(ValueError, match="exactly one"):
        model.exceedance(daily)
    with pytest.raises(ValueError, match="exactly one"):
        model.exceedance(daily, threshold=1.0, threshold_series=np.ones(m))
    with pytest.raises(ValueError, match="shape"):
        model.exceedance(daily, threshold_series=np.ones(m - 1))
    with pytest.raises(RuntimeError, match="hasn't been fitted"):
        LoadestGP().exceedance(daily, threshold=1.0)


def test_flux_kind_is_the_per_day_concentration_threshold():
    model, daily = _loadest()
    wf = flux_weights(daily, {"units": "mg/l"})
    limit = float(np.median(wf)) * 1.1  # kg per day
    flux, fcov = model.exceedance(daily, threshold=limit, kind="flux", return_cov=True)
    ser, scov = model.exceedance(daily, threshold_series=limit / wf, return_cov=True)
    assert np.array_equal(flux["mean"].values, ser["mean"].values) and np.array_equal(fcov, scov)
    assert np.array_equal(flux.coords["level"].values, [limit])
    # a day without flow is excluded; so is a NaN-weight point, like aggregate drops it
    q = np.array(daily["flow"].values, dtype=np.float64)
    q[100], q[500] = np.nan, 0.0
    holed = Dataset({"flow": ("time", q, {"units": "cubic meters per second"})}, coords={"time": daily.coords["time"].values})
    part = model.exceedance(holed, threshold=limit, kind="flux")
    assert list(part["n_points"].values) == [365, 364, 365]
    call = SpyPlan.calls[-1]
    assert call["thresh"].shape == (1, len(q) - 2) and np.all(call["groups"] >= 0)
    wts = np.ones(len(q))
    wts[100] = np.nan
    dropped = ex._exceedance(model, daily, threshold=1.1, weights=wts)
    assert list(dropped["n_points"].values) == [365, 365, 365]
    mu, cov, _ = _posterior(model, daily)
    keep = np.arange(len(q)) != 100
    _mode, s, t = target_transform(model.dm)
    _o, groups, labels, _n, _d = period_groups(daily.coords["time"].values[keep], np.ones(keep.sum()), "YE")
    rmean, _rcov = dense_exceedance_moments(cov[np.ix_(keep, keep)], mu[keep], np.full((1, keep.sum()), (np.log(1.1) - t) / s),
                                            np.ones(keep.sum()), groups, 3)
    assert np.allclose(dropped["mean"].values, rmean, rtol=0, atol=1e-9)
    with pytest.raises(ValueError, match="kind"):
        model.exceedance(daily, threshold=1.0, kind="load")
    with pytest.raises(ValueError, match="kg per day"):
        model.exceedance(daily, threshold_series=np.ones(len(q)), kind="flux")


def test_duration_curve_and_exceedance_probability():
    model, daily = _rating()
    dc = model.duration_curve(daily)
    f = dc["mean"].values
    assert f.shape == (21,) and np.all((f >= 0) & (f <= 1)) and np.all(np.diff(f) <= 1e-12)
    assert np.all(np.diff(dc.coords["level"].values) > 0) and f[0] > 0.9 and f[-1] < 0.1
    assert np.all(dc["se"].values >= 0) and np.all(dc["lower"].values <= dc["upper"].values)
    mid = slice(5, 16)
    assert np.all(dc["lower"].values[mid] < f[mid]) and np.all(dc["upper"].values[mid] > f[mid])
    below = model.duration_curve(daily, above=False)
    assert np.allclose(below["mean"].values, 1 - f, rtol=0, atol=1e-14)
    levels = dc.coords["level"].values[[3, 10, 17]]
    some = model.duration_curve(daily, levels=levels)
    assert np.allclose(some["mean"].values, f[[3, 10, 17]], rtol=0, atol=1e-14)
    m = len(daily.coords["time"].values)
    whole = model.exceedance(daily, threshold=levels, freq="YE", fraction=False)
    assert np.allclose(whole["mean"].values.sum(axis=1) / m, some["mean"].values, rtol=0, atol=1e-12)
    # pointwise probabilities: Phi((mu - u) / sigma) from the prediction
    _mode, s, t = target_transform(model.dm)
    x = torch.tensor(model.dm.Xnew(daily), dtype=torch.float64)
    for pred_noise in (False, True):
        mu, var = model._model_space_predict(x)
        if not pred_noise:
            var = var - model.likelihood.predictive_noise(m, var.device, torch.float64)
        z = (mu.detach().numpy() - (np.log(levels[1]) - t) / s) / np.sqrt(var.detach().numpy())
        p = model.exceedance_probability(daily, levels[1], pred_noise=pred_noise)
        assert p.dims == ("time",) and np.allclose(p.values, ndtr(z), rtol=0, atol=1e-14)
        q = model.exceedance_probability(daily, levels[1], above=False, pred_noise=pred_noise)
        assert np.allclose(p.values + q.values, 1.0, rtol=0, atol=1e-14)
    # the expected count is the sum of the pointwise probabilities
    p = model.exceedance_probability(daily, levels[1])
    assert np.allclose(p.values.sum() / m, some["mean"].values[1], rtol=0, atol=1e-10)


def test_an_over_budget_record_raises():
    model, daily = _loadest()
    with pytest.raises(ValueError, match=r"footprint of \d+ bytes.*max_bytes = 1000000"):
        model.exceedance(daily, threshold=1.0, max_bytes=1_000_000)
    assert not SpyPlan.calls
