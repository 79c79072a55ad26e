"""Monitoring design (``MarginalHIP.sample_value`` / ``design_value`` / ``design``) on CPU: the series-length rule, the new C
entries' argument checks without a device, and the host logic -- groups, weights, A_i, the sample variance, the mean shift
handed to ``period_moments``, the greedy loop, the error paths -- with the device plan replaced by an oracle-backed double
(tests/design_helpers.py: the direct double sum and the dense solve); one seeded Monte Carlo check of V(S)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from discontinuum_amd.backend import series_terms
from discontinuum_amd.engines.base import ModelConfig
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.loads import flux_weights, period_groups, target_transform
from discontinuum_amd.rating_gp import RatingGP
from tests.design_helpers import DesignOraclePlan, design_value_ref, direct_gain, explained_cov, greedy_ref, linear_gain
from tests.flux_helpers import daily_loadest, daily_rating

NDRAW = 200_000


class SpyPlan(DesignOraclePlan):
    """Records what the product hands to ``sample_value`` and ``period_moments``."""

    calls: list = []
    moments: list = []

    def sample_value(self, cov, m, a, scale2, groups, ngroups, obs_var=None, rows=None, nterms=None):
        host = lambda v: None if v is None else torch.as_tensor(v).detach().cpu().double().numpy().copy()  # noqa: E731
        SpyPlan.calls.append(dict(cov=host(cov), m=m, a=host(a), scale2=float(scale2), groups=host(groups), ngroups=ngroups,
                                  obs_var=host(obs_var), rows=host(rows), nterms=nterms))
        return super().sample_value(cov, m, a, scale2, groups, ngroups, obs_var, rows, nterms)

    def period_moments(self, cov, m, mu, scale2, w, groups, ngroups, mode, extra_var=None):
        host = lambda v: torch.as_tensor(v).detach().cpu().double().numpy().copy()  # noqa: E731
        SpyPlan.moments.append(dict(cov=host(cov), mu=host(mu), w=host(w), mode=mode))
        return super().period_moments(cov, m, mu, scale2, w, groups, ngroups, mode, extra_var)


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(SpyPlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)
    SpyPlan.calls, SpyPlan.moments = [], []


_MODELS = {}


def _loadest(transform="log"):
    if transform not in _MODELS:
        cov_obs, target, daily = daily_loadest(seed=0, step_days=5)  # 220 days, three years
        model = LoadestGP() if transform == "log" else LoadestGP(model_config=ModelConfig(transform=transform))
        model.fit(cov_obs, target, iterations=10)
        _MODELS[transform] = (model, daily)
    return _MODELS[transform]


def _posterior(model, daily):
    """Model-space posterior mean and covariance at the daily points, as the engine sees them."""
    model._ensure_factor()
    x = torch.tensor(model.dm.Xnew(daily), dtype=torch.float64)
    kmean, cov = model._plan.posterior_cov(model._factor_theta, x)
    return (kmean + model.model.prior_mean(x)).detach().numpy(), cov.numpy().copy()


# ------------------------------------------------------------------------------------------------ the K rule
def test_series_terms_rule_and_its_raise():
    def tail(beta, K):
        return math.fsum(math.exp(k * math.log(beta) - math.lgamma(k + 1)) for k in range(K + 1, K + 100))

    for beta in (1e-9, 1e-3, 0.1, 0.5, 1.0, 1.65, 3.0, 7.5, 12.0, 14.5):
        K = series_terms(beta)
        assert 1 <= K <= 64 and tail(beta, K) <= 2.0 ** -53 * beta * (1 + 1e-9), (beta, K)
        assert K == 1 or tail(beta, K - 1) > 2.0 ** -53 * beta * (1 - 1e-9), (beta, K)
    assert series_terms(0.0) == 1 and series_terms(1.65) in (20, 21) and series_terms(0.5) <= 16 < series_terms(1.0)
    with pytest.raises(ValueError, match=r"beta = s\^2 max C_ii = 16"):
        series_terms(16.0)
    for big in (14.9, 64.0, 65.0, 800.0, 1e3, 1e30, 1e308):  # decided at once, however large: the series is never run to the end
        with pytest.raises(ValueError, match="needs more than 64 terms"):
            series_terms(big)
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError, match="beta"):
            series_terms(bad)


# ------------------------------------------------------------------------------------------------ the C entries
def test_sample_value_abi_without_a_device():
    lib = _lib.load()
    q = lib.dgp_sample_value_workspace_bytes
    M = lib.dgp_padded_n(1000)
    # few groups: their days are cut into slabs whose partial sums live in the work area ...
    assert q(1000, 3, 2, 5, 2) == 2 * 8 * (M + 3 * 64 * 5 * M + 3)
    assert q(1000, 3, 2, 6, 2) > q(1000, 3, 2, 5, 2) and q(1000, 3, 0, 5, 2) == q(1000, 3, 64, 5, 2)
    # ... many groups fill the device by themselves: nothing of order K M P
    assert q(1000, 300, 0, 64, 1) == 8 * (M + 300)
    for bad in ((0, 3, 0, 1, 1), ((1 << 20) + 1, 3, 0, 1, 1), (10, 0, 0, 1, 1), (10, 65536, 0, 1, 1), (10, 3, -1, 1, 1), (10, 3, 65, 1, 1),
                (10, 3, 0, 0, 1), (10, 3, 0, 65, 1), (10, 3, 0, 1, 0), (10, 3, 0, 1, 1025)):
        assert q(*bad) == 0, bad
    p = C.c_void_p(16)  # never dereferenced: every call below fails its host-side checks
    need = q(1000, 3, 2, 5, 2)

    def args(**kw):
        return [kw.get("dtype", 0), kw.get("cov", p), kw.get("m", 1000), kw.get("batch", 2), kw.get("a", p), kw.get("s2", p),
                kw.get("group", p), kw.get("ng", 3), None, kw.get("rows", p), kw.get("nrows", 2), kw.get("nt", 5), kw.get("work", p),
                kw.get("wb", need), kw.get("gain", p), kw.get("var", p), None]

    f = lib.dgp_sample_value
    assert f(*args(dtype=2)) == -1 and b"dtype" in lib.dgp_last_error()
    for name in ("cov", "a", "s2", "group", "gain", "var", "rows"):
        assert f(*args(**{name: None})) == -1 and b"null" in lib.dgp_last_error(), name
    for kw in (dict(m=0), dict(m=(1 << 20) + 1), dict(batch=0), dict(batch=1025), dict(ng=0), dict(ng=65536), dict(nrows=-1),
               dict(nrows=65), dict(nt=0), dict(nt=65)):
        assert f(*args(**kw)) == -1 and b"size" in lib.dgp_last_error(), kw
    assert f(*args(wb=need - 1)) == -3 and b"workspace" in lib.dgp_last_error()
    assert f(*args(work=None)) == -3 and b"workspace" in lib.dgp_last_error()


# ------------------------------------------------------------------------------------------------ the product layer
def test_sample_value_host_logic_groups_weights_and_sample_var():
    model, daily = _loadest()
    mode, s, t = target_transform(model.dm)
    mu, cov = _posterior(model, daily)
    w = flux_weights(daily, {"units": "mg/l"})
    ds = model.sample_value(daily)
    call = SpyPlan.calls[-1]
    m = len(w)
    _o, groups, labels, n_points, _d = period_groups(daily.coords["time"].values, w, "YE")
    assert call["m"] == m and call["ngroups"] == 3 and np.array_equal(call["groups"], groups) and call["rows"] is None
    assert np.allclose(call["a"], w * np.exp(s * mu + t + 0.5 * s * s * np.diagonal(cov)), rtol=1e-12, atol=0)
    assert call["scale2"] == s * s and call["nterms"] == series_terms(s * s * np.diagonal(cov).max())
    assert np.array_equal(call["obs_var"], np.zeros(m))  # no learned noise term: an exact measurement
    gain, _v = direct_gain(cov, call["a"], s * s, groups, 3)
    assert ds["variance_reduction"].values.shape == (3, m) and np.allclose(ds["variance_reduction"].values, gain, rtol=1e-12, atol=0)
    flux = model.annual_flux(daily)
    assert np.allclose(ds["se_now"].values, flux["se"].values, rtol=1e-14, atol=0)
    assert np.array_equal(ds.coords["period"].values, labels) and np.array_equal(ds.coords["time"].values, daily.coords["time"].values)
    var = flux["se"].values ** 2
    assert np.allclose(ds["se_expected"].values, np.sqrt(np.clip(var[:, None] - gain, 0, None)), rtol=1e-10, atol=0)
    assert np.allclose(ds["score"].values, (gain / var[:, None]).sum(axis=0), rtol=1e-10, atol=0)
    assert np.all(gain >= 0) and np.all(gain <= var[:, None] * (1 + 1e-9))  # the law of total variance
    # overrides: a number, a per-day array (in the covariates' order)
    model.sample_value(daily, sample_var=0.04)
    assert np.array_equal(SpyPlan.calls[-1]["obs_var"], np.full(m, 0.04))
    per_day = np.linspace(0.01, 0.09, m)
    noisy = model.sample_value(daily, sample_var=per_day)
    assert np.array_equal(SpyPlan.calls[-1]["obs_var"], per_day)
    assert np.all(noisy["variance_reduction"].values <= gain * (1 + 1e-12))  # a noisier sample is worth less
    for bad in (-0.1, np.nan, np.ones(m - 1)):
        with pytest.raises(ValueError, match="sample_var"):
            model.sample_value(daily, sample_var=bad)
    # a day without flow is dropped like aggregate drops it: no candidate, no group member
    q = np.array(daily["flow"].values, dtype=np.float64)
    q[7] = np.nan
    from discontinuum_amd.xr_compat import Dataset

    holed = Dataset({"flow": ("time", q, {"units": "cubic meters per second"})}, coords={"time": daily.coords["time"].values})
    part = model.sample_value(holed)
    assert part["variance_reduction"].values.shape == (3, m - 1) and SpyPlan.calls[-1]["m"] == m - 1
    with pytest.raises(RuntimeError, match="hasn't been fitted"):
        LoadestGP().sample_value(daily)


def test_rating_defaults_to_the_learned_noise_and_linear_targets_take_one_term():
    cov_obs, target, unc, daily = daily_rating(end="2013-01-01")
    rating = RatingGP()
    rating.fit(cov_obs, target, target_unc=unc, iterations=10)
    stage = np.asarray(daily["stage"].values, dtype=np.float64)
    rating.sample_value(daily, stage)
    call = SpyPlan.calls[-1]
    learned = float(rating.likelihood.second_noise.detach())
    assert learned > 0 and np.array_equal(call["obs_var"], np.full(len(stage), learned)) and call["nterms"] > 1
    ds = rating.design(daily, stage, 2)
    assert ds["time"].values.shape == (2,) and len(set(ds["index"].values.tolist())) == 2
    # a standardised (linear) target: K = 1, A_i = w_i, and the closed form
    model, daily = _loadest("standard")
    mode, s, t = target_transform(model.dm)
    assert mode == 0
    w = flux_weights(daily, {"units": "mg/l"})
    ds = model.sample_value(daily, sample_var=0.02)
    call = SpyPlan.calls[-1]
    assert call["nterms"] == 1 and np.array_equal(call["a"], w)
    _mu, cov = _posterior(model, daily)
    _o, groups, _l, _n, _d = period_groups(daily.coords["time"].values, w, "YE")
    assert np.allclose(ds["variance_reduction"].values, linear_gain(cov, w, s * s, groups, 3, np.full(len(w), 0.02)), rtol=1e-12, atol=0)


def test_design_value_hands_period_moments_the_shifted_mean():
    model, daily = _loadest()
    mode, s, t = target_transform(model.dm)
    mu, cov = _posterior(model, daily)
    w = flux_weights(daily, {"units": "mg/l"})
    time = daily.coords["time"].values
    S = [10, 95, 96, 200]
    tau2 = np.full(len(w), 0.03)
    ds, V = model.design_value(daily, time[S], sample_var=0.03, return_cov=True)
    call = SpyPlan.moments[-1]
    R = explained_cov(cov, S, tau2)
    assert np.allclose(call["cov"], R, rtol=0, atol=1e-12 * np.abs(R).max())  # the recurrence against the dense solve
    assert np.allclose(call["mu"], s * mu + t + 0.5 * s * s * (np.diagonal(cov) - np.diagonal(R)), rtol=1e-13, atol=0)
    assert np.array_equal(call["w"], w) and call["mode"] == mode
    _o, groups, _l, _n, _d = period_groups(time, w, "YE")
    a = w * np.exp(s * mu + t + 0.5 * s * s * np.diagonal(cov))
    ref = design_value_ref(cov, a, s * s, groups, 3, S, tau2)
    assert np.allclose(V, ref, rtol=0, atol=1e-11 * np.abs(ref).max())
    flux = model.annual_flux(daily)
    var = flux["se"].values ** 2
    assert np.allclose(ds["se_now"].values, flux["se"].values) and np.allclose(ds["variance_explained"].values, np.diagonal(V))
    assert np.allclose(ds["se_expected"].values, np.sqrt(var - np.diagonal(V))) and np.allclose(ds["fraction"].values, np.diagonal(V) / var)
    assert np.all(np.diagonal(V) > 0) and np.all(np.diagonal(V) < var)
    by_index = model.design_value(daily, S, sample_var=0.03)  # indices select the same days
    assert np.array_equal(by_index["variance_explained"].values, ds["variance_explained"].values)
    # one sample: V_pp(S) is the gain map's column
    one = model.design_value(daily, [95], sample_var=0.03)
    gain = model.sample_value(daily, sample_var=0.03)["variance_reduction"].values
    assert np.allclose(one["variance_explained"].values, gain[:, 95], rtol=1e-10, atol=0)


def test_greedy_design_follows_the_reference_and_given_continues_it():
    model, daily = _loadest()
    mode, s, t = target_transform(model.dm)
    mu, cov = _posterior(model, daily)
    w = flux_weights(daily, {"units": "mg/l"})
    time = daily.coords["time"].values
    _o, groups, labels, _n, _d = period_groups(time, w, "YE")
    a = w * np.exp(s * mu + t + 0.5 * s * s * np.diagonal(cov))
    tau2 = np.full(len(w), 0.02)
    var = model.annual_flux(daily)["se"].values ** 2
    for objective, omega in (("relative", 1 / var), ("absolute", np.ones(3)), (labels[1], np.array([0.0, 1.0, 0.0]))):
        picks, tops = greedy_ref(cov, a, s * s, groups, 3, 4, omega, tau2)
        assert all(b < a_ * (1 - 1e-9) for a_, b in tops)
        ds = model.design(daily, 4, objective=objective, sample_var=0.02)
        assert ds["index"].values.tolist() == picks and np.array_equal(ds["time"].values, time[picks])
        assert np.allclose(ds["score"].values, [a_ for a_, _b in tops], rtol=1e-9, atol=0)
        assert len(set(picks)) == 4
        # the reported values: exact, nested, non-decreasing, below Var
        for j in range(4):
            ref = np.diagonal(design_value_ref(cov, a, s * s, groups, 3, picks[: j + 1], tau2))
            assert np.allclose(ds["variance_explained"].values[j], ref, rtol=0, atol=1e-11 * ref.max())
        ve = ds["variance_explained"].values
        assert np.all(np.diff(ve, axis=0) >= -1e-12 * var[None, :]) and np.all(ve <= var[None, :])
    rel = model.design(daily, 4, sample_var=0.02)
    cont = model.design(daily, 2, given=time[rel["index"].values[:2]], sample_var=0.02)
    assert cont["index"].values.tolist() == rel["index"].values[2:].tolist()
    assert np.allclose(cont["variance_explained"].values, rel["variance_explained"].values[2:], rtol=1e-10, atol=0)
    # candidates restrict the choice; replicates may repeat a day
    mask = np.zeros(len(w), dtype=bool)
    mask[[3, 50, 120]] = True
    some = model.design(daily, 3, candidates=mask, sample_var=0.02)
    assert sorted(some["index"].values.tolist()) == [3, 50, 120]
    rep = model.design(daily, 3, candidates=[50], replicates=True, sample_var=0.02)
    assert rep["index"].values.tolist() == [50, 50, 50] and np.all(np.diff(rep["variance_explained"].values, axis=0) > 0)


def test_error_paths():
    model, daily = _loadest()
    with pytest.raises(ValueError, match=r"footprint of \d+ bytes.*max_bytes = 100000"):
        model.sample_value(daily, max_bytes=100_000)
    with pytest.raises(ValueError, match=r"second \(M, M\) buffer.*footprint of \d+ bytes"):
        model.design_value(daily, [1], max_bytes=100_000)
    assert not SpyPlan.calls and not SpyPlan.moments
    with pytest.raises(ValueError, match="2011-06-01 is not a day of the record"):
        model.design_value(daily, [np.datetime64("2011-06-01")])
    with pytest.raises(ValueError, match="given: 2030-01-01"):
        model.sample_value(daily, given=["2030-01-01"])
    with pytest.raises(ValueError, match="out of range"):
        model.design_value(daily, [10_000])
    with pytest.raises(ValueError, match="k = 3 exceeds the 2 candidate days"):
        model.design(daily, 3, candidates=[4, 9])
    with pytest.raises(ValueError, match="at most 64"):
        model.design(daily, 65)
    with pytest.raises(ValueError, match="objective"):
        model.design(daily, 2, objective="best")
    with pytest.raises(ValueError, match="none of the period labels"):
        model.design(daily, 2, objective="1999-12-31")
    # a NaN on the diagonal is refused with beta; one off the diagonal comes out of the kernel as a NaN gain of the two
    # days it joins: the greedy loop names the first
    real = SpyPlan.posterior_cov

    def poisoned(self, theta, Xs):
        mu, cov = real(self, theta, Xs)
        cov[9, 5] = float("nan")
        return mu, cov

    SpyPlan.posterior_cov = poisoned
    try:
        with pytest.raises(ValueError, match=r"score of \d{4}-\d\d-\d\d \(point 5\) is NaN"):
            model.design(daily, 2, objective="absolute", sample_var=0.02)
    finally:
        del SpyPlan.posterior_cov


def test_design_value_matches_simulated_samples():
    """|S| = 3, 200 000 seeded draws of y_S: E[L_p | y_S] from the closed form of the conditional lognormal mean; its sample
    covariance lies within 5 Monte Carlo standard errors of V(S), entry by entry."""
    model, daily = _loadest()
    mode, s, t = target_transform(model.dm)
    mu, cov = _posterior(model, daily)
    w = flux_weights(daily, {"units": "mg/l"})
    S, tau2 = [20, 110, 190], 0.03
    _ds, V = model.design_value(daily, S, sample_var=tau2, return_cov=True)
    _o, groups, _l, _n, _d = period_groups(daily.coords["time"].values, w, "YE")
    G = cov[np.ix_(S, S)] + tau2 * np.eye(3)
    gain_mat = cov[:, S] @ np.linalg.inv(G)  # (m, 3)
    cond_var = np.diagonal(cov) - np.einsum("ij,ij->i", gain_mat, cov[:, S])
    rng = np.random.default_rng(4)
    dy = rng.standard_normal((NDRAW, 3)) @ np.linalg.cholesky(G).T  # y_S - mu_S
    A = np.zeros((len(w), 3))
    A[np.arange(len(w)), groups] = 1.0
    loads = np.empty((NDRAW, 3))
    for i0 in range(0, NDRAW, 20_000):
        cm = mu[None, :] + dy[i0:i0 + 20_000] @ gain_mat.T
        loads[i0:i0 + 20_000] = (w[None, :] * np.exp(s * cm + t + 0.5 * s * s * cond_var[None, :])) @ A
    d = loads - loads.mean(axis=0)
    for p in range(3):
        for q in range(p, 3):
            prod = d[:, p] * d[:, q]
            assert abs(V[p, q] - prod.mean()) <= 5 * prod.std(ddof=1) / np.sqrt(NDRAW), (p, q, V[p, q], prod.mean())
