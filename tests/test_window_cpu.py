"""Rolling-window statistics (``rolling.time_windows``, ``MarginalHIP.rolling_mean``, the ``window=`` keyword of
``exceedance`` / ``duration_curve`` / ``exceedance_probability``) on CPU: the window builder against a brute-force loop, the
dense reference of tests/window_helpers.py against draws, the host logic against a seeded Monte Carlo of the reference
workflow (posterior draws, rolled, compared and counted per period) with the device plan replaced by an oracle-backed double,
the refusals, the budget, the host-side checks of ``backend.window_moments`` and the new C entries' argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.stats import norm

from discontinuum_amd import _lib, backend
from discontinuum_amd.engines.base import ModelConfig
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.loads import intervals, period_groups, target_transform
from discontinuum_amd.rolling import time_windows
from tests.exceedance_helpers import dense_exceedance_moments
from tests.flux_helpers import daily_loadest, gaussian_draws, one_hot
from tests.window_helpers import WindowOraclePlan, brute_time_windows, dense_window_moments, irregular_times, trailing

DAY = 86400 * 10 ** 9


class SpyPlan(WindowOraclePlan):
    """Records what the product hands to ``window_moments`` and ``exceedance_moments``."""

    windows: list = []
    counts: list = []

    def window_moments(self, cov, m, mu, lo, hi, a=None, mode=0, scale2=None):
        SpyPlan.windows.append(dict(m=m, lo=np.asarray(lo).copy(), hi=np.asarray(hi).copy(), mode=mode, scale2=scale2))
        return super().window_moments(cov, m, mu, lo, hi, a=a, mode=mode, scale2=scale2)

    def exceedance_moments(self, cov, m, mu, thresh, w, groups, ngroups, extra_var=None):
        SpyPlan.counts.append(dict(m=m, groups=np.asarray(groups).copy(), extra_var=extra_var))
        return super().exceedance_moments(cov, m, mu, thresh, w, groups, ngroups, extra_var)


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(SpyPlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)
    SpyPlan.windows, SpyPlan.counts = [], []


_MODELS = {}


def _loadest(transform="log"):
    if transform not in _MODELS:
        cov_obs, target, daily = daily_loadest(seed=0)
        model = LoadestGP() if transform == "log" else LoadestGP(model_config=ModelConfig(transform=transform))
        model.fit(cov_obs, target, iterations=10)
        _MODELS[transform] = (model, daily)
    return _MODELS[transform]


def _posterior(model, daily):
    model._ensure_factor()
    x = torch.tensor(model.dm.Xnew(daily), dtype=torch.float64)
    kmean, cov = model._plan.posterior_cov(model._factor_theta, x)
    return (kmean + model.model.prior_mean(x)).detach().numpy(), cov.numpy().copy()


# ------------------------------------------------------------------------------------------------ the window builder
def _times(name):
    day = np.datetime64("2012-01-01", "ns")
    if name == "daily":
        return day + np.arange(120) * np.timedelta64(DAY, "ns")
    if name == "gaps":
        keep = np.r_[0:40, 55:90, 150:200]
        return day + keep * np.timedelta64(DAY, "ns")
    if name == "irregular":
        return irregular_times(150, seed=2)
    if name == "duplicates":
        d = np.sort(np.r_[np.arange(60), [10, 10, 25, 59]])
        return day + d * np.timedelta64(DAY, "ns")
    raise KeyError(name)


@pytest.mark.parametrize("name", ["daily", "gaps", "irregular", "duplicates"])
@pytest.mark.parametrize("align", ["right", "center"])
def test_time_windows_against_a_brute_force_loop(name, align):
    t = _times(name)
    rng = np.random.default_rng(1)
    perm = rng.permutation(len(t))  # the record need not come sorted
    shuffled = t[perm]
    for window, ns in (("30D", 30 * DAY), ("7D", 7 * DAY), ("96h", 4 * DAY), (np.timedelta64(31, "D"), 31 * DAY)):
        order, lo, hi, keep = time_windows(shuffled, window, align=align)
        ts = shuffled[order].astype(np.int64)
        assert np.all(np.diff(ts) >= 0) and sorted(order) == list(range(len(t)))
        blo, bhi = brute_time_windows(ts, ns, align)
        live = bhi > blo
        assert live.all() and np.array_equal(lo, blo) and np.array_equal(hi, bhi)
        assert lo.dtype == np.int32 and hi.dtype == np.int32 and np.all(np.diff(lo) >= 0) and np.all(np.diff(hi) >= 0)
        assert np.array_equal(keep, (bhi - blo) == (bhi - blo).max())  # the default: the fullest windows only
        for k in (1, 3):
            assert np.array_equal(time_windows(shuffled, window, align=align, min_periods=k)[3], (bhi - blo) >= k)


def test_time_windows_defaults_and_dropped_points():
    t = _times("daily")
    order, lo, hi, keep = time_windows(t, "30D")
    assert np.array_equal(hi - lo, np.minimum(np.arange(120) + 1, 30))
    assert not keep[:29].any() and keep[29:].all()  # the leading partial windows are excluded
    holed = t.copy()
    holed[5] = np.datetime64("NaT")
    valid = np.ones(120, bool)
    valid[50] = False
    order, lo, hi, keep = time_windows(holed, "30D", valid=valid)
    assert len(order) == 118 and 5 not in order and 50 not in order
    assert (hi - lo).max() == 30 and keep.sum() < 118 - 29  # windows over the two holes hold 29 points
    with pytest.raises(ValueError, match="align"):
        time_windows(t, "30D", align="left")
    for bad in ("ME", "-3D", "nonsense"):
        with pytest.raises(ValueError, match="window"):
            time_windows(t, bad)
    with pytest.raises(ValueError, match="min_periods"):
        time_windows(t, "30D", min_periods=0)


# ------------------------------------------------------------------------------------------------ the dense reference
def test_dense_reference_against_draws_on_a_toy():
    """m = 40, w = 7, 200 000 draws: the rolling means of the draws (mode 0) and of their exponentials (mode 1) have the
    reference's mean and covariance, and the counts of rolling means above a level have the moments the exceedance
    reference gives on the windowed covariance: all within 5 Monte Carlo standard errors."""
    rng = np.random.default_rng(0)
    m, w, n = 40, 7, 200_000
    i = np.arange(m)
    Cm = 0.6 * np.exp(-np.abs(i[:, None] - i[None, :]) / 5.0) + 0.05 * np.eye(m)
    mu = 0.3 * rng.standard_normal(m)
    a = rng.uniform(0.5, 2.0, m)
    lo, hi = trailing(m, w)
    draws = np.concatenate(list(gaussian_draws(mu, Cm, n, seed=1)))
    s2 = 0.8
    for mode in (0, 1):
        mean, S = dense_window_moments(Cm, mu, lo, hi, a, mode, s2)
        vals = draws if mode == 0 else np.exp(draws * np.sqrt(s2) + (1 - np.sqrt(s2)) * mu[None, :])  # mean mu, variance s2 C
        W = np.zeros((m, m))
        for k in range(m):
            W[k, lo[k]:hi[k]] = a[lo[k]:hi[k]] / a[lo[k]:hi[k]].sum()
        roll = vals @ W.T
        z = np.abs(mean - roll.mean(axis=0)) / (roll.std(axis=0, ddof=1) / np.sqrt(n))
        assert np.all(z < 5), (mode, z.max())
        d = roll - roll.mean(axis=0)
        for p, r in ((0, 0), (10, 10), (10, 12), (10, 20), (39, 33), (39, 39)):
            prod = d[:, p] * d[:, r]
            assert abs(S[p, r] - prod.mean()) < 5 * prod.std(ddof=1) / np.sqrt(n), (mode, p, r)
        if mode == 0:  # counts of rolling means above a level, two groups
            g = (i // 20).astype(np.int32)
            u = np.full((1, m), 0.1)
            cmean, ccov = dense_exceedance_moments(S, mean, u, np.ones(m), g, 2)
            counts = (roll > 0.1).astype(np.float64) @ one_hot(g, 2)
            zc = np.abs(cmean[0] - counts.mean(axis=0)) / (counts.std(axis=0, ddof=1) / np.sqrt(n))
            assert np.all(zc < 5), zc
            dc = counts - counts.mean(axis=0)
            for p, r in ((0, 0), (0, 1), (1, 1)):
                prod = dc[:, p] * dc[:, r]
                assert abs(ccov[0, p, r] - prod.mean()) < 5 * prod.std(ddof=1) / np.sqrt(n), (p, r)


# ------------------------------------------------------------------------------------------------ the product layer
def test_rolling_mean_of_a_log_target_is_exact_through_the_monotone_map():
    model, daily = _loadest()
    mode, s, t = target_transform(model.dm)
    assert mode == 1
    mu, cov = _posterior(model, daily)
    m = len(mu)
    ds, S = model.rolling_mean(daily, "30D", return_cov=True)
    lo, hi = trailing(m, 30)
    rmean, rS = dense_window_moments(cov, mu, lo[29:], hi[29:])
    assert ds["mean"].values.shape == (m - 29,) and np.all(ds["n_points"].values == 30)
    assert np.array_equal(ds.coords["time"].values, daily.coords["time"].values[29:])
    assert np.allclose(S, rS, rtol=0, atol=1e-14)
    sd = np.sqrt(np.diagonal(rS))
    z = norm.ppf(0.975)
    assert np.allclose(ds["mean"].values, np.exp(s * rmean + t), rtol=1e-13, atol=0)
    assert np.allclose(ds["lower"].values, np.exp(s * (rmean - z * sd) + t), rtol=1e-12, atol=0)
    assert np.allclose(ds["upper"].values, np.exp(s * (rmean + z * sd) + t), rtol=1e-12, atol=0)
    se = np.asarray(model.dm.error_pipeline.inverse_transform(np.diagonal(rS)).values).reshape(-1)
    assert np.allclose(ds["se"].values, se, rtol=1e-10, atol=0)
    assert ds.attrs["statistic"] == "geometric_mean" and ds["lower"].attrs["interval"] == "exact"
    call = SpyPlan.windows[-1]
    assert call["mode"] == backend.MODE_LINEAR and call["m"] == m and len(call["lo"]) == m - 29
    # the arithmetic mean: mode 1, exact moments, an approximate interval
    am, aS = model.rolling_mean(daily, "30D", statistic="mean", return_cov=True)
    call = SpyPlan.windows[-1]
    assert call["mode"] == backend.MODE_LOG and np.isclose(call["scale2"], s * s)
    amean, aref = dense_window_moments(cov, s * mu + t, lo[29:], hi[29:], None, 1, s * s)
    assert np.allclose(am["mean"].values, amean, rtol=1e-13, atol=0) and np.allclose(aS, aref, rtol=1e-10, atol=1e-18)
    assert np.allclose(am["se"].values, np.sqrt(np.diagonal(aref)), rtol=1e-10, atol=0)
    lower, upper = intervals(1, amean, np.diagonal(aref))
    assert np.allclose(am["lower"].values, lower) and np.allclose(am["upper"].values, upper)
    assert am.attrs["statistic"] == "mean" and "approximate" in am["lower"].attrs["interval"]
    assert np.all(am["mean"].values >= ds["mean"].values)  # AM >= GM
    # centred windows, an explicit min_periods
    c = model.rolling_mean(daily, "31D", align="center", min_periods=16)
    assert c["mean"].values.shape == (m,) and c["n_points"].values.min() == 16 and c["n_points"].values.max() == 31
    with pytest.raises(ValueError, match="statistic"):
        model.rolling_mean(daily, "30D", statistic="median")


def test_rolling_mean_of_a_linear_target():
    model, daily = _loadest("standard")
    mode, s, t = target_transform(model.dm)
    assert mode == 0
    mu, cov = _posterior(model, daily)
    ds = model.rolling_mean(daily, "7D")
    lo, hi = trailing(len(mu), 7)
    rmean, rS = dense_window_moments(cov, mu, lo[6:], hi[6:])
    assert ds.attrs["statistic"] == "mean"
    assert np.allclose(ds["mean"].values, s * rmean + t, rtol=1e-12, atol=1e-12)
    z = norm.ppf(0.975)
    assert np.allclose(ds["upper"].values - ds["lower"].values, 2 * z * abs(s) * np.sqrt(np.diagonal(rS)), rtol=1e-9, atol=1e-12)
    with pytest.raises(ValueError, match="geometric"):
        model.rolling_mean(daily, "7D", statistic="geometric_mean")


def test_windowed_exceedance_matches_the_sampling_workflow():
    """Draw, roll (30-day geometric mean = rolling mean in model space), compare with the criterion, count per year."""
    model, daily = _loadest()
    _mode, s, t = target_transform(model.dm)
    mu, cov = _posterior(model, daily)
    m = len(mu)
    gm = np.exp(s * dense_window_moments(cov, mu, *trailing(m, 30))[0] + t)
    level = float(np.quantile(gm[29:], 0.55))
    ds, pcov = model.exceedance(daily, threshold=level, window="30D", freq="YE", return_cov=True)
    assert ds["mean"].values.shape == (1, 3) and list(ds["n_points"].values) == [366 - 29, 365, 365]
    call = SpyPlan.counts[-1]
    assert call["m"] == m and np.all(call["groups"][:29] == -1) and np.all(call["groups"][29:] >= 0) and call["extra_var"] is None
    time = daily.coords["time"].values
    _o, groups, labels, _n, _d = period_groups(time, np.ones(m), "YE")
    groups = groups.copy()
    groups[:29] = -1
    A = one_hot(groups, len(labels))
    u = (np.log(level) - t) / s
    counts = []
    for f in gaussian_draws(mu, cov, 100_000, seed=3):
        cs = np.concatenate([np.zeros((f.shape[0], 1)), np.cumsum(f, axis=1)], axis=1)
        roll = np.full_like(f, -np.inf)
        roll[:, 29:] = (cs[:, 30:] - cs[:, :-30]) / 30.0
        counts.append((roll > u).astype(np.float64) @ A)
    counts = np.concatenate(counts)
    n = counts.shape[0]
    mean = ds["mean"].values[0]
    sd = counts.std(axis=0, ddof=1)
    assert np.all(np.abs(mean - counts.mean(axis=0)) < 5 * sd / np.sqrt(n) + 1e-9), (mean, counts.mean(axis=0))
    d = counts - counts.mean(axis=0)
    for a in range(3):
        for b in range(a, 3):
            prod = d[:, a] * d[:, b]
            assert abs(pcov[0, a, b] - prod.mean()) <= 5 * prod.std(ddof=1) / np.sqrt(n) + 1e-9, (a, b)
    assert np.allclose(np.sqrt(np.diagonal(pcov[0])), ds["se"].values[0])
    # the duration curve of the rolling mean is the whole record as one group
    dc = model.duration_curve(daily, levels=[level], window="30D")
    assert dc.attrs["n_points"] == m - 29
    assert np.isclose(dc["mean"].values[0] * (m - 29), mean.sum(), rtol=0, atol=1e-9)
    default = model.duration_curve(daily, window="30D")
    f = default["mean"].values
    assert f.shape == (21,) and np.all(np.diff(f) <= 1e-12) and f[0] > 0.5 > f[-1]
    # the pointwise probability comes from the diagonal of the windowed covariance
    p = model.exceedance_probability(daily, level, window="30D")
    wm, S = dense_window_moments(cov, mu, *(v[29:] for v in trailing(m, 30)))
    assert p.dims == ("time",) and np.allclose(p.values, norm.cdf((wm - u) / np.sqrt(np.diagonal(S))), rtol=0, atol=1e-12)
    assert np.isclose(p.values.sum(), mean.sum(), rtol=0, atol=1e-8)


def test_without_a_window_nothing_changes_and_the_budget_holds():
    model, daily = _loadest()
    tau = [0.8, 1.2]
    from discontinuum_amd import exceedance as ex

    old = ex._exceedance(model, daily, threshold=tau, return_cov=True)
    new = model.exceedance(daily, threshold=tau, return_cov=True, window=None)
    assert np.array_equal(old[1], new[1])
    for k in ("mean", "se", "lower", "upper", "n_points"):
        assert np.array_equal(old[0][k].values, new[0][k].values)
    assert not SpyPlan.windows  # the daily product never calls the windowing pass
    a, b = model.duration_curve(daily, levels=tau), model.duration_curve(daily, levels=tau, window=None)
    assert np.array_equal(a["mean"].values, b["mean"].values) and np.array_equal(a["se"].values, b["se"].values)
    p, q = model.exceedance_probability(daily, 1.0), model.exceedance_probability(daily, 1.0, window=None)
    assert np.array_equal(p.values, q.values)
    # "1D" on a gap-free daily record is the daily product
    one = model.exceedance(daily, threshold=tau, window="1D")
    assert np.allclose(one["mean"].values, new[0]["mean"].values, rtol=0, atol=1e-10)
    assert np.array_equal(one["n_points"].values, new[0]["n_points"].values)
    SpyPlan.windows, SpyPlan.counts = [], []
    for call in (lambda: model.exceedance(daily, threshold=1.0, window="30D", max_bytes=20_000_000),
                 lambda: model.rolling_mean(daily, "30D", max_bytes=20_000_000),
                 lambda: model.duration_curve(daily, levels=[1.0], window="30D", max_bytes=20_000_000),
                 lambda: model.exceedance_probability(daily, 1.0, window="30D", max_bytes=20_000_000)):
        with pytest.raises(ValueError, match=r"footprint of \d+ bytes.*max_bytes = 20000000"):
            call()
    assert not SpyPlan.windows and not SpyPlan.counts
    # the dense daily product fits the same budget: the window's share is what exceeds it
    model.exceedance(daily, threshold=1.0, max_bytes=20_000_000)


def test_the_refusals_say_why():
    model, daily = _loadest()
    with pytest.raises(NotImplementedError, match="row halo"):
        model.exceedance(daily, threshold=1.0, window="30D", streamed=True)
    with pytest.raises(ValueError, match="noise of an averaged"):
        model.exceedance(daily, threshold=1.0, window="30D", pred_noise=True)
    with pytest.raises(NotImplementedError, match="flux"):
        model.exceedance(daily, threshold=1.0, window="30D", kind="flux")
    with pytest.raises(NotImplementedError, match="sum of\\s+lognormals"):
        model.exceedance(daily, threshold=1.0, window="30D", statistic="mean")
    with pytest.raises(NotImplementedError, match="sum of\\s+lognormals"):
        model.duration_curve(daily, levels=[1.0], window="30D", statistic="mean")
    with pytest.raises(NotImplementedError, match="row halo"):
        model.duration_curve(daily, levels=[1.0], window="30D", streamed=True)
    with pytest.raises(ValueError, match="noise of an averaged"):
        model.exceedance_probability(daily, 1.0, window="30D", pred_noise=True)
    assert not SpyPlan.windows


# ------------------------------------------------------------------------------------------------ the backend and the C entries
def test_backend_window_moments_checks_its_windows_on_the_host():
    m = 10
    cov = torch.zeros(128, 128, dtype=torch.float64)
    mu = torch.zeros(m, dtype=torch.float64)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    good_lo, good_hi = i32([0, 0, 2]), i32([1, 3, 10])
    cases = {
        "int32": (torch.tensor([0, 0, 2]), good_hi),
        "int32 ": (good_lo, torch.tensor([1.0, 3.0, 10.0])),
        "shape": (i32([[0, 0, 2]]), i32([[1, 3, 10]])),
        "shape ": (good_lo, i32([1, 3])),
        "range": (i32([-1, 0, 2]), good_hi),
        "range ": (good_lo, i32([1, 3, 11])),
        "range  ": (i32([0, 4, 5]), i32([1, 3, 10])),
        "non-decreasing": (i32([0, 2, 1]), good_hi),
        "non-decreasing ": (good_lo, i32([3, 2, 10])),
    }
    for what, (lo, hi) in cases.items():
        with pytest.raises(ValueError, match=what.strip()):
            backend.window_moments(cov, m, mu, lo, hi)
    with pytest.raises(ValueError, match="shape"):
        backend.window_moments(torch.zeros(2, 128, 128, dtype=torch.float64), m, torch.zeros(2, m, dtype=torch.float64), good_lo, good_hi)
    with pytest.raises(ValueError, match="scale2"):
        backend.window_moments(cov, m, mu, good_lo, good_hi, mode=backend.MODE_LOG)
    with pytest.raises(ValueError, match="CUDA"):  # good windows get as far as the covariance check
        backend.window_moments(cov, m, mu, good_lo, good_hi)


def test_window_abi_without_a_device():
    lib = _lib.load()
    q = lib.dgp_window_moments_workspace_bytes
    M, Q = lib.dgp_padded_n(1000), lib.dgp_padded_n(300)
    need = q(1000, 300, 2)
    assert need == 2 * 8 * (M * Q + 2 * M + 2 * Q)
    assert q(2000, 300, 2) > need and q(1000, 400, 2) > need and q(1000, 300, 3) > need
    for bad in ((0, 3, 1), ((1 << 20) + 1, 3, 1), (10, 0, 1), (10, (1 << 20) + 1, 1), (10, 3, 0), (10, 3, 1025)):
        assert q(*bad) == 0, bad
    p = C.c_void_p(16)  # never dereferenced: every call below fails its host-side checks

    def args(**kw):
        return [kw.get("dtype", 0), kw.get("mode", 0), kw.get("cov", p), kw.get("m", 1000), kw.get("batch", 2), kw.get("mu", p),
                kw.get("scale2", p), None, kw.get("lo", p), kw.get("hi", p), kw.get("q", 300), kw.get("work", p), kw.get("wb", need),
                kw.get("mean", p), kw.get("covo", p), None]

    f = lib.dgp_window_moments
    assert f(*args(dtype=2)) == _lib.E_ARG and b"dtype" in lib.dgp_last_error()
    assert f(*args(mode=2)) == _lib.E_ARG and b"mode" in lib.dgp_last_error()
    for name in ("cov", "mu", "lo", "hi", "mean", "covo"):
        assert f(*args(**{name: None})) == _lib.E_ARG and b"null" in lib.dgp_last_error(), name
    assert f(*args(mode=1, scale2=None)) == _lib.E_ARG and b"null" in lib.dgp_last_error()
    for kw in (dict(m=0), dict(m=(1 << 20) + 1), dict(q=0), dict(q=(1 << 20) + 1), dict(batch=0), dict(batch=1025)):
        assert f(*args(**kw)) == _lib.E_ARG and b"size" in lib.dgp_last_error(), kw
    assert f(*args(wb=need - 1)) == _lib.E_WORKSPACE and b"workspace" in lib.dgp_last_error()
    assert f(*args(work=None)) == _lib.E_WORKSPACE and b"workspace" in lib.dgp_last_error()
    assert f(*args(work=C.c_void_p(20))) == _lib.E_ARG and b"aligned" in lib.dgp_last_error()
