"""The exact skewness of period loads on CPU: the closed form of the third central moment against brute-force raw moments, the
three-moment (shifted lognormal) fit, both against a seeded Monte Carlo on storm-dominated records, the host path
(``annual_flux`` / ``aggregate`` / ``annual_flux_many`` with ``interval="three-moment"``) over an oracle-backed plan, and the
C entry's argument checks without a device."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.stats import norm

from discontinuum_amd import _lib, backend, loads
from discontinuum_amd.engines.base import ModelConfig
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.loads import (_site_bytes, _third_moment_bytes, annual_flux_many, intervals, period_groups, target_transform,
                                    three_moment_fit, three_moment_intervals)
from tests.flux_helpers import daily_loadest, dense_period_moments, gaussian_draws
from tests.skew_helpers import SkewOraclePlan, brute_third_moments, dense_third_moments, storm_record

NDRAW = 200_000


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(SkewOraclePlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    monkeypatch.setattr(backend, "GPPlan", SkewOraclePlan)  # aggregate_many builds its plans itself
    torch.manual_seed(0)


# ------------------------------------------------------------------------------------------------ 1. the closed form
@pytest.mark.parametrize("m", [1, 2, 65, 130])
def test_closed_form_against_brute_force(m):
    """k3 by the subtraction-free closed form against M3 - 3 M1 M2 + 2 M1^3 (triple einsum) on a random positive-definite
    covariance of rank 3 + a ridge (about half of its entries negative for m > 2): one period, several periods with excluded
    points, with and without extra_var.  1e-10 relative, on periods with cv >= 0.1 (all of them here: asserted)."""
    rng = np.random.default_rng(100 + m)
    B = rng.standard_normal((m, 3)) * 0.45
    cov = B @ B.T + 0.05 * np.eye(m)
    if m > 2:
        assert 0.3 < np.mean(cov < 0) < 0.7
    mu, w = 0.3 * rng.standard_normal(m), rng.uniform(0.5, 2.0, m)
    ev = rng.uniform(0.0, 0.1, m)
    layouts = {"one": np.zeros(m, np.int64)}
    if m > 2:
        g = np.minimum(np.arange(m) // (m // 3), 2)
        g[[0, m // 2, m - 1]] = -1
        layouts["three, holes"] = g
    for name, g in layouts.items():
        P = int(g.max()) + 1
        for extra in (None, ev):
            k3 = dense_third_moments(cov, mu, 0.8, w, g, P, extra).numpy()
            ref, cv = brute_third_moments(cov, mu, 0.8, w, g, P, extra)
            assert np.all(cv >= 0.1), (m, name, cv)
            err = np.abs(k3 - ref) / np.abs(ref)
            print(f"m = {m} {name} extra_var = {extra is not None}: cv {cv.min():.3f}..{cv.max():.3f}, closed form vs brute force {err.max():.2e}")
            assert np.all(err <= 1e-10), (m, name, err)
            assert np.all(k3 > 0)


# ------------------------------------------------------------------------------------------------ 2. the fit
def test_the_fit_solves_its_equation_and_reproduces_the_moments():
    gam = np.logspace(-6, np.log10(50.0), 400)
    u, sigma, rel = three_moment_fit(gam)  # u = omega - 1
    assert np.max(np.abs((u + 3.0) * np.sqrt(u) - gam) / gam) <= 1e-13  # (omega + 2) sqrt(omega - 1) = gamma
    # the closed form of the issue, where it is well conditioned (omega - 1 is not lost to cancellation)
    big = gam > 0.1
    r = np.sqrt(gam ** 2 + gam ** 4 / 4)
    omega = np.cbrt(1 + gam ** 2 / 2 + r) + np.cbrt(1 + gam ** 2 / 2 - r) - 1
    assert np.max(np.abs(omega[big] - 1 - u[big]) / u[big]) <= 1e-12
    # mean, variance and skewness of shift + scale exp(sigma Z) at mean = 7, sd = 3
    mean, sd = 7.0, 3.0
    scale, om = rel * sd, 1.0 + u
    shift = mean - scale * np.sqrt(om)
    # E X - mean = scale (exp(sigma^2 / 2) - sqrt(omega)), both taken relative to 1 (the shift is -9e6 at gamma = 1e-6)
    assert np.max(scale * np.abs(np.expm1(0.5 * sigma ** 2) - u / (np.sqrt(om) + 1))) <= 1e-12 * sd
    assert np.max(np.abs(scale ** 2 * om * u / sd ** 2 - 1)) <= 1e-12
    assert np.max(np.abs((om + 2) * np.sqrt(u) / gam - 1)) <= 1e-12
    assert np.max(np.abs(sigma ** 2 - np.log1p(u))) <= 1e-12 * np.max(sigma ** 2)
    # the interval's ends are the fitted distribution's quantiles (where the shift is resolved: gamma >= 1e-3)
    ok = gam >= 1e-3
    lo, hi, clipped = three_moment_intervals(np.full_like(gam, mean), np.full_like(gam, sd ** 2), gam, ci=0.9)
    free = ok & (lo > 0)
    assert np.max(np.abs(norm.cdf(np.log((lo[free] - shift[free]) / scale[free]) / sigma[free]) - 0.05)) <= 1e-9
    assert np.max(np.abs(norm.cdf(np.log((hi[ok] - shift[ok]) / scale[ok]) / sigma[ok]) - 0.95)) <= 1e-9
    assert clipped == int(np.count_nonzero(lo == 0.0)) and np.all(lo >= 0)


def test_one_day_period_is_the_lognormal_interval():
    """One lognormal day: mean a, variance a^2 e, skewness (e + 3) sqrt(e) with e = expm1(s2 c) -- the fit has omega = 1 + e and
    shift 0, i.e. the lognormal interval itself.  The two are different expressions of the same numbers, about twenty rounded
    operations each with factors |z sigma| <= 2 behind them: 1e-13 relative."""
    e = np.expm1(np.array([0.01, 0.1, 0.5, 1.0]))
    a = np.array([3.0, 0.2, 11.0, 1.0])
    mean, var, skew = a, a * a * e, (e + 3.0) * np.sqrt(e)
    for ci in (0.5, 0.95):
        lo3, hi3 = intervals(backend.MODE_LOG, mean, var, ci, interval="three-moment", skew=skew)
        lo2, hi2 = intervals(backend.MODE_LOG, mean, var, ci)
        assert np.max(np.abs(lo3 / lo2 - 1)) <= 1e-13 and np.max(np.abs(hi3 / hi2 - 1)) <= 1e-13


def test_small_skewness_joins_the_normal_interval():
    mean, sd, z = 5.0, 2.0, norm.ppf(0.975)
    for gam in (1e-8, 1e-6, 1e-4, 1e-2):  # Cornish-Fisher: the quantile is mean + sd (z + gamma (z^2 - 1) / 6) + O(gamma^2)
        lo, hi, _ = three_moment_intervals(mean, sd ** 2, gam)
        first = gam * (z * z - 1) / 6
        assert abs((lo - mean) / sd - (-z + first)) <= 2 * gam ** 2 + 1e-14
        assert abs((hi - mean) / sd - (z + first)) <= 2 * gam ** 2 + 1e-14
    below = three_moment_intervals(mean, sd ** 2, 0.9e-8)
    assert below[:2] == intervals(backend.MODE_LINEAR, mean, sd ** 2)  # the normal interval itself
    assert three_moment_intervals(mean, sd ** 2, -0.3)[:2] == below[:2]
    assert three_moment_intervals(mean, 0.0, np.nan) == (mean, mean, 0)
    lo, _hi, clipped = three_moment_intervals(1.0, 4.0, 0.5)  # a wide, weakly skewed fit reaches below 0: clipped
    assert lo == 0.0 and clipped == 1


# ------------------------------------------------------------------------------------------------ 3. Monte Carlo
@pytest.mark.parametrize("sd, ell, nobs, flowsd", [(0.8, 15, 12, 1.5), (1.0, 10, 12, 2.0)])
def test_storm_dominated_records_by_monte_carlo(sd, ell, nobs, flowsd):
    """A year whose load a few high-flow days carry: the exact skewness within 5 % of that of 200 000 joint draws, and both
    ends of the three-moment interval nearer to the draws' 2.5 % / 97.5 % quantiles than the two-moment lognormal's."""
    mu, cov, w = storm_record(sd, ell, nobs, flowsd, seed=2024)
    g = np.zeros(len(mu), np.int64)
    mean, pcov = dense_period_moments(cov, mu, 1.0, w, g, 1, backend.MODE_LOG)
    mean, var = mean.numpy(), np.diagonal(pcov.numpy())
    skew = dense_third_moments(cov, mu, 1.0, w, g, 1).numpy() / var ** 1.5
    sums = np.concatenate([np.exp(f) @ w for f in gaussian_draws(mu, cov, NDRAW, seed=7)])
    d = sums - sums.mean()
    mc_skew = np.mean(d ** 3) / np.mean(d ** 2) ** 1.5
    q_lo, q_hi = np.quantile(sums, [0.025, 0.975])
    lo2, hi2 = intervals(backend.MODE_LOG, mean, var)
    lo3, hi3 = intervals(backend.MODE_LOG, mean, var, interval="three-moment", skew=skew)
    fw_skew = (np.sqrt(var) / mean) ** 3 + 3 * np.sqrt(var) / mean
    r_lo, r_hi = abs(lo3[0] - q_lo) / abs(lo2[0] - q_lo), abs(hi3[0] - q_hi) / abs(hi2[0] - q_hi)
    print(f"sd {sd} ell {ell} nobs {nobs} flowsd {flowsd}: cv {np.sqrt(var[0]) / mean[0]:.3f} skew exact {skew[0]:.3f} MC {mc_skew:.3f} "
          f"FW {fw_skew[0]:.3f}; ends / mean: MC {q_lo / mean[0]:.3f} {q_hi / mean[0]:.3f}, lognormal {lo2[0] / mean[0]:.3f} "
          f"{hi2[0] / mean[0]:.3f}, three-moment {lo3[0] / mean[0]:.3f} {hi3[0] / mean[0]:.3f}; error ratios {r_lo:.2f} {r_hi:.2f}; "
          f"tails {np.mean(sums < lo3[0]):.4f} {np.mean(sums > hi3[0]):.4f} (lognormal {np.mean(sums < lo2[0]):.4f} {np.mean(sums > hi2[0]):.4f})")
    assert abs(sums.mean() / mean[0] - 1) < 5 * np.sqrt(var[0] / NDRAW) / mean[0]
    assert abs(skew[0] / mc_skew - 1) <= 0.05
    assert abs(lo3[0] - q_lo) < abs(lo2[0] - q_lo)
    assert abs(hi3[0] - q_hi) < abs(hi2[0] - q_hi)


# ------------------------------------------------------------------------------------------------ 4. the engine path
def _posterior(model, daily, pred_noise=False):
    model._ensure_factor()
    x = torch.tensor(model.dm.Xnew(daily), dtype=torch.float64)
    kmean, cov = model._plan.posterior_cov(model._factor_theta, x)
    mu = (kmean + model.model.prior_mean(x)).detach()
    extra = model.likelihood.predictive_noise(x.shape[0], x.device, torch.float64).detach() if pred_noise else None
    return mu, cov, extra


def _reference(model, daily, weights, freq, ci=0.95, pred_noise=False):
    mu, cov, extra = _posterior(model, daily, pred_noise)
    _mode, s, t = target_transform(model.dm)
    _o, groups, labels, _n, _d = period_groups(daily.coords["time"].values, weights, freq)
    mean, pcov = dense_period_moments(cov, s * mu + t, s * s, weights, groups, len(labels), backend.MODE_LOG, extra)
    k3 = dense_third_moments(cov, s * mu + t, s * s, weights, groups, len(labels), extra).numpy()
    var = np.diagonal(pcov.numpy())
    skew = k3 / var ** 1.5
    return skew, three_moment_intervals(mean.numpy(), var, skew, ci)


@pytest.fixture(scope="module")
def fitted():
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(MarginalHIP, "_plan_factory", staticmethod(SkewOraclePlan))
        mp.setattr(MarginalHIP, "device", "cpu")
        torch.manual_seed(0)
        cov_obs, target, daily = daily_loadest()
        model = LoadestGP()
        model.fit(cov_obs, target, iterations=10)
        yield model, daily


def test_annual_flux_and_aggregate_three_moment(fitted):
    model, daily = fitted
    before = SkewOraclePlan.third_calls
    plain = model.annual_flux(daily)
    assert SkewOraclePlan.third_calls == before  # the default makes no third-moment call
    assert "skewness" not in plain and "interval" not in plain.attrs and set(plain) == {"mean", "se", "lower", "upper", "n_points"}
    ds = model.annual_flux(daily, interval="three-moment")
    assert SkewOraclePlan.third_calls == before + 1
    again = model.annual_flux(daily, interval="lognormal")
    for key in ("mean", "se", "lower", "upper", "n_points"):  # the default is untouched, and the moments are the same
        assert np.array_equal(plain[key].values, again[key].values)
    assert np.array_equal(ds["mean"].values, plain["mean"].values) and np.array_equal(ds["se"].values, plain["se"].values)
    w = np.asarray(daily["flow"].values) * 86400 * 1e-3
    skew, (lo, hi, clipped) = _reference(model, daily, w, "YE")
    assert np.allclose(ds["skewness"].values, skew, rtol=1e-12, atol=0) and np.all(skew > 0)
    assert np.allclose(ds["lower"].values, lo, rtol=1e-12) and np.allclose(ds["upper"].values, hi, rtol=1e-12)
    assert ds.attrs["interval"] == "three-moment" and ds.attrs["clipped_lower"] == clipped == 0 and ds.attrs["freq"] == "YE"
    # the two-moment lognormal implies a smaller skewness, and its lower end lies below the three-moment one
    cv = plain["se"].values / plain["mean"].values
    assert np.all(skew > cv ** 3 + 3 * cv) and np.all(ds["lower"].values > plain["lower"].values)
    # aggregate: monthly sums with predictive noise, another ci
    dsm = model.aggregate(daily, w, freq="ME", ci=0.8, pred_noise=True, interval="three-moment")
    skew_m, (lo_m, hi_m, _c) = _reference(model, daily, w, "ME", ci=0.8, pred_noise=True)
    assert len(skew_m) == 36 and np.allclose(dsm["skewness"].values, skew_m, rtol=1e-12)
    assert np.allclose(dsm["lower"].values, lo_m, rtol=1e-12) and np.allclose(dsm["upper"].values, hi_m, rtol=1e-12)
    assert dsm["lower"].attrs["ci"] == 0.8
    for call in (lambda: model.annual_flux(daily, interval="normal"), lambda: model.aggregate(daily, w, interval=None),
                 lambda: annual_flux_many([model], [daily], interval="3"), lambda: intervals(1, [1.0], [1.0], interval="x")):
        with pytest.raises(ValueError, match="interval must be one of"):
            call()


def test_three_moment_refusals(fitted):
    model, daily = fitted
    n, m = model.dm.X.shape[0], len(daily.coords["time"].values)
    two, three = _site_bytes(n, m, 8), _site_bytes(n, m, 8) + _third_moment_bytes(m, 3)
    before = SkewOraclePlan.third_calls
    with pytest.raises(ValueError, match=f"needs {three} bytes"):  # fits the budget for two moments, not for three
        model.annual_flux(daily, interval="three-moment", max_bytes=three - 1)
    with pytest.raises(NotImplementedError, match="dense"):  # would take the streamed path
        model.annual_flux(daily, interval="three-moment", max_bytes=two - 1)
    with pytest.raises(ValueError, match=f"needs {three} bytes"):
        annual_flux_many([model], [daily], interval="three-moment", max_bytes=three - 1)
    with pytest.raises(NotImplementedError, match="dense"):
        annual_flux_many([model], [daily], interval="three-moment", max_bytes=two - 1)
    assert SkewOraclePlan.third_calls == before
    assert model.annual_flux(daily, interval="three-moment", max_bytes=three).attrs["interval"] == "three-moment"
    assert model.annual_flux(daily, max_bytes=two)["mean"].values.shape == (3,)  # the default's budget is what it was


def test_annual_flux_many_three_moment(fitted):
    model, daily = fitted
    cov_obs, target, daily2 = daily_loadest(n_obs=45, start="2011-06-01", end="2013-03-01", seed=4)
    other = LoadestGP()
    other.fit(cov_obs, target, iterations=5)
    models, dailies = [model, other], [daily, daily2]
    singles = [mdl.annual_flux(d, freq="YE-SEP", interval="three-moment") for mdl, d in zip(models, dailies)]
    # (the oracle-backed plan is single-site: a budget that just holds the larger site's footprint gives batches of one)
    two = max(_site_bytes(mdl.dm.X.shape[0], len(d.coords["time"].values), 8) for mdl, d in zip(models, dailies))
    before = SkewOraclePlan.third_calls
    plain = annual_flux_many(models, dailies, freq="YE-SEP", max_bytes=two)
    assert SkewOraclePlan.third_calls == before and "skewness" not in plain[0] and "interval" not in plain[0].attrs
    P_all = max(len(ds["mean"].values) for ds in singles)
    budget = max(_site_bytes(mdl.dm.X.shape[0], len(d.coords["time"].values), 8) + _third_moment_bytes(len(d.coords["time"].values), P_all)
                 for mdl, d in zip(models, dailies))
    many = annual_flux_many(models, dailies, freq="YE-SEP", interval="three-moment", max_bytes=budget)
    assert SkewOraclePlan.third_calls == before + 2
    for one, ds in zip(singles, many):
        assert np.array_equal(one.coords["time"].values, ds.coords["time"].values)
        for key in ("mean", "se", "skewness", "lower", "upper"):
            assert np.allclose(one[key].values, ds[key].values, rtol=1e-9, atol=0), key
        assert ds.attrs["interval"] == "three-moment" and ds.attrs["clipped_lower"] == 0
    for old, ds in zip(plain, many):  # the same moments, and the default's interval is the two-moment one
        assert np.array_equal(old["mean"].values, ds["mean"].values) and np.array_equal(old["se"].values, ds["se"].values)
        assert np.array_equal(old["lower"].values, intervals(backend.MODE_LOG, old["mean"].values, old["se"].values ** 2)[0])


def test_linear_targets_and_hyperparameter_totals():
    cov_obs, target, daily = daily_loadest(seed=3)
    model = LoadestGP(model_config=ModelConfig(transform="standard"))
    model.fit(cov_obs, target, iterations=5)
    before = SkewOraclePlan.third_calls
    plain, ds = model.annual_flux(daily), model.annual_flux(daily, interval="three-moment")
    assert SkewOraclePlan.third_calls == before  # Gaussian: nothing to compute
    assert np.all(ds["skewness"].values == 0.0) and ds.attrs["interval"] == "three-moment" and ds.attrs["clipped_lower"] == 0
    assert np.array_equal(ds["lower"].values, plain["lower"].values) and np.array_equal(ds["upper"].values, plain["upper"].values)
    # hyperparameters=True: lower / upper three-moment, lower_total / upper_total as they are
    mean, cov, covh = np.array([10.0, 20.0]), np.diag([4.0, 9.0]), np.diag([1.0, 2.0])
    labels = np.array(["2012-12-31", "2013-12-31"], dtype="datetime64[ns]")
    k3 = np.array([6.0, 30.0])
    two = loads._dataset(backend.MODE_LOG, mean, cov, labels, [366, 365], {}, 0.95, "YE", covh)
    three = loads._dataset(backend.MODE_LOG, mean, cov, labels, [366, 365], {}, 0.95, "YE", covh, interval="three-moment", k3=k3)
    for key in ("lower_total", "upper_total", "se_hyper", "se_total", "mean", "se"):
        assert np.array_equal(two[key].values, three[key].values)
    assert np.allclose(three["skewness"].values, k3 / np.array([8.0, 27.0]))
    assert not np.array_equal(two["lower"].values, three["lower"].values)


# ------------------------------------------------------------------------------------------------ 5. the ABI without a device
def test_third_moments_abi_without_a_device():
    """Every entry point that include/dgp_hip.h declares -- these two among them -- is bound through ``_lib.SIGNATURES`` and
    exported, and the table binds nothing else; sizes and every refusal with null device addresses: each call is refused before
    a launch."""
    import os
    import re

    lib = _lib.load()
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "dgp_hip.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(dgp_[a-z_0-9]+)\s*\(", header))
    assert names == set(_lib.SIGNATURES) and "dgp_period_third_moments" in names
    assert all(hasattr(lib, name) for name in names)
    size = lib.dgp_period_third_moments_workspace_bytes
    need = size(1000, 3, 2)
    M = lib.dgp_padded_n(1000)
    assert need == 2 * _third_moment_bytes(1000, 3) and need >= 2 * 8 * 2 * M * M
    assert need <= 2 * 8 * (2 * M * M + M * M // 128 + 8 * M + 1024)  # 2 M^2 + the (tile, row) partials + O(M + P) doubles
    assert size(1, 1, 1) == _third_moment_bytes(1, 1) and size(11323, 31, 1) == _third_moment_bytes(11323, 31)
    for bad in ((0, 3, 1), (-5, 3, 1), ((1 << 20) + 1, 3, 1), (10, 0, 1), (10, 65536, 1), (10, 3, 0), (10, 3, 1025)):
        assert size(*bad) == 0, bad
    p, work = C.c_void_p(16), C.c_void_p(4096)  # never dereferenced: every call below fails its host-side checks
    args = lambda **kw: [kw.get("dtype", 0), kw.get("cov", p), kw.get("m", 1000), kw.get("batch", 2), kw.get("mu", p),  # noqa: E731
                         kw.get("s2", p), kw.get("w", p), kw.get("g", p), kw.get("ng", 3), None, kw.get("tile", 0),
                         kw.get("work", work), kw.get("wb", need), kw.get("out", p), None]
    call = lib.dgp_period_third_moments
    assert call(*args(dtype=2)) == -1 and b"dgp_period_third_moments: dtype" in lib.dgp_last_error()
    for name in ("cov", "mu", "s2", "w", "g", "out"):
        assert call(*args(**{name: None})) == -1 and b"null" in lib.dgp_last_error(), name
    for kw in ({"m": 0}, {"m": (1 << 20) + 1}, {"ng": 0}, {"ng": 65536}, {"batch": 0}, {"batch": 1025}):
        assert call(*args(**kw)) == -1 and b"size" in lib.dgp_last_error(), kw
    for tile in (1, 32, 256, -64):
        assert call(*args(tile=tile)) == -1 and b"tile" in lib.dgp_last_error()
    assert call(*args(wb=need - 1)) == -3 and b"workspace" in lib.dgp_last_error()
    assert call(*args(work=None)) == -3 and b"workspace" in lib.dgp_last_error()
    assert call(*args(work=C.c_void_p(4096 + 128))) == -1 and b"256-byte aligned" in lib.dgp_last_error()
