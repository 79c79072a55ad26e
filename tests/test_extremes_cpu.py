"""Period extremes without a GPU: the numpy / scipy restatement of the orthant estimator (tests/extremes_helpers.orthant_ref)
against closed forms and joint draws, the host layer (generators, shifts, level chunking, the quantile search, the refusals)
and the argument checks of the two new C entries."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from scipy.special import ndtr

from discontinuum_amd import _lib
from discontinuum_amd import backend as B
from discontinuum_amd import extremes as X
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.rolling import time_windows as X_time_windows
from discontinuum_amd.xr_compat import Dataset
from tests.extremes_helpers import equicorrelated_factor, equicorrelated_truth, orthant_ref, smooth_cov
from tests.flux_helpers import daily_loadest
from tests.helpers import OraclePlan


# ------------------------------------------------------------------------------------------------ the restatement
def test_diagonal_factor_is_exact():
    """A diagonal L makes the integrand constant: the product of the marginals to 1e-13, reported error <= 1e-15."""
    m = 200
    sig = np.linspace(0.5, 2.0, m)
    prob, se = orthant_ref(np.diag(sig), -np.inf, 3.0, B.richtmyer_generators(m), B.orthant_shifts(m, 8, 0).numpy(), 256)
    assert abs(prob - np.prod(ndtr(3.0 / sig))) <= 1e-13 and se <= 1e-15


@pytest.mark.parametrize("m,rho,b", [(300, 0.5, 2.5), (130, 0.9, 1.0)])
def test_equicorrelated_blocks_against_quadrature(m, rho, b):
    """8 shifts x 2048 points, seed 0: within 4 reported errors of the one-dimensional quadrature AND the reported error at most
    3e-3 (a useless estimator with wide error bars must not pass).  Measured: m = 300: 0.731856 +- 6.7e-4 against 0.731687;
    m = 130: 0.573489 +- 6.1e-4 against 0.573750."""
    truth = equicorrelated_truth(m, rho, b)
    assert abs(truth - {300: 0.73169, 130: 0.57375}[m]) < 1e-5
    prob, se = orthant_ref(equicorrelated_factor(m, rho), -np.inf, b, B.richtmyer_generators(m), B.orthant_shifts(m, 8, 0).numpy(), 2048)
    print(f"m = {m}: {prob:.6f} +- {se:.1e}, truth {truth:.6f}")
    assert abs(prob - truth) <= 4 * se and se <= 3e-3


def test_lower_limits_against_joint_draws():
    """``kind="min"``: P(f_i >= -1 for all i) on a 365-point smooth covariance (tests/extremes_helpers.smooth_cov) with 16 shifts
    x 2048 points, seed 0, against 4e5 joint normal draws: |difference| <= 4 sqrt(err^2 + p (1 - p) / n_draws).
    Measured: 0.15030 +- 0.00151 against 0.15076 +- 0.00057 from the draws: 0.28 combined standard errors apart."""
    m, n_draws = 365, 400_000
    Lc = np.linalg.cholesky(smooth_cov(m))
    prob, se = orthant_ref(Lc, -1.0, np.inf, B.richtmyer_generators(m), B.orthant_shifts(m, 16, 0).numpy(), 2048)
    rng = np.random.default_rng(0)
    count = 0
    for _ in range(8):
        count += int(np.sum((rng.standard_normal((n_draws // 8, m)) @ Lc.T).min(axis=1) >= -1.0))
    p = count / n_draws
    comb = np.sqrt(se ** 2 + p * (1 - p) / n_draws)
    print(f"{prob:.5f} +- {se:.5f} against {p:.5f} from draws: {abs(prob - p) / comb:.2f} combined standard errors")
    assert abs(prob - p) <= 4 * comb


def test_limits_cases_of_the_restatement():
    """An unconstrained level is exactly 1 with error 0; an impossible one exactly 0; nothing non-finite."""
    m = 40
    Lc = np.linalg.cholesky(smooth_cov(m, ell=5.0, noise=0.3))
    gen, sh = B.richtmyer_generators(m), B.orthant_shifts(m, 4, 1).numpy()
    assert orthant_ref(Lc, -np.inf, np.inf, gen, sh, 64) == (1.0, 0.0)
    lo = np.full(m, -np.inf)
    lo[7] = 1.0
    hi = np.full(m, np.inf)
    hi[7] = -1.0
    assert orthant_ref(Lc, lo, hi, gen, sh, 64) == (0.0, 0.0)
    assert orthant_ref(Lc, 40.0, np.inf, gen, sh, 64) == (0.0, 0.0)
    # both limits far in the upper tail: the flipped branch keeps full relative accuracy
    p1, _ = orthant_ref(np.eye(1), 8.0, 9.0, gen, sh, 16)
    assert abs(p1 - (ndtr(-8.0) - ndtr(-9.0))) <= 1e-15 * ndtr(-8.0)


# ------------------------------------------------------------------------------------------------ host logic
def test_richtmyer_generators_against_a_hand_list():
    primes = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71]
    g = B.richtmyer_generators(20)
    assert np.array_equal(g, np.sqrt(np.array(primes, dtype=np.float64)) % 1.0) and np.all((g > 0) & (g < 1))
    big = B.richtmyer_generators(9000)
    assert big.shape == (9000,) and np.array_equal(big[:20], g)
    assert abs(big[-1] - np.sqrt(93179.0) % 1.0) == 0  # the 9000th prime
    with pytest.raises(ValueError):
        B.richtmyer_generators(0)


def test_level_chunks_and_shifts():
    """Chunking under ``max_bytes``: the most levels that fit, 64 at most, a ``ValueError`` naming the bytes when one level does
    not fit; the shifts are a function of (m, nshifts, seed) alone, so no chunking can change which shifts a level gets."""
    m, S, N = 366, 16, 4096
    lib = _lib.load()
    one = int(lib.dgp_orthant_probability_workspace_bytes(m, 1, S, N))
    assert one == 8 * (N // 128) * S * (384 * 128 + 1)
    assert int(lib.dgp_orthant_probability_workspace_bytes(m, 5, S, N)) == 5 * one
    assert B.orthant_level_chunks(m, 16, S, N, max_bytes=16 * one) == (16, one)
    assert B.orthant_level_chunks(m, 16, S, N, max_bytes=16 * one - 1) == (15, one)
    assert B.orthant_level_chunks(m, 16, S, N, max_bytes=one) == (1, one)
    assert B.orthant_level_chunks(m, 100, S, N, max_bytes=1 << 50) == (64, one)
    with pytest.raises(ValueError, match=f"{one} bytes for ONE level"):
        B.orthant_level_chunks(m, 16, S, N, max_bytes=one - 1)
    with pytest.raises(ValueError, match="bad size"):
        B.orthant_level_chunks(m, 16, 1, N)
    a, b = B.orthant_shifts(m, S, 3), B.orthant_shifts(m, S, 3)
    assert a.shape == (S, m) and a.dtype == torch.float64 and torch.equal(a, b) and bool(((a >= 0) & (a < 1)).all())
    assert not torch.equal(a, B.orthant_shifts(m, S, 4))


def test_quantile_search_on_a_known_distribution():
    """The bracketing search with a synthetic monotone distribution function in place of the device call: the known quantiles
    lie in the reported bracket, the value within its width, the bracket shrinks by (grid - 1) per round."""
    from scipy.special import ndtri

    loc, scale = np.array([0.3, -2.0, 5.0]), np.array([1.0, 0.2, 3.0])
    q = np.array([0.1, 0.5, 0.9])
    calls = []

    def cdf(t):
        calls.append(t.shape)
        return ndtr((t - loc[:, None, None]) / scale[:, None, None]), np.full(t.shape, 1e-3)

    lo, hi = loc - 6 * scale, loc + 7 * scale
    res = X.quantile_search(cdf, lo, hi, q, grid=16, rounds=3)
    truth = loc[:, None] + scale[:, None] * ndtri(q)[None, :]
    assert calls == [(3, 3, 16)] * 3
    width = res["upper"] - res["lower"]
    assert np.allclose(width, ((hi - lo) / 15 ** 3)[:, None])
    assert np.all((res["lower"] <= truth) & (truth <= res["upper"])) and np.all(np.abs(res["value"] - truth) <= width)
    assert np.all(np.abs(res["value"] - truth) <= 0.05 * width)  # the interpolation is far better than the bracket
    assert np.all((res["f_lower"] <= q[None, :]) & (q[None, :] <= res["f_upper"])) and np.all(res["error"] == 1e-3)
    assert np.all(np.diff(res["value"], axis=1) > 0)
    # a noisy, locally non-monotone function cannot lose the bracket; a quantile outside the start bracket gives the nearer end
    rng = np.random.default_rng(0)
    noisy = lambda t: (ndtr((t - loc[:, None, None]) / scale[:, None, None]) + 1e-4 * rng.standard_normal(t.shape), np.zeros(t.shape))  # noqa: E731
    res = X.quantile_search(noisy, lo, hi, q, grid=8, rounds=2)
    assert np.all(np.abs(ndtr((res["value"] - loc[:, None]) / scale[:, None]) - q[None, :]) <= 2e-3)
    res = X.quantile_search(cdf, loc, hi, np.array([0.2]), grid=5, rounds=2)
    assert np.allclose(res["value"][:, 0], loc)
    with pytest.raises(ValueError):
        X.quantile_search(cdf, lo, hi, q, grid=2)


def test_quantile_brackets_hold_the_quantiles():
    """The elementary bounds bracket the quantiles of the extreme whatever the correlations: checked on draws."""
    m = 50
    Cm = smooth_cov(m, ell=8.0, noise=0.2)
    mu = np.linspace(-0.5, 0.5, m)
    f = mu + np.random.default_rng(2).standard_normal((20000, m)) @ np.linalg.cholesky(Cm).T
    q = np.array([0.05, 0.95])
    for kind, ext in (("max", f.max(axis=1)), ("min", f.min(axis=1))):
        lo, hi = X.quantile_brackets(mu, np.sqrt(np.diag(Cm)), q, kind)
        assert lo < np.quantile(ext, 0.05) and np.quantile(ext, 0.95) < hi


@pytest.fixture()
def cpu_model(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(OraclePlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)
    cov_obs, target, daily = daily_loadest(n_obs=40, end="2013-01-01", seed=3)
    model = LoadestGP()
    model.fit(cov_obs, target, iterations=1)
    return model, daily


def test_every_refusal_says_why(cpu_model):
    model, daily = cpu_model
    with pytest.raises(NotImplementedError, match="dense posterior covariance.*drop streamed=True"):
        model.extreme_probability(daily, threshold=1.0, streamed=True)
    with pytest.raises(NotImplementedError, match=r"need the dense m x m covariance: this record \(\d+ bytes dense, max_bytes = 1000\)"):
        model.extreme_probability(daily, threshold=1.0, max_bytes=1000)
    with pytest.raises(ValueError, match="pred_noise=True is not implemented for period extremes"):
        model.extreme_probability(daily, threshold=1.0, pred_noise=True)
    with pytest.raises(NotImplementedError, match="kind='flux' is not implemented for period extremes"):
        model.extreme_probability(daily, threshold=1.0, kind="flux")
    with pytest.raises(ValueError, match="kind must be 'max' or 'min'"):
        model.extreme_probability(daily, threshold=1.0, kind="median")
    with pytest.raises(NotImplementedError, match="arithmetic rolling mean of a log target"):
        model.extreme_probability(daily, threshold=1.0, window="7D", statistic="mean")
    with pytest.raises(ValueError, match="exactly one of threshold and threshold_series"):
        model.extreme_probability(daily)
    for kw in (dict(streamed=True), dict(pred_noise=True), dict(kind="flux"), dict(window="7D", statistic="mean"), dict(max_bytes=1000)):
        with pytest.raises((NotImplementedError, ValueError)):
            model.extreme_quantiles(daily, **kw)
    with pytest.raises(ValueError, match="strictly between 0 and 1"):
        model.extreme_quantiles(daily, q=(0.0, 0.5))
    # a period longer than the sweep's limit: 17 000 half-hours in one year
    t = (np.datetime64("2012-01-01T00:00") + np.arange(17000) * np.timedelta64(30, "m")).astype("datetime64[ns]")
    long = Dataset({"flow": ("time", np.full(17000, 10.0), {"units": "cubic meters per second"})}, coords={"time": t})
    with pytest.raises(ValueError, match=f"a period holds 17000 points, more than the orthant sweep's limit of {B.ORTHANT_MAX_DIM}"):
        model.extreme_probability(long, threshold=1.0)


def test_host_layer_end_to_end_against_joint_draws(monkeypatch):
    """``extreme_probability`` / ``extreme_quantiles`` with an oracle-backed plan in place of the device (the sweep answered by
    the restatement): periods, dropped points, the threshold map, the windowed path, ``kind="min"`` and the quantile search,
    each held against 40 000 joint draws of the oracle's own posterior -- within 4 combined standard errors."""
    from tests.extremes_helpers import make_oracle_plan
    from tests.flux_helpers import gaussian_draws

    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(make_oracle_plan()))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)
    cov_obs, target, daily = daily_loadest(n_obs=40, start="2012-10-01", end="2013-03-01", seed=3, step_days=2)
    model = LoadestGP()
    model.fit(cov_obs, target, iterations=3)
    time = daily.coords["time"].values.copy()
    time[[0, 30, len(time) - 1]] = np.datetime64("NaT")  # dropped points
    rec = Dataset({"flow": ("time", np.asarray(daily["flow"].values), {"units": "cubic meters per second"})}, coords={"time": time})
    kw = dict(npoints=256, nshifts=8, seed=1)
    vals = np.asarray(target.values)
    levels = np.quantile(vals, [0.6, 0.9])
    ds = model.extreme_probability(rec, threshold=levels, **kw)
    n_pts = list(ds["n_points"].values)
    assert ds["prob_never"].values.shape == (2, 2) and sum(n_pts) == len(time) - 3 and ds.attrs["exact"] is False
    # joint draws of the latent posterior at the kept points, mapped to data space
    keep = np.nonzero(~np.isnat(time))[0]
    xs = torch.tensor(model.dm.Xnew(rec), dtype=torch.float64)[keep]
    model._eval_ready(xs)
    kmean, cov = model._plan.posterior_cov(model._factor_theta, xs)
    mu = (kmean + model.model.prior_mean(xs)).detach().numpy()
    Cm = cov.detach().numpy()
    Cm = np.tril(Cm) + np.tril(Cm, -1).T
    draws = np.concatenate(list(gaussian_draws(mu, Cm, 40000, seed=5)))
    _mode, s, t = X.target_transform(model.dm)
    conc = np.exp(s * draws + t)
    year = time[keep].astype("datetime64[Y]").astype(int)
    nd = draws.shape[0]
    for g, y in enumerate(np.unique(year)):
        peak, low = conc[:, year == y].max(axis=1), conc[:, year == y].min(axis=1)
        for l, tau in enumerate(levels):
            p = np.mean(peak <= tau)
            got, err = ds["prob_never"].values[l, g], ds["error"].values[l, g]
            assert abs(got - p) <= 4 * np.sqrt(err ** 2 + p * (1 - p) / nd) + 1e-4, (g, l, got, p, err)
        dmin = model.extreme_probability(rec, threshold=np.quantile(vals, 0.2), kind="min", **kw)
        p = np.mean(low >= np.quantile(vals, 0.2))
        got, err = dmin["prob_never"].values[0, g], dmin["error"].values[0, g]
        assert abs(got - p) <= 4 * np.sqrt(err ** 2 + p * (1 - p) / nd) + 1e-4
    dq = model.extreme_quantiles(rec, q=(0.1, 0.5, 0.9), **kw)
    dl = model.extreme_quantiles(rec, q=(0.1, 0.5, 0.9), kind="min", **kw)
    for g, y in enumerate(np.unique(year)):
        peak, low = conc[:, year == y].max(axis=1), conc[:, year == y].min(axis=1)
        for k, q in enumerate((0.1, 0.5, 0.9)):
            for dsq, ext in ((dq, peak), (dl, low)):
                v, e, mass = dsq["value"].values[k, g], dsq["error"].values[k, g], dsq["bracket_prob"].values[k, g]
                assert abs(np.mean(ext <= v) - q) <= 4 * np.sqrt(e ** 2 + q * (1 - q) / nd) + mass + 1e-4, (g, k, v)
        assert np.all(np.diff(dq["value"].values[:, g]) > 0) and np.all(dq["value"].values[:, g] > dl["value"].values[:, g])
    # a window: the extreme of the rolling geometric mean over 3 points (6 days at a 2-day step), against the same draws
    dw = model.extreme_probability(rec, threshold=levels[0], window="6D", kind="max", **kw)
    order, lo, hi, keepw = X_time_windows(time, "6D")
    assert np.array_equal(order, keep)
    cs = np.concatenate([np.zeros((nd, 1)), np.cumsum(draws, axis=1)], axis=1)
    roll = np.exp(s * ((cs[:, hi] - cs[:, lo]) / (hi - lo)) + t)
    for g, y in enumerate(np.unique(year)):
        sel = keepw & (year == y)
        assert dw["n_points"].values[g] == sel.sum()
        p = np.mean(roll[:, sel].max(axis=1) <= levels[0])
        got, err = dw["prob_never"].values[0, g], dw["error"].values[0, g]
        assert abs(got - p) <= 4 * np.sqrt(err ** 2 + p * (1 - p) / nd) + 1e-4, (g, got, p, err)


# ------------------------------------------------------------------------------------------------ the C entries, no device
def test_abi_is_declared_bound_and_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    names = {"dgp_orthant_probability", "dgp_orthant_probability_workspace_bytes"}
    assert names <= set(_lib.EXT2_SIGNATURES) and not names & set(_lib.SIGNATURES) and not names & set(_lib.EXT_SIGNATURES)
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    ext2 = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "dgp_hip_ext2.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(dgp_[a-z_0-9]+)\s*\(", ext2))
    for name in names:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.EXT2_SIGNATURES[name][1] and fn.restype == _lib.EXT2_SIGNATURES[name][0]
    wq, op = lib.dgp_orthant_probability_workspace_bytes, lib.dgp_orthant_probability
    assert wq(1, 1, 2, 1) == 8 * 2 * (64 * 128 + 1) and wq(8832, 64, 64, 4096) > 0 and wq(16384, 1, 2, 1 << 20) > 0
    for bad in ((0, 1, 2, 100), (100, 1, 1, 100), (100, 65, 2, 100), (100, 0, 2, 100), (16385, 1, 2, 100), (100, 1, 65, 100),
                (100, 1, 2, 0), (100, 1, 2, (1 << 20) + 1)):
        assert wq(*bad) == 0, bad
    one = C.c_void_p(256)  # never dereferenced: every call below returns before any launch
    err = lib.dgp_last_error
    need = wq(300, 3, 4, 200)
    ok = [one, 300, 384, one, one, 3, one, one, 4, 200, one, need, one, one, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return op(*a)

    for i in (0, 3, 4, 6, 7, 12, 13):  # L, lo, hi, gen, shift, prob, se
        assert call(**{f"a{i}": None}) == _lib.E_ARG and b"null" in err(), i
    for kw in (dict(a1=0), dict(a1=16385), dict(a5=0), dict(a5=65), dict(a8=1), dict(a8=65), dict(a9=0)):
        assert call(**kw) == _lib.E_ARG and b"size" in err(), kw
    assert call(a2=383) == _lib.E_ARG and call(a2=300) == _lib.E_ARG and b"ld" in err()
    assert call(a2=385) == _lib.E_ARG and call(a0=C.c_void_p(264)) == _lib.E_ARG  # odd ld; a factor that is not 16-byte aligned
    assert call(a10=None) == _lib.E_WORKSPACE and call(a11=need - 1) == _lib.E_WORKSPACE and b"workspace" in err()
    assert call(a10=C.c_void_p(264)) == _lib.E_ARG and b"aligned" in err()
