"""Exceedance-count distributions without a GPU: the numpy / scipy restatement of the estimator (tests/count_helpers.counts_ref)
against closed forms, the host layer (``frequency``: statistics per shift, links, compliance, the refusals) over an oracle
plan whose ``path_counts`` is that restatement, level chunking, and the argument checks of the two new C entries."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from scipy.special import ndtr, ndtri

from discontinuum_amd import _lib
from discontinuum_amd import backend as B
from discontinuum_amd import frequency as F
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.xr_compat import Dataset
from tests.count_helpers import (binomial_pmf, counts_ref, equicorrelated_count_pmf, longest_run_cdf, make_count_oracle_plan,
                                 paths_ref)
from tests.extremes_helpers import equicorrelated_factor, smooth_cov
from tests.flux_helpers import daily_loadest
from tests.helpers import OraclePlan


def _stats(hist, npoints):
    return F.histogram_statistics(hist, hist.shape[1] - 1, npoints)


# ------------------------------------------------------------------------------------------------ the restatement against truth
def test_diagonal_factor_is_binomial_and_runs_follow_the_dp():
    """A diagonal L with thresholds at the same standardised level: N is binomial(m, p), the longest run that of m independent
    trials.  Every value of both distribution functions within 5 reported errors plus the rule's resolution 1 / (npoints x
    nshifts): an event rarer than that (N = 12 has probability 0.3^12 = 5e-7) is seen by no path, and its estimate 0 comes with
    an error of 0.  So that a huge error bar cannot pass, each reported error is at most 3 times the plain Monte-Carlo error of
    the same number of paths (plus 1e-12 for the exact ends)."""
    m, S, N, p = 12, 16, 4096, 0.3
    sig = np.linspace(0.5, 2.0, m)
    thr = (sig * -ndtri(p))[None, :]  # P(f_i > thr_i) = p
    ch, sh, gap = counts_ref(np.diag(sig), thr, True, None, B.richtmyer_generators(m), B.orthant_shifts(m, S, 0).numpy(), N)
    assert gap > 0 and np.all(ch.sum(axis=2) == N) and np.all(sh.sum(axis=2) == N)
    for hist, truth in ((ch[0], np.cumsum(binomial_pmf(m, p))), (sh[0], longest_run_cdf(m, p))):
        st = _stats(hist, N)
        z = np.abs(st["cdf"][:-1] - truth[:-1]) / np.maximum(st["cdf_error"][:-1], 1e-300)
        print("worst:", z.max(), "largest error:", st["cdf_error"].max())
        assert np.all(np.abs(st["cdf"][:-1] - truth[:-1]) <= 5 * st["cdf_error"][:-1] + 1.0 / (N * S))
        assert np.all(st["cdf_error"] <= 3 * np.sqrt(truth * (1 - truth) / (N * S)) + 1e-12)
        assert st["cdf"][-1] == 1.0 and abs(truth[-1] - 1.0) < 1e-12


def test_equicorrelated_block_against_quadrature():
    """m = 64, rho = 0.5, b = 0.8, 16 shifts x 4096 points, seed 0, against the one-dimensional quadrature of the pmf: every
    value of the distribution function with k < m within 5 standard errors, and ``mean_error`` <= 3 sqrt(Var N / (npoints x
    nshifts)) with Var N from the closed form.  Measured: worst 2.19 standard errors, largest standard error 1.3e-3, mean
    13.569 +- 0.010 against 13.559."""
    m, rho, b, S, N = 64, 0.5, 0.8, 16, 4096
    pmf = equicorrelated_count_pmf(m, rho, b)
    assert abs(pmf.sum() - 1.0) < 1e-12
    k = np.arange(m + 1)
    mean_t = float(pmf @ k)
    var_t = float(pmf @ (k - mean_t) ** 2)
    assert abs(mean_t - m * ndtr(-b)) < 1e-9  # the mean is m P(f_i > b) whatever the correlation
    ch, _sh, gap = counts_ref(equicorrelated_factor(m, rho), np.full((1, m), b), True, None, B.richtmyer_generators(m),
                              B.orthant_shifts(m, S, 0).numpy(), N)
    st = _stats(ch[0], N)
    truth = np.cumsum(pmf)
    z = np.abs(st["cdf"][:m] - truth[:m]) / st["cdf_error"][:m]
    print(f"worst {z.max():.2f} standard errors, largest standard error {st['cdf_error'].max():.2e}, "
          f"mean {st['mean']:.3f} +- {st['mean_error']:.3f} against {mean_t:.3f}; variance {st['variance']:.2f} against {var_t:.2f}")
    assert gap > 0 and np.all(np.abs(st["cdf"][:m] - truth[:m]) <= 5 * st["cdf_error"][:m])
    assert st["mean_error"] <= 3 * np.sqrt(var_t / (N * S))
    assert abs(st["mean"] - mean_t) <= 5 * st["mean_error"] and abs(st["variance"] - var_t) <= 5 * st["variance_error"]


def test_restatement_rules():
    """A NaN threshold never counts, on either side; +-inf thresholds count always / never; ``above=False`` mirrors
    ``above=True`` when no path ties; a ``link`` break shortens spells and leaves the counts alone; ``link[0]`` is ignored."""
    m, S, N = 40, 4, 128
    Lc = np.linalg.cholesky(smooth_cov(m, ell=5.0, noise=0.3))
    gen, sh = B.richtmyer_generators(m), B.orthant_shifts(m, S, 1).numpy()
    sd = np.sqrt(np.diag(Lc @ Lc.T))
    thr = np.stack([0.3 * sd, np.full(m, np.nan), np.full(m, -np.inf), np.full(m, np.inf)])
    up, up_run, gap = counts_ref(Lc, thr, True, None, gen, sh, N)
    dn, dn_run, _ = counts_ref(Lc, thr, False, None, gen, sh, N)
    assert gap > 0 and np.all(up.sum(axis=2) == N) and np.all(dn_run.sum(axis=2) == N)
    assert np.array_equal(dn[0], up[0][:, ::-1])  # N_below = m - N_above
    for h in (up[1], dn[1], up_run[1], dn_run[1], up[3], dn[2]):
        assert np.all(h[:, 0] == N) and np.all(h[:, 1:] == 0)  # never
    for h in (up[2], up_run[2], dn[3], dn_run[3]):
        assert np.all(h[:, m] == N)  # always: N = R = m
    link = np.ones(m, dtype=np.int32)
    link[[0, 12, 28]] = 0
    cut, cut_run, _ = counts_ref(Lc, thr, True, link, gen, sh, N)
    assert np.array_equal(cut, up)
    assert np.all(cut_run[2][:, 16] == N)  # always exceeding: the pieces are 0 .. 11, 12 .. 27, 28 .. 39
    mean = lambda h: (h * np.arange(m + 1)).sum(axis=1)  # noqa: E731
    assert np.all(mean(cut_run[0]) <= mean(up_run[0])) and np.any(mean(cut_run[0]) < mean(up_run[0]))
    link[0] = 1
    assert np.array_equal(counts_ref(Lc, thr, True, link, gen, sh, N)[1], cut_run)
    # the paths themselves: f = L y with the weights' own draws, and w = 0 gives the clamp
    f = paths_ref(Lc, gen, sh, 8)
    assert f.shape == (S, 8, m) and np.all(np.isfinite(f))
    assert np.all(paths_ref(np.eye(1), np.array([0.5]), np.array([[0.0], [0.5]]), 1)[:, 0, 0] == [-38.0, 38.0])


def test_histogram_statistics_on_a_hand_example():
    hist = np.array([[2, 1, 1, 0], [0, 2, 2, 0]])  # two shifts of 4 points, counts 0 .. 3
    st = F.histogram_statistics(hist, 3, 4)
    assert np.allclose(st["pmf"], [0.25, 0.375, 0.375, 0.0]) and np.allclose(st["cdf"], [0.25, 0.625, 1.0, 1.0])
    assert np.allclose(st["cdf_error"], np.array([0.5, 0.25, 0.0, 0.0]) / np.sqrt(2) / np.sqrt(2))
    assert np.isclose(st["mean"], 1.125) and np.isclose(st["mean_error"], 0.75 / np.sqrt(2) / np.sqrt(2))
    k = np.arange(4)
    assert np.isclose(st["variance"], st["pmf"] @ (k - 1.125) ** 2)
    # a longer buffer than n_p + 1 is cut, as a period shorter than the longest is
    assert np.allclose(F.histogram_statistics(np.pad(hist, ((0, 0), (0, 3))), 3, 4)["cdf"], st["cdf"])


def test_links_follow_the_records_median_step():
    t = np.datetime64("2012-01-01") + np.array([0, 1, 2, 3, 9, 10, 11, 12, 13]) * np.timedelta64(1, "D")
    link, med = F.spell_links(t)
    assert med == np.timedelta64(1, "D").astype("timedelta64[ns]").astype(np.int64)
    assert list(link) == [0, 1, 1, 1, 0, 1, 1, 1, 1]
    assert list(F.spell_links(t[::2])[0]) == [0, 1, 0, 1, 1]  # days 0, 2, 9, 11, 13: median step 2


def test_level_chunks():
    """One work area serves 16 levels: the chunking counts in groups of 16, at most 64 levels per call."""
    m, S, N = 366, 16, 4096
    lib = _lib.load()
    one = int(lib.dgp_path_counts_workspace_bytes(m, 1, S, N))
    assert one == 8 * (N // 128) * S * 384 * 128
    assert int(lib.dgp_path_counts_workspace_bytes(m, 16, S, N)) == one and int(lib.dgp_path_counts_workspace_bytes(m, 17, S, N)) == 2 * one
    assert B.path_count_level_chunks(m, 40, S, N, max_bytes=one) == (16, one)
    assert B.path_count_level_chunks(m, 40, S, N, max_bytes=3 * one - 1) == (32, one)
    assert B.path_count_level_chunks(m, 5, S, N, max_bytes=one) == (5, one)
    assert B.path_count_level_chunks(m, 100, S, N, max_bytes=1 << 50) == (64, one)
    with pytest.raises(ValueError, match=f"{one} bytes for ONE level"):
        B.path_count_level_chunks(m, 16, S, N, max_bytes=one - 1)
    with pytest.raises(ValueError, match="bad size"):
        B.path_count_level_chunks(m, 16, 1, N)


# ------------------------------------------------------------------------------------------------ host logic over the oracle plan
KW = dict(npoints=512, nshifts=8, seed=1)


@pytest.fixture(scope="module")
def oracle_model():
    """A LoadestGP on the oracle plan and a two-year daily record with three dropped points and a ten-day gap in 2013."""
    mp = pytest.MonkeyPatch()
    plan_cls = make_count_oracle_plan()
    mp.setattr(MarginalHIP, "_plan_factory", staticmethod(plan_cls))
    mp.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)
    cov_obs, target, daily = daily_loadest(n_obs=40, start="2012-01-01", end="2014-01-01", seed=3)
    model = LoadestGP()
    model.fit(cov_obs, target, iterations=3)
    time = daily.coords["time"].values.copy()
    time[[0, 30, len(time) - 1]] = np.datetime64("NaT")
    time[500:510] = np.datetime64("NaT")
    rec = Dataset({"flow": ("time", np.asarray(daily["flow"].values), {"units": "cubic meters per second"})}, coords={"time": time})
    levels = np.quantile(np.asarray(target.values), [0.75, 0.97])
    yield model, rec, levels, plan_cls
    mp.undo()


def test_dataset_shapes_and_the_distribution_functions(oracle_model):
    model, rec, levels, plan_cls = oracle_model
    plan_cls.calls.clear()
    ds = model.exceedance_distribution(rec, threshold=levels, **KW)
    n_p = list(ds["n_points"].values)
    assert n_p == [364, 354] and list(ds.coords["count"].values) == list(range(365))
    assert ds.attrs["exact"] is False and ds.attrs["above"] is True and ds.attrs["npoints"] == 512 and ds.attrs["nshifts"] == 8
    assert ds.attrs["seed"] == 1 and ds.attrs["jitter"] >= 0.0 and ds.attrs["freq"] == "YE" and "window" not in ds.attrs
    for name in ("pmf", "cdf", "cdf_error", "spell_pmf", "spell_cdf", "spell_cdf_error"):
        v = ds[name].values
        assert v.shape == (2, 2, 365)
        assert np.all(np.isnan(v[:, 1, 355:])) and np.all(np.isfinite(v[:, 1, :355])) and np.all(np.isfinite(v[:, 0]))
    for name in ("mean", "mean_error", "variance", "variance_error"):
        assert ds[name].values.shape == (2, 2) and np.all(np.isfinite(ds[name].values))
    for name in ("cdf", "spell_cdf"):
        for g, n in enumerate(n_p):
            c = ds[name].values[:, g, :n + 1]
            assert np.all(np.diff(c, axis=1) >= 0) and np.all(c[:, -1] == 1.0) and np.all(c >= 0)
    assert np.allclose(np.nansum(ds["pmf"].values, axis=2), 1.0, atol=1e-12)
    # the calls: one per period, the histograms sum to npoints, the gap in the record breaks the runs of 2013 and nothing else
    assert [c["m"] for c in plan_cls.calls] == n_p and all(c["gap"] > 0 for c in plan_cls.calls)
    l0, l1 = plan_cls.calls[0]["link"], plan_cls.calls[1]["link"]
    assert l0[0] == 0 and np.all(l0[1:29] == 1) and l0[29] == 0  # day 30 is dropped: day 31 does not continue day 29
    assert np.count_nonzero(l0[1:] == 0) == 1 and np.count_nonzero(l1[1:] == 0) == 1  # day 30 dropped; days 500 .. 509 dropped
    assert np.nonzero(l1[1:] == 0)[0][0] + 1 == 500 - 366
    # a spell is never longer than the count, and P(R = 0) = P(N = 0)
    assert np.all(ds["spell_cdf"].values[:, :, 0] == ds["cdf"].values[:, :, 0])
    assert np.all(ds["spell_cdf"].values[:, 0, :] >= ds["cdf"].values[:, 0, :])


def test_below_mirrors_above_and_chunking_changes_nothing(oracle_model):
    model, rec, levels, plan_cls = oracle_model
    up = model.exceedance_distribution(rec, threshold=levels, **KW)
    plan_cls.calls.clear()
    dn = model.exceedance_distribution(rec, threshold=levels, above=False, **KW)
    assert all(c["gap"] > 0 and c["above"] is False for c in plan_cls.calls) and dn.attrs["above"] is False
    for g, n in enumerate(up["n_points"].values):
        assert np.array_equal(dn["pmf"].values[:, g, :n + 1], up["pmf"].values[:, g, :n + 1][:, ::-1])
    assert np.allclose(dn["mean"].values, up["n_points"].values[None, :] - up["mean"].values, rtol=0, atol=1e-9)
    # 40 levels under a budget of one work area: 16 per call, the same numbers
    many = np.quantile(levels, np.linspace(0, 1, 40))
    small = dict(npoints=128, nshifts=4, seed=2)
    whole = model.exceedance_distribution(rec, threshold=many, **small)
    one = B.path_count_level_chunks(364, 1, 4, 128)[1]
    plan_cls.calls.clear()
    periods_bytes = F.X._Periods(model, rec, "YE", None, "right", None, F.DEFAULT_MAX_BYTES).dense_bytes
    split = model.exceedance_distribution(rec, threshold=many, max_bytes=periods_bytes + one, **small)
    assert [c["per_call"] for c in plan_cls.calls] == [16, 16]
    for name in ("pmf", "spell_pmf", "cdf_error", "mean", "variance"):
        assert np.array_equal(split[name].values, whole[name].values, equal_nan=True)
    with pytest.raises(ValueError, match="bytes for ONE level"):
        model.exceedance_distribution(rec, threshold=many, max_bytes=periods_bytes + one - 1, **small)


def test_cross_checks_against_the_exact_products(oracle_model):
    """``compliance_probability(allowed=0)`` against ``extreme_probability``'s ``prob_never`` within 5 hypot of the two errors;
    ``mean`` against ``exceedance()``'s exact mean within 5 ``mean_error``; ``variance`` against its exact variance within 5
    standard errors of the per-shift variances."""
    model, rec, levels, _plan_cls = oracle_model
    ds = model.exceedance_distribution(rec, threshold=levels, **KW)
    comp = model.compliance_probability(rec, threshold=levels, allowed=0, max_spell=3, **KW)
    ext = model.extreme_probability(rec, threshold=levels, **KW)
    exact = model.exceedance(rec, threshold=levels)
    print("prob", comp["prob"].values, "+-", comp["error"].values, "never", ext["prob_never"].values, "+-", ext["error"].values)
    print("mean", ds["mean"].values, "+-", ds["mean_error"].values, "exact", exact["mean"].values)
    print("variance", ds["variance"].values, "+-", ds["variance_error"].values, "exact", exact["se"].values ** 2)
    assert np.array_equal(comp["prob"].values, ds["cdf"].values[:, :, 0]) and list(comp["allowed_count"].values) == [0, 0]
    assert np.array_equal(comp["prob_spell"].values, ds["spell_cdf"].values[:, :, 3])
    assert np.array_equal(comp["error_spell"].values, ds["spell_cdf_error"].values[:, :, 3])
    assert np.all(np.abs(comp["prob"].values - ext["prob_never"].values) <= 5 * np.hypot(comp["error"].values, ext["error"].values))
    assert np.all(np.abs(ds["mean"].values - exact["mean"].values) <= 5 * ds["mean_error"].values)
    assert np.all(np.abs(ds["variance"].values - exact["se"].values ** 2) <= 5 * ds["variance_error"].values)
    assert np.any((comp["prob"].values > 0.02) & (comp["prob"].values < 0.98))  # (a check between 0 and 0 would show nothing)


def test_compliance_rules_and_argument_checks(oracle_model):
    model, rec, levels, _plan_cls = oracle_model
    ds = model.exceedance_distribution(rec, threshold=levels, **KW)
    frac = model.compliance_probability(rec, threshold=levels, allowed_fraction=0.1, **KW)
    assert list(frac["allowed_count"].values) == [36, 35] and frac.attrs["allowed_fraction"] == 0.1 and "prob_spell" not in frac
    for g, k in enumerate((36, 35)):
        assert np.array_equal(frac["prob"].values[:, g], ds["cdf"].values[:, g, k])
        assert np.array_equal(frac["error"].values[:, g], ds["cdf_error"].values[:, g, k])
    full = model.compliance_probability(rec, threshold=levels, allowed=1000, max_spell=1000, **KW)  # beyond every period
    assert np.all(full["prob"].values == 1.0) and np.all(full["prob_spell"].values == 1.0) and np.all(full["error"].values == 0.0)
    assert list(F._allowed_counts([30, 365, 0], None, 0.1)) == [3, 36, 0]
    for kw in (dict(), dict(allowed=1, allowed_fraction=0.1)):
        with pytest.raises(ValueError, match="exactly one of allowed and allowed_fraction"):
            model.compliance_probability(rec, threshold=levels, **kw)
    for kw, text in ((dict(allowed=-1), "whole number"), (dict(allowed=1.5), "whole number"), (dict(allowed_fraction=1.2), r"\[0, 1\]"),
                     (dict(allowed=0, max_spell=-2), "max_spell")):
        with pytest.raises(ValueError, match=text):
            model.compliance_probability(rec, threshold=levels, **kw)


def test_window_and_threshold_series(oracle_model):
    """``window="7D"``: the counts of the rolling geometric mean -- the window attrs, fewer points (the leading partial windows
    and those over the gap are left out), runs broken where outputs are missing; a per-day threshold series works."""
    model, rec, levels, plan_cls = oracle_model
    plan_cls.calls.clear()
    dw = model.exceedance_distribution(rec, threshold=levels[0], window="7D", above=False, **KW)
    n_p = list(dw["n_points"].values)
    assert dw.attrs["window"] == "7D" and dw.attrs["align"] == "right" and dw.attrs["statistic"] == "geometric_mean"
    assert n_p[0] < 364 and n_p[1] < 354 and [c["m"] for c in plan_cls.calls] == n_p
    assert all(np.count_nonzero(c["link"][1:] == 0) >= 1 for c in plan_cls.calls)
    assert np.all(dw["cdf"].values[0, 1, n_p[1]] == 1.0) and np.all(np.isfinite(dw["mean"].values))
    exact = model.exceedance(rec, threshold=levels[0], window="7D", above=False)
    assert np.all(np.abs(dw["mean"].values - exact["mean"].values) <= 5 * dw["mean_error"].values)
    series = np.full(len(rec.coords["time"].values), levels[0])
    a = model.exceedance_distribution(rec, threshold_series=series, **KW)
    b = model.exceedance_distribution(rec, threshold=levels[0], **KW)
    assert np.array_equal(a["pmf"].values, b["pmf"].values, equal_nan=True)


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
    for call in (model.exceedance_distribution, lambda *a, **k: model.compliance_probability(*a, allowed=1, **k)):
        with pytest.raises(NotImplementedError, match="dense posterior covariance.*drop streamed=True"):
            call(daily, threshold=1.0, streamed=True)
        with pytest.raises(NotImplementedError, match=r"need the dense m x m covariance: this record \(\d+ bytes dense, max_bytes = 1000\)"):
            call(daily, threshold=1.0, max_bytes=1000)
        with pytest.raises(ValueError, match="pred_noise=True is not implemented for exceedance-count distributions"):
            call(daily, threshold=1.0, pred_noise=True)
        with pytest.raises(NotImplementedError, match="kind='flux' is not implemented for exceedance-count distributions"):
            call(daily, threshold=1.0, kind="flux")
        with pytest.raises(ValueError, match="kind must be None"):
            call(daily, threshold=1.0, kind="max")
        with pytest.raises(NotImplementedError, match="arithmetic rolling mean of a log target"):
            call(daily, threshold=1.0, window="7D", statistic="mean")
        with pytest.raises(ValueError, match="exactly one of threshold and threshold_series"):
            call(daily)
    assert F.REFUSALS["streamed"] is F.X.REFUSALS["streamed"]
    t = (np.datetime64("2012-01-01T00:00") + np.arange(17000) * np.timedelta64(30, "m")).astype("datetime64[ns]")
    long = Dataset({"flow": ("time", np.full(17000, 10.0), {"units": "cubic meters per second"})}, coords={"time": t})
    with pytest.raises(ValueError, match=f"a period holds 17000 points, more than the orthant sweep's limit of {B.ORTHANT_MAX_DIM}"):
        model.exceedance_distribution(long, threshold=1.0)


# ------------------------------------------------------------------------------------------------ the C entries, no device
def test_abi_is_declared_bound_and_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    names = {"dgp_path_counts", "dgp_path_counts_workspace_bytes"}
    assert names <= set(_lib.EXT2_SIGNATURES)
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    ext2 = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "dgp_hip_ext2.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(dgp_[a-z_0-9]+)\s*\(", ext2))
    wq, op = lib.dgp_path_counts_workspace_bytes, lib.dgp_path_counts
    assert wq(1, 1, 2, 1) == 8 * 2 * 128 * 128 and wq(8832, 64, 64, 4096) > 0 and wq(16384, 1, 2, 1 << 20) > 0
    for bad in ((0, 1, 2, 100), (100, 1, 1, 100), (100, 65, 2, 100), (100, 0, 2, 100), (16385, 1, 2, 100), (100, 1, 65, 100),
                (100, 1, 2, 0), (100, 1, 2, (1 << 20) + 1)):
        assert wq(*bad) == 0, bad
    one = C.c_void_p(256)  # never dereferenced: every call below returns before any launch
    err = lib.dgp_last_error
    need = wq(300, 3, 4, 200)
    #     L    m    ld   thr  nlev above link gen  shift S  N    work  bytes count spell stream
    ok = [one, 300, 384, one, 3, 1, None, one, one, 4, 200, one, need, one, one, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return op(*a)

    for i in (0, 3, 7, 8, 13, 14):  # L, thr, gen, shift, count_hist, spell_hist (a null link is allowed)
        assert call(**{f"a{i}": None}) == _lib.E_ARG and b"null" in err(), i
    for kw in (dict(a1=0), dict(a1=16385), dict(a4=0), dict(a4=65), dict(a9=1), dict(a9=65), dict(a10=0), dict(a10=(1 << 20) + 1)):
        assert call(**kw) == _lib.E_ARG and b"size" in err(), kw
    assert call(a2=383) == _lib.E_ARG and call(a2=300) == _lib.E_ARG and b"ld" in err()
    assert call(a2=385) == _lib.E_ARG and call(a0=C.c_void_p(264)) == _lib.E_ARG  # odd ld; a factor that is not 16-byte aligned
    assert call(a11=None) == _lib.E_WORKSPACE and call(a12=need - 1) == _lib.E_WORKSPACE and b"workspace" in err()
    assert call(a11=C.c_void_p(264)) == _lib.E_ARG and b"aligned" in err()
