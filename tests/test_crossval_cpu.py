"""Exact cross-validation (``MarginalHIP.cross_validate``, ``LoadestGP.flux_bias``, ``validation.cv_folds``) on CPU: the
host logic -- fold schemes, sorting by fold, transforms, summary statistics -- with the device plan replaced by an
oracle-backed double that cross-validates by dense DELETION, against a reference built in the test from the engine's own
state through ``orc.posterior``; and the new C entries' argument checks without a device."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch
from scipy.stats import norm

from discontinuum_amd import _lib
from discontinuum_amd.backend import cross_validate_folds
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.loads import target_transform
from discontinuum_amd.rating_gp import RatingGP
from discontinuum_amd.validation import cross_validate, cv_folds, flux_bias
from tests.crossval_helpers import CVOraclePlan, posterior_deletion_reference
from tests.helpers import loadest_dataset, rating_dataset


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(CVOraclePlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)


# a record that spans a water-year boundary (Oct 1) and has an empty calendar year (2013), not in time order
TIME = np.array(["2012-09-29", "2011-03-01", "2012-10-02", "2014-01-05", "2011-11-30", "2012-09-30", "2014-06-01", "2011-03-02",
                 "2014-12-31", "2012-01-01"], dtype="datetime64[ns]")


def _is_partition(groups, nfolds):
    return groups.min() == 0 and sorted(set(groups)) == list(range(nfolds))


def test_cv_folds_schemes():
    n = len(TIME)
    g, lab = cv_folds(TIME, "loo")
    assert list(g) == list(range(n)) and np.array_equal(lab, TIME)
    g, lab = cv_folds(TIME, "YE")  # 2011, 2012, 2014: the empty 2013 is no fold
    assert list(pd.DatetimeIndex(lab).strftime("%Y-%m-%d")) == ["2011-12-31", "2012-12-31", "2014-12-31"]
    assert list(g) == [{2011: 0, 2012: 1, 2014: 2}[y] for y in pd.DatetimeIndex(TIME).year] and _is_partition(g, 3)
    g, lab = cv_folds(TIME, "YE-SEP")  # water years end Sep 30: 2011, 2012, 2013 (Oct 2012), 2014, 2015 (Dec 2014)
    assert list(pd.DatetimeIndex(lab).strftime("%Y-%m-%d")) == ["2011-09-30", "2012-09-30", "2013-09-30", "2014-09-30", "2015-09-30"]
    wy = pd.DatetimeIndex(TIME).year + (pd.DatetimeIndex(TIME).month >= 10)
    assert list(g) == [int(y) - 2011 for y in wy] and _is_partition(g, 5)
    for alias, nf in (("QE", 8), ("ME", 8)):
        g, lab = cv_folds(TIME, alias)
        assert len(lab) == nf and _is_partition(g, nf)
        per = pd.DatetimeIndex(TIME).to_period(alias[0])
        assert all((per[i] == per[j]) == (g[i] == g[j]) for i in range(n) for j in range(n))
        assert np.all(np.diff(lab.astype("int64")) > 0)
    g, lab = cv_folds(TIME, 3)  # contiguous blocks in time order, sizes 4, 3, 3
    assert list(lab) == [0, 1, 2] and _is_partition(g, 3)
    assert list(g[np.argsort(TIME)]) == [0, 0, 0, 0, 1, 1, 1, 2, 2, 2]
    g7, _ = cv_folds(TIME, 7)
    assert sorted(np.bincount(g7)) == [1, 1, 1, 1, 2, 2, 2] and np.all(np.diff(g7[np.argsort(TIME)]) >= 0)
    ga, lab = cv_folds(TIME, ("random", 4, 11))
    gb, _ = cv_folds(TIME, ("random", 4, 11))
    gc, _ = cv_folds(TIME, ("random", 4, 12))
    assert np.array_equal(ga, gb) and not np.array_equal(ga, gc) and _is_partition(ga, 4) and list(lab) == [0, 1, 2, 3]
    assert sorted(np.bincount(ga)) == [2, 2, 3, 3]
    explicit = np.array([3, 0, 0, -1, 1, 1, 3, 0, -1, 1])
    g, lab = cv_folds(TIME, explicit)
    assert np.array_equal(g, explicit) and list(lab) == [0, 1, 2, 3]
    for bad in ("nonsense", 0, n + 1, ("random", 0, 1), np.zeros(3, dtype=int), np.full(n, -1), np.full(n, -2), np.ones(n)):
        with pytest.raises((ValueError, TypeError)):
            cv_folds(TIME, bad)


def test_fold_sorting_for_the_device():
    class Plan:
        batch, n, _site_sizes = 1, 7, [7]

    seen = {}

    def launch(order, start, ngroups, max_group):
        seen.update(order=order, start=start, ngroups=ngroups, max_group=max_group)
        return None

    cross_validate_folds(Plan, np.array([2, -1, 0, 2, 4, 0, 2]), launch)
    assert seen["ngroups"] == 5 and seen["max_group"] == 3
    assert seen["order"].dtype == torch.int32 and seen["start"].dtype == torch.int32
    assert seen["start"].tolist() == [0, 2, 2, 5, 5, 6] and seen["order"].tolist() == [2, 5, 0, 3, 6, 4, 1]
    for bad in (np.full(7, -1), np.array([0, 1, 2, 3, 4, 5, -2]), np.zeros(6, dtype=int), np.zeros(7), np.array([0, 0, 0, 0, 0, 0, 7])):
        with pytest.raises(ValueError):
            cross_validate_folds(Plan, bad, launch)


def _fitted(kind):
    if kind == "loadest":
        covariates, target = loadest_dataset(n=40, seed=1)
        model = LoadestGP()
        model.fit(covariates, target, iterations=8)
    else:
        covariates, target, unc = rating_dataset(n=36, seed=2)
        model = RatingGP()
        model.fit(covariates, target, target_unc=unc, iterations=8)
    return model


@pytest.mark.parametrize("kind", ["loadest", "rating"])
def test_cross_validate_matches_deletion_through_the_oracle_posterior(kind):
    model = _fitted(kind)
    time = model.dm.data.target.coords["time"].values
    y = model._train_y.numpy()
    observed = np.asarray(model.dm.data.target.values, dtype=np.float64)
    for scheme in ("loo", "YE", ("random", 5, 0)):
        groups, labels = cv_folds(time, scheme)
        ds, folds = model.cross_validate(scheme, return_folds=True)
        mu, var, covs = posterior_deletion_reference(model, groups)
        assert np.allclose(ds["predicted"].values, model.dm.y_t(mu).values, rtol=1e-9, atol=0), (kind, scheme)
        assert np.allclose(ds["se"].values, model.dm.error_pipeline.inverse_transform(var).values, rtol=1e-9, atol=0), (kind, scheme)
        z = (y - mu) / np.sqrt(var)
        assert np.allclose(ds["z"].values, z, rtol=1e-9, atol=1e-9 * np.abs(z).max()), (kind, scheme)
        assert np.array_equal(ds["fold"].values, groups) and np.array_equal(ds.coords["time"].values, time)
        assert np.array_equal(ds["observed"].values, observed)
        q = norm.ppf(0.975)
        assert np.allclose(ds["lower"].values, model.dm.y_t(mu - q * np.sqrt(var)).values, rtol=1e-9)
        assert np.allclose(ds["upper"].values, model.dm.y_t(mu + q * np.sqrt(var)).values, rtol=1e-9)
        # the summaries, recomputed from the returned arrays and from the reference's joint densities
        inside = (ds["observed"].values >= ds["lower"].values) & (ds["observed"].values <= ds["upper"].values)
        assert ds.attrs["coverage"] == pytest.approx(inside.mean(), abs=1e-15)
        assert ds.attrs["rmse"] == pytest.approx(np.sqrt(np.mean((y - ds["mu"].values) ** 2)), rel=1e-12)
        assert ds.attrs["rmse"] == pytest.approx(np.sqrt(np.mean((y - mu) ** 2)), rel=1e-9)
        lpd = []
        for f in range(len(labels)):
            B = np.nonzero(groups == f)[0]
            e = (y - mu)[B]
            _sign, logdet = np.linalg.slogdet(covs[f])
            lpd.append(-0.5 * e @ np.linalg.solve(covs[f], e) - 0.5 * logdet - 0.5 * len(B) * np.log(2 * np.pi))
        assert np.allclose(folds["lpd"].values, lpd, rtol=1e-9, atol=1e-9)
        assert ds.attrs["elpd"] == pytest.approx(np.sum(lpd), rel=1e-9)
        assert ds.attrs["elpd"] == pytest.approx(folds["lpd"].values.sum(), rel=1e-12)
        assert ds.attrs["n_folds"] == len(labels) and list(folds["n_points"].values) == list(np.bincount(groups))
        assert np.array_equal(folds.coords["fold"].values, labels)
    assert model.cross_validate("loo").attrs["scheme"] == "loo" and model.cross_validate(4).attrs["scheme"] == "4-block"
    assert 0.0 <= ds.attrs["coverage"] <= 1.0
    narrow = cross_validate(model, "loo", ci=0.5)
    assert narrow.attrs["coverage"] <= model.cross_validate("loo").attrs["coverage"]
    assert np.all(narrow["upper"].values - narrow["lower"].values < ds["upper"].values - ds["lower"].values + 1e-300)


def test_explicit_folds_land_on_the_right_observations():
    model = _fitted("loadest")
    n = model._train_y.shape[0]
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 6, n)
    ids[ids == 4] = 5  # fold id 4 is never used
    ids[[3, 17]] = -1  # two observations are never held out
    ds, folds = model.cross_validate(ids, return_folds=True)
    mu, var, _ = posterior_deletion_reference(model, ids)
    held = ids >= 0
    assert np.allclose(ds["predicted"].values[held], model.dm.y_t(mu[held]).values, rtol=1e-9)
    assert np.all(np.isnan(ds["predicted"].values[~held])) and np.all(np.isnan(ds["z"].values[~held]))
    assert folds["lpd"].values[4] == 0.0 and folds["n_points"].values[4] == 0 and ds.attrs["n_folds"] == 5
    assert ds.attrs["scheme"] == "explicit"
    # permuting the fold ids of the observations permutes the folds, not the observations
    relabel = np.array([5, 3, 0, 1, 4, 2])
    ids2 = np.where(held, relabel[np.clip(ids, 0, None)], -1)
    ds2, folds2 = model.cross_validate(ids2, return_folds=True)
    assert np.allclose(ds2["predicted"].values[held], ds["predicted"].values[held], rtol=1e-12)
    assert np.allclose(folds2["lpd"].values[relabel], folds["lpd"].values, rtol=1e-12, atol=1e-12)
    # moving fold ids between observations moves the results with them
    perm = rng.permutation(n)
    ds3 = model.cross_validate(ids[perm])
    mu3, _var3, _ = posterior_deletion_reference(model, ids[perm])
    h3 = ids[perm] >= 0
    assert np.allclose(ds3["predicted"].values[h3], model.dm.y_t(mu3[h3]).values, rtol=1e-9)
    assert np.array_equal(ds3["fold"].values, ids[perm])


def test_flux_bias():
    model = _fitted("loadest")
    cv = model.cross_validate("loo")
    mode, s, t = target_transform(model.dm)
    assert mode == 1
    flow = np.asarray(model.dm.data.covariates["flow"].values)
    obs = np.asarray(model.dm.data.target.values)
    P = np.exp(s * cv["mu"].values + t + 0.5 * s * s * cv["var"].values) * flow
    direct = (P.sum() - (obs * flow).sum()) / P.sum()
    assert model.flux_bias(cv=cv) == pytest.approx(direct, rel=1e-12)
    assert model.flux_bias() == pytest.approx(direct, rel=1e-12)
    assert flux_bias(model, folds="YE") == pytest.approx(model.flux_bias(cv=model.cross_validate("YE")), rel=1e-12)
    assert abs(direct) < 0.5  # a fitted model is not wildly biased on its own record
    # the lognormal MEAN is used, not the median that `predicted` holds
    median_bias = ((cv["predicted"].values * flow).sum() - (obs * flow).sum()) / (cv["predicted"].values * flow).sum()
    assert direct > median_bias
    # P == O gives exactly 0: a cross-validation whose mean reproduces every observation with no variance
    from discontinuum_amd.xr_compat import Dataset

    exact = Dataset({"mu": ("time", (np.log(obs) - t) / s), "var": ("time", np.zeros_like(obs)), "fold": ("time", np.arange(len(obs)))},
                    coords={"time": cv.coords["time"].values})
    assert abs(model.flux_bias(cv=exact)) < 1e-14
    with pytest.raises(RuntimeError, match="hasn't been fitted"):
        LoadestGP().flux_bias()
    with pytest.raises(RuntimeError, match="hasn't been fitted"):
        RatingGP().cross_validate()


def test_cross_validate_abi_without_a_device():
    lib = _lib.load()
    assert hasattr(lib, "dgp_cross_validate") and hasattr(lib, "dgp_cross_validate_workspace_bytes")
    h = C.c_void_p()
    assert lib.dgp_plan_create(_lib.MODEL_LOADEST, _lib.F64, 1000, 3, C.byref(h)) == 0
    N = lib.dgp_padded_n(1000)
    assert lib.dgp_cross_validate_workspace_bytes(None, 4, 10) == 0
    assert lib.dgp_cross_validate_workspace_bytes(h, 0, 10) == 0 and lib.dgp_cross_validate_workspace_bytes(h, 1001, 1) == 0
    assert lib.dgp_cross_validate_workspace_bytes(h, 4, 0) == 0 and lib.dgp_cross_validate_workspace_bytes(h, 4, 1001) == 0
    loo = lib.dgp_cross_validate_workspace_bytes(h, 1000, 1)
    assert loo >= 8 * (N // 128) * N  # the slab partials of the one pass over T
    small = lib.dgp_cross_validate_workspace_bytes(h, 16, 64)
    assert 0 < small <= 4096  # groups of up to 64 live in LDS
    big = lib.dgp_cross_validate_workspace_bytes(h, 5, 200)
    assert big >= 8 * (3 * 256 * 256 + N * 256)  # at least one block's three matrices and its panel
    assert lib.dgp_cross_validate_workspace_bytes(h, 2, 1000) >= 8 * (3 * N * N + N * N)  # 2-fold works
    p = C.c_void_p(256)  # never dereferenced: every call below fails its host-side checks
    args = lambda **kw: [kw.get("plan", h), kw.get("order", p), p, kw.get("ng", 5), kw.get("mg", 200), kw.get("work", p),  # noqa: E731
                         kw.get("wb", big), p, p, kw.get("lpd", p), p, None]
    assert lib.dgp_cross_validate(*args(plan=None)) == -1 and b"null" in lib.dgp_last_error()
    assert lib.dgp_cross_validate(*args(order=None)) == -1 and b"null" in lib.dgp_last_error()
    assert lib.dgp_cross_validate(*args(lpd=None)) == -1
    assert lib.dgp_cross_validate(*args(ng=0)) == -1 and b"size" in lib.dgp_last_error()
    assert lib.dgp_cross_validate(*args(ng=1001)) == -1
    assert lib.dgp_cross_validate(*args(mg=0)) == -1 and lib.dgp_cross_validate(*args(mg=1001)) == -1
    assert lib.dgp_cross_validate(*args()) == -3 and b"workspace" in lib.dgp_last_error()  # the plan has no workspace yet
    assert lib.dgp_plan_destroy(h) == 0
