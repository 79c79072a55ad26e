"""The influence of the held samples on the period sums without a GPU: the identities ``dgp_deletion_influence`` implements
against brute-force deletion through the oracle's posterior on every case of the GPU suite (bound 1e-10, two orders inside
the GPU bound, as in tests/test_sensitivity_cpu.py), the host logic of ``discontinuum_amd.influence`` on the plan double, and
the C ABI of the entry point.

Measured here (formulas against deletion, worst over the 105 cases, every fold scheme, both modes): load change 9.5e-14,
variance change 4.0e-11 (rating n = 300, one fold holding everything: the prior's variance is 1e5 times the posterior's, and
the reference itself subtracts the two), shift 8.6e-13."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from discontinuum_amd.engines.base import ModelConfig
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.influence import jackknife_se
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.rating_gp import RatingGP
from discontinuum_amd.xr_compat import Dataset
from tests import influence_helpers as ih
from tests.flux_helpers import daily_loadest, daily_rating

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("model,d,n,m", ih.CASES)
def test_formulas_against_deletion(model, d, n, m):
    name, X, r, noise, theta, Xs = ih.build_case(model, d, n, m)
    w, periods, P = ih.record(m)
    for scheme, ids in ih.fold_schemes(n).items():
        refs = ih.reference(model, d, n, m, scheme)
        for mode in (ih.MODE_LINEAR, ih.MODE_LOG):
            ref = refs[mode]
            dload, dvar, shift, info = ih.formula_deletion_influence(name, X, r, noise, theta, Xs, ids, ref["a"], ih.SCALE, periods, P, mode,
                                                                     ref["inv_sd"])
            assert int(info.abs().max()) == 0  # the oracle alone has no failing fold at these shapes
            el, ev, es = ih.errors(ref, dload, dvar, shift)
            assert el <= 1e-10 and es <= 1e-10 and (ev is None or ev <= 1e-10), (model, d, n, m, scheme, mode, el, ev, es)
            if dvar is not None:
                assert bool((dvar >= 0).all())


def test_the_reference_is_the_oracles_posterior_on_the_remaining_rows():
    """``influence_helpers`` evaluates the Grams once and drops rows: the same numbers as ``oracle.posterior`` on the rest."""
    from oracle import gp_oracle as orc

    name, X, r, noise, theta, Xs = ih.build_case("rating", 2, 129, 130)
    keep = torch.as_tensor(np.setdiff1d(np.arange(129), np.arange(7, 129, 9)))
    gram = orc.GRAMS[name]
    mu, cov = ih._posterior_of_rows(gram(X, X, theta) + torch.diag(noise), gram(X, Xs, theta), gram(Xs, Xs, theta), r, keep)
    mu_o, cov_o = orc.posterior(name, X[keep], r[keep], noise[keep], theta, Xs, full_cov=True)
    assert torch.equal(mu, mu_o) and torch.equal(cov, cov_o)


# ------------------------------------------------------------------------------------------------ the host logic
@pytest.fixture()
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(ih.InfluenceOraclePlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)


def _fitted(kind):
    if kind in ("loadest", "loadest-linear"):
        cov_obs, target, daily = daily_loadest(n_obs=200, seed=0, step_days=5)
        model = LoadestGP() if kind == "loadest" else LoadestGP(model_config=ModelConfig(transform="standard"))
        model.fit(cov_obs, target, iterations=6)
        return model, daily
    cov_obs, target, unc, daily = daily_rating(n_obs=150, seed=0)
    daily = Dataset({"stage": ("time", np.asarray(daily["stage"].values)[::6])}, coords={"time": np.asarray(daily.coords["time"].values)[::6]})
    model = RatingGP()
    model.fit(cov_obs, target, target_unc=unc, iterations=6)
    return model, daily


def _through_the_oracles(model, kind, daily, weights, folds, freq="YE"):
    return ih.engine_reference(model, kind, daily, weights, folds, freq)


@pytest.mark.parametrize("kind", ["loadest", "rating", "loadest-linear"])
@pytest.mark.parametrize("folds", ["loo", "YE", 5, ("random", 4, 3)])
def test_public_methods_against_deletion_through_the_model_oracles(kind, folds, cpu_engine):
    from discontinuum_amd.loads import _target_attrs, flux_weights

    model, daily = _fitted(kind)
    if kind != "rating":
        w = flux_weights(daily, _target_attrs(model.dm))
        ds = model.sample_influence(daily, folds=folds, freq="YE")
    else:
        w = np.ones(len(daily.coords["time"].values))
        ds = model.influence(daily, w, folds=folds, freq="YE")
    ref, ids, periods, P, mode = _through_the_oracles(model, kind.split("-")[0], daily, w, folds)
    assert mode == (0 if kind == "loadest-linear" else 1)
    el, ev, es = ih.errors(ref, ds["load_change"].values, ds["var_change"].values if mode == 0 else None, ds["max_shift"].values)
    # the engine-level bound of the GPU suite (1e-7): the engine's and the oracle's hyperparameters agree to rounding only, and
    # cond(K^) carries that into the posterior; measured here: 4.8e-11 (load), 1.9e-9 (variance, a year deleted), 7.1e-12 (shift)
    assert el <= 1e-7 and es <= 1e-7 and (ev is None or ev <= 1e-7), (el, ev, es)
    load = ref["load"].numpy()
    assert np.allclose(ds["load"].values, load, rtol=1e-10)
    assert np.array_equal(ds["load_without"].values, ds["load"].values[None, :] + ds["load_change"].values)
    assert np.allclose(ds["relative_change"].values, ds["load_change"].values / load[None, :], rtol=1e-9)
    assert ds["load_change"].values.shape == (int(ids.max()) + 1, P) and int(np.abs(ds["info"].values).max()) == 0
    assert np.array_equal(ds["fold_size"].values, np.bincount(ids[ids >= 0]))
    assert ds.attrs["hyperparameters"] == "held fixed" and ds.attrs["sign"] == "without the fold minus with it"
    # the sign convention, spelled out: load_change is (the load of a fit WITHOUT the fold) - (the load of the full fit)
    assert np.allclose(ds["load_without"].values, (ref["load"][None, :] + ref["dload"]).numpy(), rtol=1e-8)
    if mode == 0:
        assert np.all(ds["var_change"].values >= 0)
        assert np.allclose(ds["se_without"].values ** 2, (ref["var"][None, :] + ref["dvar"]).numpy(), rtol=1e-7)
    # the folds partition the observations: the delete-a-group jackknife is reported
    k = len(ds["fold_size"].values)
    lw = ds["load_without"].values
    jk = np.sqrt((k - 1) / k * ((lw - lw.mean(axis=0)) ** 2).sum(axis=0))
    assert np.allclose(ds["se_jackknife"].values, jk, rtol=1e-12) and np.all(jk > 0)


def test_jackknife_needs_a_partition_and_empty_folds_change_nothing(cpu_engine):
    model, daily = _fitted("loadest")
    n = 200
    ids = np.arange(n) % 4
    ids[ids == 2] = 5  # fold ids 2, 3 -> 5, 3: ids 2 and 4 are empty
    ds = model.sample_influence(daily, folds=ids)
    assert ds["load_change"].values.shape[0] == 6
    for empty in (2, 4):
        assert np.all(ds["load_change"].values[empty] == 0) and ds["fold_size"].values[empty] == 0 and ds["max_shift"].values[empty] == 0
    lw = ds["load_without"].values[[0, 1, 3, 5]]  # the empty folds do not count: k = 4
    assert np.allclose(ds["se_jackknife"].values, np.sqrt(3 / 4 * ((lw - lw.mean(axis=0)) ** 2).sum(axis=0)), rtol=1e-12)
    ids[7] = -1  # one observation in no fold: not a partition any more
    ds2 = model.sample_influence(daily, folds=ids)
    assert np.all(np.isnan(ds2["se_jackknife"].values)) and np.all(np.isfinite(ds2["load_change"].values))
    assert np.all(np.isnan(jackknife_se(np.ones((1, 3)), np.array([n]), n)))  # a single fold has no spread


def test_deleting_everything_returns_the_prior(cpu_engine):
    from discontinuum_amd.loads import _kept, _target_attrs, flux_weights, period_groups, target_transform

    model, daily = _fitted("loadest")
    ds = model.sample_influence(daily, folds=np.zeros(200, dtype=np.int64))
    w = flux_weights(daily, _target_attrs(model.dm))
    order, periods, labels, _n, _d = _kept(*period_groups(daily.coords["time"].values, w, "YE"))
    x = torch.tensor(model.dm.Xnew(daily), dtype=torch.float64)[torch.as_tensor(order)]
    mode, s, t = target_transform(model.dm)
    with torch.no_grad():
        from oracle import gp_oracle as orc

        prior_var = torch.diagonal(orc.GRAMS["loadest"](x, x, model._factor_theta.double()))
        point = torch.as_tensor(w[order]) * torch.exp(s * model.model.prior_mean(x).double() + t + 0.5 * s * s * prior_var)
    prior_load = np.bincount(periods, weights=point.numpy(), minlength=len(labels))
    assert mode == 1 and np.allclose(ds["load_without"].values[0], prior_load, rtol=1e-9)


def test_bad_folds_and_budget_raise(cpu_engine):
    model, daily = _fitted("loadest")
    for bad in ("nonsense", 0, 201, np.zeros(199, dtype=np.int64), np.full(200, -1), np.zeros(200), ("random", 0, 1)):
        with pytest.raises(ValueError):
            model.sample_influence(daily, folds=bad)
    with pytest.raises(ValueError, match="max_bytes"):
        model.sample_influence(daily, max_bytes=1000)


# ------------------------------------------------------------------------------------------------ the C entries
def test_abi_of_dgp_deletion_influence():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "dgp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(dgp_deletion_influence\w*)\s*\(([^;]*?)\)\s*;", text)}
    assert decl["dgp_deletion_influence_workspace_bytes"] == "const dgp_plan* plan, int64_t m, int nfolds, int64_t max_fold, int ngroups"
    assert decl["dgp_deletion_influence"] == (
        "dgp_plan* plan, const double* theta_host, const void* Xs_dev, int64_t m, const int32_t* order_dev, const int32_t* start_dev, "
        "int nfolds, int64_t max_fold, int mode, const double* a_dev, const double* scale_dev, const int32_t* group_dev, int ngroups, "
        "const double* inv_sd_dev, void* work_dev, size_t work_bytes, double* dload_dev, double* dvar_dev, double* shift_dev, "
        "int32_t* info_dev, void* stream")
    vp, i, i64, sz, dp = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.POINTER(C.c_double)
    assert _lib.SIGNATURES["dgp_deletion_influence_workspace_bytes"] == (sz, [vp, i64, i, i64, i])
    assert _lib.SIGNATURES["dgp_deletion_influence"] == (i, [vp, dp, vp, i64, vp, vp, i, i64, i, vp, vp, vp, i, vp, vp, sz, vp, vp, vp, vp, vp])
    assert hasattr(lib, "dgp_deletion_influence") and hasattr(lib, "dgp_deletion_influence_workspace_bytes")
    # queries and argument checks need no device
    h = C.c_void_p()
    assert lib.dgp_plan_create(_lib.MODEL_RATING, _lib.F32, 300, 2, C.byref(h)) == 0
    q = lib.dgp_deletion_influence_workspace_bytes
    N, M = 384, 256
    for good in ((130, 300, 1, 3), (130, 5, 64, 3), (130, 3, 129, 3), (1, 1, 300, 1), (1 << 20, 300, 1, 65535)):
        assert q(h, *good) >= 3 * N * 128 * 4 and q(h, *good) % 256 == 0
    assert q(h, 130, 300, 1, 3) >= 3 * N * M * 4
    assert q(h, 130, 5, 64, 3) - q(h, 130, 5, 2, 3) >= 5 * (64 * 64 - 2 * 2) * 8 - 512  # M^-1 of every fold of the LDS route
    assert q(h, 130, 3, 129, 3) - q(h, 130, 3, 64, 3) >= 2 * 256 * M * 8  # one block-route chunk: panel and Z at order 256
    for bad in ((0, 3, 1, 3), (-1, 3, 1, 3), ((1 << 20) + 1, 3, 1, 3), (130, 0, 1, 3), (130, 301, 1, 3), (130, 3, 0, 3), (130, 3, 301, 3),
                (130, 3, 1, 0), (130, 3, 1, 65536)):
        assert q(h, *bad) == 0, bad
    assert q(None, 130, 3, 1, 3) == 0
    theta = (C.c_double * 16)(*([1.0] * 16))
    fake = C.c_void_p(256)  # never dereferenced: every call below fails its checks first

    def call(plan=h, th=theta, xs=fake, m=130, order=fake, nfolds=3, maxf=1, mode=0, a=fake, ngroups=3, isd=fake, dload=fake, dvar=fake,
             shift=fake, info=fake):
        return lib.dgp_deletion_influence(plan, th, xs, m, order, fake, nfolds, maxf, mode, a, fake, fake, ngroups, isd, fake, 1 << 40, dload, dvar,
                                          shift, info, None)

    assert call(plan=None) == -1 and call(th=None) == -1 and call(xs=None) == -1 and call(order=None) == -1 and call(a=None) == -1
    assert call(dload=None) == -1 and call(info=None) == -1
    assert call(m=0) == -1 and call(nfolds=0) == -1 and call(nfolds=301) == -1 and call(maxf=0) == -1 and call(maxf=301) == -1
    assert call(ngroups=0) == -1 and b"bad size" in lib.dgp_last_error()
    assert call(mode=2) == -1 and call(mode=-1) == -1
    assert call(mode=1) == -1 and b"mode 0 only" in lib.dgp_last_error()  # dvar in mode 1
    assert call(isd=None) == -1 and b"inv_sd" in lib.dgp_last_error()    # shift without 1 / sigma
    assert call() == -3 and call(mode=1, dvar=None) == -3                 # a plan without workspace
    assert lib.dgp_plan_destroy(h) == 0
