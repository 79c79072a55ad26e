"""Cross-validation of censored fits by Laplace cavity folds on CPU: the dense helpers (deletion in the W-form against the
G / Sigma identity the device code uses, the cavity against a refit per fold) and the host side -- ``cross_validate(...,
laplace="cavity")`` and ``flux_bias(..., laplace="cavity")`` -- over an oracle plan that answers
``GPPlan.laplace_cross_validate`` from the dense helper."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch
from scipy import integrate
from scipy.stats import norm

from discontinuum_amd import _lib
from discontinuum_amd.backend import MODE_LOG
from discontinuum_amd.loadest_gp import LoadestGP, censoring_from_bounds
from discontinuum_amd.loads import target_transform
from discontinuum_amd.validation import cross_validate, cv_folds, flux_bias
from oracle import gp_oracle as orc
from tests import censored_cv_helpers as cvh
from tests import censored_helpers as ch
from tests import interval_helpers as ih
from tests.crossval_helpers import CVOraclePlan
from tests.helpers import loadest_dataset

LN2 = 0.6931471805599453


def _theta(d=2):
    nt = orc.loadest_ntheta(d)
    return torch.full((nt,), LN2, dtype=torch.float64) * torch.linspace(0.8, 1.3, nt, dtype=torch.float64)


def plan_fixture(n, seed):
    """The plan-level dataset of tests/test_gpu_censored_cv.py and its mode (numpy)."""
    X, _ = orc.synth_loadest(n, 2, seed=seed)
    y, side, v, m, upper = cvh.censored_fixture(X, seed)
    theta = _theta()
    K = ch.gram("loadest", torch.tensor(X), theta)
    f, _it, _dmax, _halv, conv = ih.newton(K, y, side, v, m, upper)
    assert conv
    return X, y, side, v, m, upper, theta, K, f


def plan_schemes(n):
    """The fold schemes of the GPU test: LOO, i mod 7, i mod 2, contiguous 170 / 130 (n = 300 only), and one with rows that are
    never held out and an unused fold id."""
    holes = np.arange(n) % 5
    holes[::11] = -1
    holes[holes == 3] = 6  # ids 3, 5 unused
    out = {"loo": np.arange(n), "mod7": np.arange(n) % 7, "mod2": np.arange(n) % 2, "holes": holes}
    if n == 300:
        out["contiguous"] = (np.arange(n) >= 170).astype(np.int64)
    return out


PLAN_CASES = ((130, 1), (300, 7))


@pytest.mark.parametrize("n,seed", PLAN_CASES)
def test_deletion_and_identity_agree_on_the_gpu_datasets(n, seed):
    """The condition under which the device comparison means anything: the reference (deletion, W-form) and the identity the
    device uses agree to 1e-10 on the very datasets and folds of the GPU test."""
    X, y, side, v, m, upper, theta, K, f = plan_fixture(n, seed)
    tm = ih.terms(f, y, side, v, m, upper)
    assert tm["capped"] == 5 and sorted(set(side.tolist())) == [-1, 0, 1, 2]
    for name, g in plan_schemes(n).items():
        held = g >= 0
        mu_d, vc_d = cvh.latent_cavity(K, y, side, v, m, f, g, upper)
        mu_i, vc_i = cvh.identity_cavity(K, y, side, v, m, f, g, upper)
        assert np.max(np.abs(mu_i - mu_d)[held]) <= 1e-10 * np.max(np.abs(mu_d[held])), name
        assert np.max(np.abs(vc_i - vc_d)[held] / vc_d[held]) <= 1e-10, name
        assert np.all(mu_d[~held] == 0.0) and np.all(vc_d[~held] == 0.0)


def test_subtraction_form_fails_on_capped_rows():
    """Why the identity: ``C_ii - n~_i`` from the pseudo-data's own leave-one-out loses the capped rows' variance."""
    X, y, side, v, m, upper, theta, K, f = plan_fixture(130, 1)
    tm = ih.terms(f, y, side, v, m, upper)
    capped = tm["nn"] > 1e9 * v
    assert capped.sum() == 5
    _mu, vc = cvh.latent_cavity(K, y, side, v, m, f, np.arange(130), upper)
    G = np.linalg.inv(K + np.diag(tm["nn"]))
    sub = 1.0 / np.diag(G) - tm["nn"]
    assert np.max(np.abs(sub - vc)[capped] / vc[capped]) > 1e-6
    assert np.max(np.abs(sub - vc)[~capped] / vc[~capped]) < 1e-6


def test_planes_of_an_all_observed_fit_are_the_gaussian_ones():
    X, _ = orc.synth_loadest(50, 2, seed=4)
    y, side, v, m = ch.synth(X, 0.3, 4)
    side[:] = 0
    K = ch.gram("loadest", torch.tensor(X), _theta())
    f = m + K @ np.linalg.solve(K + np.diag(v), y - m)
    g = np.arange(50) % 4
    res = cvh.dense_cavity_cv(K, y, side, v, m, f, g, shift=0.7)
    from tests.crossval_helpers import dense_deletion_cv

    resid, var, _lpd = dense_deletion_cv(K + np.diag(v), y - m, g)
    assert np.allclose(res["mu"], y - resid.numpy(), rtol=0, atol=1e-12) and np.allclose(res["var"], var.numpy(), rtol=1e-11)
    assert np.allclose(res["lpd"], norm.logpdf(y, res["mu"], np.sqrt(res["var"])), rtol=1e-12)
    assert np.array_equal(res["pit_lower"], res["pit_upper"]) and np.all(res["tilt"] == 0.0)


# ---- the cavity against a refit per fold (the approximation itself).  Recorded on this fixture ("Cross-validation of
# censored fits"); the assertions allow three times the recorded value: room for another seed's draw.
REFIT_RECORDED = {  # scheme: (median gap of the held-out mean in held-out sd, its 90th percentile, |delta elpd|)
    "loo": (6.8e-6, 3.5e-3, 0.154),
    "mod6": (9.1e-4, 1.6e-2, 0.114),
}


@pytest.mark.parametrize("scheme", sorted(REFIT_RECORDED))
def test_cavity_against_refit(scheme):
    n, seed = 60, 12
    X, _ = orc.synth_loadest(n, 2, seed=seed)
    y, side, v, m = ch.synth(X, 0.3, seed)
    K = ch.gram("loadest", torch.tensor(X), _theta())
    f, _it, _dmax, _halv, conv = ih.newton(K, y, side, v, m)
    assert conv
    g = np.arange(n) if scheme == "loo" else np.arange(n) % 6
    cav = cvh.dense_cavity_cv(K, y, side, v, m, f, g)
    ref = cvh.refit_cv(K, y, side, v, m, f, g)
    gap = np.abs(cav["mu"] - ref["mu"]) / np.sqrt(ref["var"])
    median, p90, delpd = float(np.median(gap)), float(np.percentile(gap, 90)), abs(float(cav["lpd"].sum() - ref["lpd"].sum()))
    print(f"cavity vs refit, {scheme}: median {median:.3e}, p90 {p90:.3e}, |delta elpd| {delpd:.3e}")
    rec = REFIT_RECORDED[scheme]
    assert median <= 3 * rec[0] and p90 <= 3 * rec[1] and delpd <= 3 * rec[2]
    assert delpd > 0.0  # an approximation: the refit is not reproduced exactly


# ---- the host side over the oracle plan
class _Plan(cvh.LaplaceCVOraclePlan):
    cross_validate = CVOraclePlan.cross_validate


@pytest.fixture()
def cpu_engine(monkeypatch):
    monkeypatch.setattr(LoadestGP, "_plan_factory", staticmethod(_Plan))
    monkeypatch.setattr(LoadestGP, "device", "cpu")
    return LoadestGP


def _bounds(target, seed=1, k2=6, kminus=4, kplus=2):
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


@pytest.fixture()
def fitted(cpu_engine):
    cov, target = loadest_dataset(40, seed=2)
    low, high = _bounds(target)
    tgt, codes, upper = censoring_from_bounds(low, high)
    assert sorted(set(codes.tolist())) == [-1, 0, 1, 2]
    m = cpu_engine()
    m.fit(cov, tgt, iterations=4, censored=codes, target_upper=upper)
    return m, cov, tgt, codes, upper


def _dense(m, groups, shift):
    with torch.no_grad():
        theta = m._theta_fn().detach()
        mean = m.model.prior_mean(m._train_x).numpy()
        noise = m.likelihood.train_noise(torch.device("cpu"), torch.float64).numpy()
    K = ch.gram("loadest", m._train_x, theta)
    return cvh.dense_cavity_cv(K, m._train_y.numpy(), m._censor.side.numpy(), np.broadcast_to(noise, mean.shape), mean, m._censor.f.numpy(),
                               groups, m._censor.upper.numpy(), shift)


@pytest.mark.parametrize("folds", ["loo", "YE", 5, ("random", 4, 3)], ids=["loo", "YE", "k5", "random"])
def test_dataset_contents(fitted, folds):
    m, cov, tgt, codes, upper = fitted
    ds, per_fold = m.cross_validate(folds, return_folds=True, laplace="cavity")
    groups, labels = cv_folds(np.asarray(tgt.coords["time"].values), folds)
    mode, s, _t = target_transform(m.dm)
    assert mode == MODE_LOG
    ref = _dense(m, groups, s)
    side = codes.astype(np.int64)
    assert m._plan.cavity_calls >= 1
    assert np.array_equal(ds["censored"].values, side) and np.array_equal(ds["fold"].values, groups)
    assert np.array_equal(ds["observed"].values, np.asarray(tgt.values))
    up = ds["observed_upper"].values
    assert np.array_equal(np.isnan(up), side != 2) and np.array_equal(up[side == 2], np.asarray(upper)[side == 2])
    for k in ("mu", "var", "lpd", "pit_lower", "pit_upper", "dlp", "tilt"):
        assert np.array_equal(ds[k].values, ref[k]), k
    # predicted / se / lower / upper from mu, var exactly as the plain path builds them
    mu, var = ds["mu"].values, ds["var"].values
    q = norm.ppf(0.975)
    assert np.array_equal(ds["predicted"].values, np.asarray(m.dm.y_t(mu).values).reshape(-1))
    assert np.array_equal(ds["lower"].values, np.asarray(m.dm.y_t(mu - q * np.sqrt(var)).values).reshape(-1))
    assert np.array_equal(ds["upper"].values, np.asarray(m.dm.y_t(mu + q * np.sqrt(var)).values).reshape(-1))
    assert np.array_equal(ds["se"].values, np.asarray(m.dm.error_pipeline.inverse_transform(var).values).reshape(-1))
    # attributes
    a = ds.attrs
    assert a["elpd"] == pytest.approx(ds["lpd"].values.sum(), rel=1e-14) and a["elpd_kind"] == "pointwise"
    assert a["approximation"] == "laplace-cavity" and a["n_censored"] == int((side != 0).sum()) and a["ci"] == 0.95
    assert a["n_folds"] == len(labels) and a["scheme"] == {"loo": "loo", "YE": "YE", 5: "5-block"}.get(folds, "random-4-3")
    obs = side == 0
    y = m._train_y.numpy()
    assert a["rmse"] == pytest.approx(math.sqrt(np.mean((y - mu)[obs] ** 2)), rel=1e-14)
    inside = (ds["observed"].values >= ds["lower"].values) & (ds["observed"].values <= ds["upper"].values)
    assert a["coverage"] == pytest.approx(inside[obs].mean(), rel=1e-14)
    # z: observed rows only
    z = ds["z"].values
    assert np.all(np.isnan(z[~obs])) and np.allclose(z[obs], ((y - mu) / np.sqrt(var))[obs], rtol=1e-14)
    # PIT bounds per row kind
    lo, hi = ds["pit_lower"].values, ds["pit_upper"].values
    assert np.array_equal(lo[obs], hi[obs]) and np.all(lo[side == -1] == 0.0) and np.all(hi[side == 1] == 1.0)
    assert np.all(lo[side == 2] < hi[side == 2]) and np.all((lo >= 0) & (hi <= 1))
    assert np.allclose(np.exp(ds["lpd"].values[side != 0]), (hi - lo)[side != 0], rtol=1e-9)
    assert np.all(ds["tilt"].values[obs] == 0.0) and np.any(ds["tilt"].values[~obs] != 0.0)
    # per fold: the sum of the pointwise lpd
    assert np.array_equal(per_fold["n_points"].values, np.bincount(groups, minlength=len(labels)))
    assert np.allclose(per_fold["lpd"].values, np.bincount(groups, weights=ds["lpd"].values, minlength=len(labels)), rtol=1e-13)
    assert per_fold["lpd"].values.sum() == pytest.approx(a["elpd"], rel=1e-13)


def test_rows_never_held_out(fitted):
    m, _cov, _tgt, codes, _upper = fitted
    groups = np.arange(40) % 3
    groups[[0, 7, 20]] = -1
    ds = cross_validate(m, groups, laplace="cavity")
    out = groups < 0
    for k in ("mu", "var", "lpd", "pit_lower", "pit_upper", "z", "dlp", "tilt"):
        assert np.all(np.isnan(ds[k].values[out])), k
    assert ds.attrs["elpd"] == pytest.approx(np.nansum(ds["lpd"].values), rel=1e-14) and np.isfinite(ds.attrs["rmse"])


def test_flux_bias_against_quadrature(fitted):
    m, cov, tgt, codes, _upper = fitted
    cv = m.cross_validate("loo", laplace="cavity")
    mode, s, t = target_transform(m.dm)
    mu, var = cv["mu"].values, cv["var"].values
    sd = np.sqrt(var)
    y, up = m._train_y.numpy(), m._censor.upper.numpy()
    flow = np.asarray(cov["flow"].values, dtype=np.float64)
    O = np.asarray(tgt.values, dtype=np.float64).copy()
    for i in np.flatnonzero(codes != 0):
        a = -np.inf if codes[i] == -1 else y[i]
        b = np.inf if codes[i] == 1 else (y[i] if codes[i] == -1 else up[i])
        a, b = max(a, mu[i] - 12 * sd[i] - 2), min(b, mu[i] + 12 * sd[i] + 2)
        num = integrate.quad(lambda c: math.exp(s * c + t) * norm.pdf(c, mu[i], sd[i]), a, b, epsabs=0, epsrel=1e-12, limit=200)[0]
        den = integrate.quad(lambda c: norm.pdf(c, mu[i], sd[i]), a, b, epsabs=0, epsrel=1e-12, limit=200)[0]
        O[i] = num / den
    P = np.exp(s * mu + t + 0.5 * s * s * var)
    direct = ((P * flow).sum() - (O * flow).sum()) / (P * flow).sum()
    assert m.flux_bias(cv=cv, laplace="cavity") == pytest.approx(direct, rel=1e-8, abs=1e-10)
    assert m.flux_bias(laplace="cavity") == pytest.approx(direct, rel=1e-8, abs=1e-10)
    assert flux_bias(m, folds="YE", laplace="cavity") == pytest.approx(m.flux_bias(cv=m.cross_validate("YE", laplace="cavity"), laplace="cavity"),
                                                                        rel=1e-12)
    # a bracket lies inside its own ends: O of a censored row does
    exp_c = np.exp(s * mu + t + 0.5 * s * s * var + cv["tilt"].values)
    br = codes == 2
    assert np.all(exp_c[br] > np.asarray(tgt.values)[br]) and np.all(exp_c[br] < cv["observed_upper"].values[br])
    with pytest.raises(ValueError, match="cavity"):
        m.flux_bias(cv=Dataset_without_approximation(cv), laplace="cavity")


def Dataset_without_approximation(cv):
    from discontinuum_amd.xr_compat import Dataset

    return Dataset({k: ("time", cv[k].values) for k in ("mu", "var", "fold")}, coords={"time": cv.coords["time"].values})


def test_linear_target_expectation_through_dlp():
    """s (mu + var dlp) + t is the mean of the truncated normal: the dense planes against scipy's truncnorm."""
    from scipy.stats import truncnorm

    mu, vc, v = np.array([0.1, -0.3, 0.4]), np.array([0.02, 0.05, 0.01]), np.array([0.01, 0.01, 0.01])
    y, side, upper = np.array([0.0, 0.2, 0.35]), np.array([-1, 1, 2]), np.array([np.nan, np.nan, 0.6])
    pl = cvh.row_planes(mu, vc, y, side, v, upper)
    sd = np.sqrt(vc + v)
    lo = np.array([-np.inf, (y[1] - mu[1]) / sd[1], (y[2] - mu[2]) / sd[2]])
    hi = np.array([(y[0] - mu[0]) / sd[0], np.inf, (upper[2] - mu[2]) / sd[2]])
    assert np.allclose(mu + (vc + v) * pl["dlp"], truncnorm.mean(lo, hi, loc=mu, scale=sd), rtol=1e-10)


def test_default_still_refuses_with_the_hint(fitted):
    m = fitted[0]
    for call in (m.cross_validate, m.flux_bias, lambda: cross_validate(m), lambda: flux_bias(m)):
        with pytest.raises(NotImplementedError, match="not available for a fit with censored observations") as e:
            call()
        assert 'laplace="cavity"' in str(e.value)
    with pytest.raises(NotImplementedError, match="censored") as e:
        m.hyperparameter_uncertainty()
    assert "cavity" not in str(e.value)  # the hint belongs to the two calls that have the alternative
    for bad in ("refit", True, 1):
        with pytest.raises(ValueError, match="laplace"):
            m.cross_validate(laplace=bad)
        with pytest.raises(ValueError, match="laplace"):
            m.flux_bias(laplace=bad)


def test_uncensored_fit_ignores_the_keyword(cpu_engine):
    cov, target = loadest_dataset(40, seed=2)
    m = cpu_engine()
    m.fit(cov, target, iterations=3)
    assert m._censor is None
    for folds in ("loo", "YE"):
        a, fa = m.cross_validate(folds, return_folds=True)
        b, fb = m.cross_validate(folds, return_folds=True, laplace="cavity")
        assert set(a) == set(b) and a.attrs == b.attrs and "lpd" not in set(b)
        for k in list(a):
            assert np.array_equal(a[k].values, b[k].values, equal_nan=True), k
        assert np.array_equal(fa["lpd"].values, fb["lpd"].values)
    assert m.flux_bias() == m.flux_bias(laplace="cavity")
    assert getattr(m._plan, "cavity_calls", 0) == 0
    with pytest.raises(ValueError, match="laplace"):
        m.cross_validate(laplace="loo")


def test_abi_declares_the_entry():
    assert _lib.SIGNATURES["dgp_laplace_cross_validate_workspace_bytes"][1] == _lib.SIGNATURES["dgp_cross_validate_workspace_bytes"][1]
    assert len(_lib.SIGNATURES["dgp_laplace_cross_validate"][1]) == 18 and len(_lib.LCV_PLANE_NAMES) == 7
    assert tuple(_lib.LCV_PLANE_NAMES) == cvh.PLANES
