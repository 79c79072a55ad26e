"""Censored observations (non-detects) without a GPU: the dense restatement checks itself (direct formula, central
differences), and the engine's host side -- ``fit(censored=...)``, the warm start, the prediction-time cache build, the
refusals, checkpointing -- runs over the oracle-backed plan."""
import io

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from discontinuum_amd.engines.hip import censor_sides
from discontinuum_amd.loadest_gp import LoadestGP
from oracle import gp_oracle as orc
from tests import censored_helpers as ch
from tests.helpers import loadest_dataset, rating_dataset

LN2 = 0.6931471805599453


def _fixture(n=40, d=2, ncens=8, seed=3):
    X, _y = orc.synth_loadest(n, d, seed=seed)
    y, side, v, m = ch.synth(X, ncens / n, seed, ends=False)
    assert (side == -1).any() and (side == 1).any() and (side != 0).sum() == ncens
    theta = torch.full((orc.loadest_ntheta(d),), LN2, dtype=torch.float64)
    theta = theta * torch.linspace(0.8, 1.3, theta.numel(), dtype=torch.float64)
    return torch.tensor(X), y, side, v, m, theta


def test_helper_direct_formula_equals_engine_plus_correction():
    X, y, side, v, m, theta = _fixture()
    res = ch.laplace("loadest", X, y, side, v, m, theta, tol=1e-12)
    assert res["converged"] and res["capped"] == 0 and 2 <= res["iterations"] <= 30
    direct = ch.nll_direct(res, y, side, v, m)
    assert abs(direct - res["nll"]) <= 1e-11 * abs(direct), (direct, res["nll"])
    # the mode is a stationary point: grad log p = K^-1 (f - m) = a
    tm = ch.terms(res["f"], y, side, v, m)
    assert np.max(np.abs(tm["g"] - res["alpha"])) < 1e-8
    # with nothing censored the correction vanishes and the engine's own value is left
    none = ch.laplace("loadest", X, y, np.zeros_like(side), v, m, theta)
    assert none["corr"] == 0.0 and none["iterations"] == 0 and np.all(none["dr"] == none["alpha"])


def test_helper_gradients_against_central_differences():
    X, y, side, v, m, theta = _fixture()
    res = ch.laplace("loadest", X, y, side, v, m, theta, tol=1e-12)

    def nll(th, mean):
        return ch.laplace("loadest", X, y, side, v, mean, th, f0=res["f"], tol=1e-13, with_grad=False)["nll"]

    step = 1e-5
    for p in range(theta.numel()):
        e = torch.zeros_like(theta)
        e[p] = step
        fd = (nll(theta + e, m) - nll(theta - e, m)) / (2 * step)
        assert abs(fd - res["dtheta"][p]) <= 1e-6 * max(1.0, abs(fd)), (p, fd, res["dtheta"][p])
    # d NLL_L / d r_i = alpha_i - u_i: a shift of the prior mean at row i is minus that; rows of both kinds
    for i in (0, int(np.flatnonzero(side == -1)[0]), int(np.flatnonzero(side == 1)[0]), 17):
        e = np.zeros_like(m)
        e[i] = step
        fd = (nll(theta, m + e) - nll(theta, m - e)) / (2 * step)
        assert abs(-fd - res["dr"][i]) <= 1e-6 * max(1.0, abs(fd)), (i, fd, res["dr"][i])
    fd = (nll(theta, m + step) - nll(theta, m - step)) / (2 * step)  # a constant mean: -sum (alpha - u)
    assert abs(fd + res["dr"].sum()) <= 1e-6 * max(1.0, abs(fd))


def test_scalar_mode_by_bisection():
    X = torch.tensor([[0.3, -0.2]])
    theta = torch.full((orc.loadest_ntheta(2),), LN2, dtype=torch.float64)
    for s, limit in ((-1, -0.4), (1, 0.9)):
        res = ch.laplace("loadest", X, np.array([limit]), np.array([s]), np.array([0.01]), np.array([0.1]), theta, tol=1e-13)
        ref = ch.scalar_mode(float(res["K"][0, 0]), limit, s, 0.01, 0.1)
        assert res["converged"] and abs(res["f"][0] - ref) < 1e-11, (res["f"], ref)


def test_censor_argument_forms():
    assert censor_sides(None, 3) is None and censor_sides(np.zeros(3, dtype=bool), 3) is None and censor_sides([0, 0, 0], 3) is None
    assert censor_sides(np.array([True, False, True]), 3).tolist() == [-1, 0, -1]
    assert censor_sides([1, 0, -1], 3).tolist() == [1, 0, -1] and censor_sides([1, 0, -1], 3).dtype == np.int32
    with pytest.raises(ValueError, match="align"):
        censor_sides([0, 1], 3)
    with pytest.raises(ValueError, match="-1"):
        censor_sides([0, 2, 0], 3)


@pytest.fixture()
def cpu_engine(monkeypatch):
    monkeypatch.setattr(LoadestGP, "_plan_factory", staticmethod(ch.LaplaceOraclePlan))
    monkeypatch.setattr(LoadestGP, "device", "cpu")
    return LoadestGP


def _mask(target, k=8, seed=1):
    """The k smallest-but-one values become non-detects reported at a common detection limit."""
    vals = np.asarray(target.values, dtype=np.float64)
    order = np.argsort(vals)
    mask = np.zeros(len(vals), dtype=bool)
    mask[order[:k]] = True
    reported = vals.copy()
    reported[mask] = vals[order[k]]  # the detection limit: the truth lies below it
    return type(target)(reported, dims=target.dims, coords=target.coords, name=target.name, attrs=getattr(target, "attrs", {})), mask


def _objective(model):
    from discontinuum_amd.gp.mll import ExactMarginalLogLikelihood

    with torch.no_grad():
        return float(-ExactMarginalLogLikelihood(model.likelihood, model.model)(model._prior(), model._train_y))


def test_engine_fit_with_mask_lowers_the_objective_and_predicts_the_laplace_posterior(cpu_engine):
    cov, target = loadest_dataset(40, seed=2)
    reported, mask = _mask(target)
    short, long_ = cpu_engine(), cpu_engine()
    short.fit(cov, reported, iterations=1, censored=mask)
    long_.fit(cov, reported, iterations=12, censored=mask)
    assert long_._censor is not None and long_._plan.laplace_calls >= 12
    assert _objective(long_) < _objective(short)
    it, dmax, _halvings, capped = long_.laplace_status_
    assert 1 <= it <= 30 and dmax <= long_.laplace_tol and capped == 0
    # predict: the helper's Laplace posterior at the fitted hyperparameters, in model space
    Xs = torch.tensor(long_.dm.Xnew(cov), dtype=torch.float64)
    mu, var = long_._model_space_predict(Xs)
    with torch.no_grad():
        theta = long_._theta_fn().detach()
        mean = long_.model.prior_mean(long_._train_x).numpy()
    side = np.where(mask, -1, 0)
    res = ch.laplace("loadest", long_._train_x, long_._train_y.numpy(), side, np.full(40, 0.01), mean, theta, tol=1e-12)
    ref_mu, ref_var = ch.posterior("loadest", long_._train_x, res, Xs)
    assert torch.allclose(mu, ref_mu + float(mean[0]), rtol=0, atol=1e-8)
    assert torch.allclose(var, ref_var + long_.likelihood.predictive_noise(40, Xs.device, torch.float64), rtol=0, atol=1e-8)
    # the fit differs from the one that takes the limits for samples
    plain = cpu_engine()
    plain.fit(cov, reported, iterations=12)
    assert float((plain._model_space_predict(Xs)[0] - mu).abs().max()) > 1e-3
    # products that read the held factorisation run unchanged
    se = long_.predict(cov)[1]
    assert np.all(np.isfinite(se.values))
    assert np.all(np.isfinite(long_.sample(cov, n=3).values))


def test_no_censoring_is_the_plain_fit(cpu_engine):
    cov, target = loadest_dataset(30, seed=5)
    fits = []
    for censored in (None, np.zeros(30, dtype=bool), np.zeros(30, dtype=int)):
        m = cpu_engine()
        m.fit(cov, target, iterations=6, censored=censored)
        assert m._censor is None and m.laplace_status_ is None and getattr(m._plan, "laplace_calls", 0) == 0
        fits.append(torch.cat([p.detach().reshape(-1) for p in m.model.parameters()]))
    assert torch.equal(fits[0], fits[1]) and torch.equal(fits[0], fits[2])


def test_refusals(cpu_engine, monkeypatch):
    cov, target = loadest_dataset(30, seed=4)
    reported, mask = _mask(target, k=5)
    m = cpu_engine()
    m.fit(cov, reported, iterations=2, censored=mask)
    from tests.flux_helpers import daily_loadest

    daily = daily_loadest(n_obs=30, end="2013-01-01")[-1]
    calls = {
        "cross_validate": lambda: m.cross_validate(),
        "flux_bias": lambda: m.flux_bias(),
        "influence": lambda: m.influence(cov, np.ones(30)),
        "sample_influence": lambda: m.sample_influence(daily),
        "hyperparameter_uncertainty": lambda: m.hyperparameter_uncertainty(),
        "predict_marginalized": lambda: m.predict_marginalized(cov),
        "aggregate": lambda: m.aggregate(cov, np.ones(30), hyperparameters=True),
        "annual_flux": lambda: m.annual_flux(daily, hyperparameters=True),
    }
    for name, call in calls.items():
        with pytest.raises(NotImplementedError, match="censored"):
            call()
    from discontinuum_amd.multisite_fit import fit_many, fit_many_distributed

    for fn in (fit_many, fit_many_distributed):
        with pytest.raises(NotImplementedError, match="censored"):
            fn([cpu_engine()], [(cov, reported, None, mask)])
    # learned noise (rating-gp) has no gradient here
    from discontinuum_amd.rating_gp import RatingGP

    monkeypatch.setattr(RatingGP, "_plan_factory", staticmethod(ch.LaplaceOraclePlan))
    monkeypatch.setattr(RatingGP, "device", "cpu")
    rcov, rtarget, runc = rating_dataset(30)
    with pytest.raises(NotImplementedError, match="censored"):
        RatingGP().fit(rcov, rtarget, runc, iterations=1, censored=mask)
    with pytest.raises(ValueError, match="align"):
        cpu_engine().fit(cov, reported, iterations=1, censored=mask[:-1])


def test_checkpoint_round_trips_the_mask(cpu_engine):
    cov, target = loadest_dataset(30, seed=6)
    reported, mask = _mask(target, k=6)
    m = cpu_engine()
    m.fit(cov, reported, iterations=3, censored=mask)
    buf = io.BytesIO()
    m.save(buf)
    buf.seek(0)
    back = cpu_engine.load(buf, cov, reported)
    assert back._censor is not None and back._censor.side.tolist() == np.where(mask, -1, 0).tolist()
    Xs = torch.tensor(m.dm.Xnew(cov), dtype=torch.float64)
    a, b = m._model_space_predict(Xs), back._model_space_predict(Xs)
    assert torch.allclose(a[0], b[0], rtol=0, atol=1e-9) and torch.allclose(a[1], b[1], rtol=0, atol=1e-9)
    # an explicit argument outranks the saved vector; an uncensored checkpoint stays uncensored
    buf.seek(0)
    other = np.zeros(30, dtype=int)
    other[3] = 1
    assert cpu_engine.load(buf, cov, reported, censored=other)._censor.side.tolist() == other.tolist()
    plain = cpu_engine()
    plain.fit(cov, target, iterations=2)
    buf2 = io.BytesIO()
    plain.save(buf2)
    buf2.seek(0)
    assert cpu_engine.load(buf2, cov, target)._censor is None


def test_abi_declares_the_censored_entries():
    lib = _lib.load()
    for name in ("dgp_laplace_fit_step", "dgp_laplace_factorize", "dgp_laplace_workspace_bytes", "dgp_debug_censored_terms",
                 "dgp_debug_bilinear"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.E_NOCONV == -6
    # argument validation before any launch, without a device
    import ctypes as C

    h64, h32 = C.c_void_p(), C.c_void_p()
    assert lib.dgp_plan_create(_lib.MODEL_LOADEST, _lib.F64, 100, 2, C.byref(h64)) == 0
    assert lib.dgp_plan_create(_lib.MODEL_LOADEST, _lib.F32, 100, 2, C.byref(h32)) == 0
    assert lib.dgp_laplace_workspace_bytes(h64) > 13 * 128 * 8 and lib.dgp_laplace_workspace_bytes(h32) == 0
    stat = (C.c_double * 4)()
    theta = (C.c_double * 9)(*([LN2] * 9))
    one = C.c_void_p(256)  # never dereferenced: every call below fails before a launch
    assert lib.dgp_laplace_fit_step(h32, theta, one, one, one, one, one, 5, 1e-10, one, 1 << 20, one, one, stat, None) == -1
    assert b"float64" in lib.dgp_last_error()
    assert lib.dgp_laplace_fit_step(h64, theta, one, one, one, one, None, 5, 1e-10, one, 1 << 20, one, one, stat, None) == -1
    assert b"f_dev" in lib.dgp_last_error()
    assert lib.dgp_laplace_factorize(h64, theta, one, one, one, one, one, 0, 1e-10, one, 1 << 20, one, stat, None) == -1
    assert lib.dgp_laplace_fit_step(h64, theta, one, one, one, one, one, 5, 1e-10, one, 1 << 20, one, one, stat, None) == -3  # no workspace
    assert lib.dgp_debug_censored_terms(None, 4, one, None) == -1
    assert lib.dgp_plan_set_batch(h64, 4) == 0
    assert lib.dgp_laplace_factorize(h64, theta, one, one, one, one, one, 5, 1e-10, one, 1 << 20, one, stat, None) == -1
    assert b"batched" in lib.dgp_last_error()
    assert lib.dgp_plan_destroy(h64) == 0 and lib.dgp_plan_destroy(h32) == 0
