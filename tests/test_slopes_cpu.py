"""Posterior slopes (``MarginalHIP.slope``, ``RatingGP.rating_exponent``, ``discontinuum_amd.slopes``) on CPU: the closed-form
prior block of tests/slopes_helpers.py against autograd just off the diagonal; the host logic -- chain rule through the
covariate pipelines, target scale, the prior mean's derivative, intervals -- with the device plan replaced by an
oracle-backed double, against central differences of the same double's ``predict`` in COVARIATE space; and the new C entries'
queries and argument checks without a device."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.stats import norm

from discontinuum_amd import _lib
from discontinuum_amd import pipeline as pl
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.loads import target_transform
from discontinuum_amd.rating_gp import RatingGP
from discontinuum_amd.xr_compat import Dataset
from oracle import gp_oracle as orc
from tests.helpers import loadest_dataset, rating_dataset
from tests.slopes_helpers import (PRIORS, SlopesOraclePlan, autograd_prior_block, composite_prior, cross_planes,
                                  model_reference, shifted)
from tests.test_gpu_stages import make_case

# rbf(0) + matern12(1): column 1 is not differentiable;  periodic(0) x matern52(0) + unscaled matern32(0, 1 ARD) x rbf(1)
SPEC_M12 = [2, 2, 1, 1, 0, 0, 0, 1, 0, 1, 1, 1, 1, 0, 1, 1]
SPEC_PER = [2, 2, 1, 2, 2, 0, 0, 1, 0, 1, 5, 0, 1, 0, 0, 2, 1, 3, 1, 2, 0, 1, 0, 0, 0, 1, 1]


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(SlopesOraclePlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)


def _fitted(kind):
    if kind == "loadest":
        covariates, target = loadest_dataset(n=40, seed=1)
        model = LoadestGP()
        model.fit(covariates, target, iterations=8)
    else:
        covariates, target, unc = rating_dataset(n=36, seed=2)
        model = RatingGP()
        model.fit(covariates, target, target_unc=unc, iterations=8)
    return model, covariates


def _define(spec):
    lib = _lib.load()
    arr, mid = (C.c_int * len(spec))(*spec), C.c_int()
    assert lib.dgp_composite_define(arr, len(spec), C.byref(mid)) == 0
    return mid.value


def _prior_cases():
    cases = []
    for model, d in (("loadest", 2), ("loadest", 3), ("rating", 2)):
        _X, _r, _noise, theta = make_case(model, d, 10, seed=1, perturb=0.3)
        Xs = make_case(model, d, 25, seed=8)[0]
        ls = {"loadest": lambda c, th=theta, d=d: min(float(th[3]), float(th[1]), float(th[5 + d])) if c == 0
              else min(float(th[4 + c]), float(th[5 + d + c])),
              "rating": lambda c, th=theta: min(float(th[i]) for i in ((3, 6, 9, 13, 15) if c == 0 else (2, 5, 8, 11)))}[model]
        cases.append((f"{model} d={d}", orc.GRAMS[model], PRIORS[model], theta, Xs, ls))
    theta = torch.tensor([0.8, 1.3, 0.9, 0.7, 1.1, 0.6, 1.7], dtype=torch.float64)
    Xs = torch.tensor(np.random.default_rng(3).standard_normal((25, 2)))
    cases.append(("composite periodic + unscaled", orc.composite_gram(SPEC_PER), composite_prior(SPEC_PER), theta, Xs,
                  lambda c: 0.5))
    return cases


@pytest.mark.parametrize("case", _prior_cases(), ids=lambda c: c[0])
def test_closed_form_prior_block_against_autograd_off_the_diagonal(case):
    """D_a D'_b k(x, x') at x = x' (closed form, slopes_helpers) against autograd's k, d_x k, d_x' k, d_x d_x' k at
    x' = x + eps e_c, eps = 1e-7 of the column's (smallest) lengthscale, for every column c: 1e-5 of the prior scale
    sqrt(prior_aa prior_bb) (the truncation is first order in eps / l for the Matern-3/2 parts, ~4e-7).  An offset along e_c
    leaves the oracle's distance clamp ACTIVE in the factors that do not see column c (loadest's time-only seasonal part
    under a flow offset), which zeroes their share of the other columns' entries: that offset checks the entries over
    (value, c); the whole block, cross-column entries included, is checked with all columns offset at once."""
    name, gram, prior_fn, theta, Xs, ls = case
    closed = prior_fn(theta, Xs)
    d = Xs.shape[1]
    diag = torch.sqrt(torch.stack([closed[a, a] for a in range(1 + d)]))
    assert bool((diag > 0).all()) and torch.equal(closed, closed.transpose(0, 1))
    rel = lambda block: (block - closed).abs() / (diag[:, None] * diag[None, :])  # noqa: E731
    worst = 0.0
    for c in range(d):
        eps = torch.zeros(d, dtype=torch.float64)
        eps[c] = 1e-7 * ls(c)
        sel = [0, 1 + c]
        worst = max(worst, rel(autograd_prior_block(gram, theta, Xs, eps))[sel][:, sel].max().item())
    everywhere = torch.tensor([1e-7 * ls(c) for c in range(d)], dtype=torch.float64)
    worst = max(worst, rel(autograd_prior_block(gram, theta, Xs, everywhere)).max().item())
    print(f"prior block {name}: closed form vs autograd off the diagonal {worst:.2e}")
    assert worst < 1e-5, worst
    if name.startswith("rating"):  # the gates correlate value and stage slope a priori; nothing else is off the diagonal
        assert closed[2, 0].abs().max() > 0 and bool((closed[1, 0] == 0).all()) and bool((closed[2, 1] == 0).all())


def test_reference_planes_vanish_at_coincident_points_and_match_differences():
    """The construction every GPU bound rests on: the autograd planes are exactly 0 at coincident pairs for the stationary
    model, and agree with central differences of the oracle's Gram (step 1e-6: < 2e-8 of the plane's largest entry)."""
    for model, d in (("loadest", 3), ("rating", 2)):
        X, _r, _noise, theta = make_case(model, d, 60, seed=1, perturb=0.3)
        Xs = make_case(model, d, 40, seed=8)[0]
        Xs[:7] = X[:7]
        planes = cross_planes(orc.GRAMS[model], X, Xs, theta, list(range(d)))
        for c in range(d):
            e = torch.zeros_like(Xs)
            e[:, c] = 1e-6
            fd = (orc.GRAMS[model](X, Xs + e, theta) - orc.GRAMS[model](X, Xs - e, theta)) / 2e-6
            off = torch.ones(60, 40, dtype=torch.bool)
            off[:7, :7] &= ~torch.eye(7, dtype=torch.bool)  # differences straddle the kink of the Matern-3/2 part there
            assert ((planes[1 + c] - fd).abs()[off].max() / planes[1 + c].abs().max()).item() < 2e-8
            if model == "loadest" or c == 0:
                assert bool((torch.diagonal(planes[1 + c][:7, :7]) == 0).all())


def test_differentiability_query_without_a_device():
    lib = _lib.load()
    q = lib.dgp_model_input_differentiable
    assert [q(_lib.MODEL_LOADEST, 3, c) for c in range(3)] == [1, 1, 1] and q(_lib.MODEL_RATING, 2, 1) == 1
    assert q(_lib.MODEL_LOADEST, 3, 3) < 0 and q(_lib.MODEL_LOADEST, 3, -1) < 0 and q(_lib.MODEL_LOADEST, 7, 0) < 0
    assert q(_lib.MODEL_RATING, 3, 0) < 0 and q(9, 2, 0) < 0
    mid = _define(SPEC_M12)
    assert q(mid, 2, 0) == 1 and q(mid, 2, 1) == 0 and q(mid, 2, 2) < 0 and q(mid, 3, 0) < 0
    per = _define(SPEC_PER)
    assert q(per, 2, 0) == 1 and q(per, 2, 1) == 1


def test_predict_slopes_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.dgp_plan_create(_lib.MODEL_LOADEST, _lib.F64, 1000, 3, C.byref(h)) == 0
    N, M = lib.dgp_padded_n(1000), lib.dgp_padded_n(300)
    wsb = lib.dgp_predict_slopes_workspace_bytes
    assert wsb(None, 300, 1) == 0 and wsb(h, 0, 1) == 0 and wsb(h, -5, 1) == 0 and wsb(h, 300, 0) == 0 and wsb(h, 300, 4) == 0
    need = wsb(h, 300, 3)
    assert need >= 8 * (2 * 4 * N * M + 10 * M) and need > wsb(h, 300, 1)
    assert wsb(h, 300, 2) >= 8 * 2 * 3 * N * M  # the same width as the three parts of dgp_predict_terms
    p = C.c_void_p(256)  # never dereferenced: every call below fails its host-side checks
    th = (C.c_double * 11)(*([1.0] * 11))
    cols = lambda *v: (C.c_int * len(v))(*v)  # noqa: E731
    call = lib.dgp_predict_slopes
    assert call(None, th, p, 300, cols(0), 1, p, need, p, p, None) == -1 and b"null plan" in lib.dgp_last_error()
    assert call(h, None, p, 300, cols(0), 1, p, need, p, p, None) == -1
    assert call(h, th, None, 300, cols(0), 1, p, need, p, p, None) == -1
    assert call(h, th, p, 300, None, 1, p, need, p, p, None) == -1
    assert call(h, th, p, 300, cols(0), 1, None, need, p, p, None) == -1
    assert call(h, th, p, 300, cols(0), 1, p, need, None, p, None) == -1
    assert call(h, th, p, 0, cols(0), 1, p, need, p, p, None) == -1 and b"m <= 0" in lib.dgp_last_error()
    assert call(h, th, p, 300, cols(0), 0, p, need, p, p, None) == -1 and b"ncols" in lib.dgp_last_error()
    assert call(h, th, p, 300, cols(0, 1, 2, 0), 4, p, need, p, p, None) == -1
    assert call(h, th, p, 300, cols(0, 3), 2, p, need, p, p, None) == -1 and b"outside" in lib.dgp_last_error()
    assert call(h, th, p, 300, cols(1, 1), 2, p, need, p, p, None) == -1 and b"repeated" in lib.dgp_last_error()
    assert call(h, th, p, 300, cols(2, 0), 2, p, need, p, None, None) == -3 and b"workspace" in lib.dgp_last_error()  # none yet
    assert lib.dgp_plan_destroy(h) == 0
    mid = _define(SPEC_M12)
    assert lib.dgp_plan_create(mid, _lib.F64, 100, 2, C.byref(h)) == 0
    assert call(h, th, p, 300, cols(1), 1, p, need, p, p, None) == -2 and b"differentiable" in lib.dgp_last_error()  # DGP_E_MODEL
    assert call(h, th, p, 300, cols(0, 1), 2, p, need, p, p, None) == -2
    assert call(h, th, p, 300, cols(0), 1, p, need, p, p, None) == -3  # the differentiable column passes on to the next check
    assert lib.dgp_plan_destroy(h) == 0


@pytest.mark.parametrize("kind", ["loadest", "rating"])
def test_slope_chain_rule_and_units_against_differences_of_predict(kind):
    """``slope`` in units of the transformed target per unit of u (ln flow, years, stage) against central differences of
    ``predict`` -- the same double, moved in covariate space -- which carry the pipelines, the target scale and the prior
    mean's derivative without any of this module's code.  Step 1e-4 (time: 1e-4 years): truncation + rounding of the
    differences stay below 1e-6 of the largest slope."""
    model, covariates = _fitted(kind)
    names = list(model.dm.covariate_pipelines)
    ds = model.slope(covariates, return_cov=True)
    m = len(covariates.coords["time"].values)
    assert list(ds.coords["wrt"].values) == names and list(ds.coords["wrt_2"].values) == names
    assert np.array_equal(ds.coords["time"].values, np.asarray(covariates.coords["time"].values))
    expect_per = ["year", "ln flow"] if kind == "loadest" else ["year", "stage"]
    assert ds.attrs["per"] == expect_per and ds["mean"].attrs["per"] == expect_per and ds.attrs["space"] == "log"
    mean, se, lower, upper, prob = (np.asarray(ds[k].values) for k in ("mean", "se", "lower", "upper", "prob_positive"))
    assert mean.shape == (len(names), m) and np.asarray(ds["cov"].values).shape == (len(names), len(names), m)
    for q, name in enumerate(names):
        step = 1e-4
        (hi, du_hi), (lo, du_lo) = shifted(covariates, name, step), shifted(covariates, name, -step)
        f_hi = np.log(np.asarray(model.predict(hi)[0].values, dtype=np.float64).reshape(-1))
        f_lo = np.log(np.asarray(model.predict(lo)[0].values, dtype=np.float64).reshape(-1))
        fd = (f_hi - f_lo) / (du_hi - du_lo)
        err = np.abs(mean[q] - fd).max() / max(1.0, np.abs(fd).max())
        print(f"slope {kind} wrt {name}: largest |slope| {np.abs(fd).max():.3g}, against differences of predict {err:.2e}")
        assert err < 1e-6, (name, err)
    # standard errors, covariances and the value-slope covariance: the reference in model space, scaled by s a
    _mode, s, _t = target_transform(model.dm)
    Xnew = torch.tensor(model.dm.Xnew(covariates), dtype=torch.float64)
    ref_mean, ref_cov, _scales = model_reference(model, Xnew, list(range(len(names))))
    a = []
    for name in names:
        scaler = dict(model.dm.covariate_pipelines[name].steps)["scaler"]
        a.append(1.0 / float(scaler.max_ - scaler.min_) if isinstance(scaler, pl.UnitScaler)
                 else (1.0 / float(np.asarray(scaler.scale_).reshape(-1)[0]) if scaler.with_std else 1.0))
    a = np.asarray(a)
    cov = np.asarray(ds["cov"].values)
    want = s * s * a[:, None, None] * a[None, :, None] * ref_cov.numpy()[1:, 1:]
    assert np.abs(cov - want).max() <= 1e-10 * np.abs(want).max()
    assert np.abs(np.asarray(ds["cov_value"].values) - s * s * a[:, None] * ref_cov.numpy()[1:, 0]).max() <= 1e-10 * s * s * a.max()
    assert np.allclose(se ** 2, np.einsum("aam->am", cov).clip(0), rtol=1e-12, atol=0) and np.all(se > 0)
    z = norm.ppf(0.975)
    assert np.allclose(lower, mean - z * se, rtol=1e-13, atol=1e-15) and np.allclose(upper, mean + z * se, rtol=1e-13, atol=1e-15)
    assert np.allclose(prob, norm.cdf(mean / se), rtol=1e-13, atol=0) and np.all((prob >= 0) & (prob <= 1))
    narrow = model.slope(covariates, wrt=names[1], ci=0.5)
    assert list(narrow.coords["wrt"].values) == [names[1]] and "cov" not in narrow
    assert np.allclose(narrow["mean"].values[0], mean[1], rtol=0, atol=1e-10 * max(1.0, np.abs(mean[1]).max()))
    assert np.all(narrow["upper"].values[0] <= upper[1]) and np.all(narrow["lower"].values[0] >= lower[1])
    swapped = model.slope(covariates, wrt=names[::-1])
    assert np.allclose(swapped["mean"].values[::-1], mean, rtol=0, atol=1e-10 * max(1.0, np.abs(mean).max()))
    if kind == "rating":
        ex = model.rating_exponent(covariates)
        h = np.asarray(covariates["stage"].values)
        assert np.allclose(ex["mean"].values, h * mean[1], rtol=1e-12) and np.allclose(ex["se"].values, h * se[1], rtol=1e-12)
        assert np.allclose(ex["prob_positive"].values, prob[1], rtol=0, atol=0)
        assert np.allclose(ex["lower"].values, h * lower[1], rtol=1e-12) and np.allclose(ex["upper"].values, h * upper[1], rtol=1e-12)
        # the synthetic rating is Q ~ h^1.6: the exponent is of that order wherever the data pin it
        assert 0.5 < np.median(ex["mean"].values) < 3.0
        # d ln Q / d ln h against differences of predict in ln h
        step = 1e-5
        data = lambda f: Dataset({"stage": ("time", h * f)}, coords={"time": np.asarray(covariates.coords["time"].values)})  # noqa: E731
        f_hi, f_lo = (np.log(np.asarray(model.predict(data(np.exp(sg * step)))[0].values, dtype=np.float64).reshape(-1))
                      for sg in (1, -1))
        assert np.abs(ex["mean"].values - (f_hi - f_lo) / (2 * step)).max() < 1e-6 * max(1.0, np.abs(ex["mean"].values).max())


def test_slope_error_cases():
    model, covariates = _fitted("loadest")
    for bad in ("stage", ["flow", "nope"], [], ["flow", "flow"]):
        with pytest.raises(ValueError):
            model.slope(covariates, wrt=bad)
    for ci in (0.0, 1.0, -0.2, 1.5):
        with pytest.raises(ValueError):
            model.slope(covariates, ci=ci)
    with pytest.raises(RuntimeError, match="hasn't been fitted"):
        LoadestGP().slope(covariates)
    with pytest.raises(RuntimeError, match="hasn't been fitted"):
        RatingGP().rating_exponent(covariates)
    # a Matern-1/2 factor on the flow column: no slope exists there
    name = model._plan.model
    model._plan.model = f"composite:{_define(SPEC_M12)}"
    with pytest.raises(ValueError, match="not differentiable"):
        model.slope(covariates, wrt="flow")
    model._plan.model = name
    # a pipeline that is not (log | decimal year) + affine
    pipe = model.dm.covariate_pipelines["flow"]
    steps = list(pipe.steps)
    pipe.steps = steps[:-1] + [("square", pl.SquareTransformer()), steps[-1]]
    with pytest.raises(NotImplementedError, match="square"):
        model.slope(covariates, wrt="flow")
    pipe.steps = steps + [("again", pl.LogTransformer())]
    with pytest.raises(NotImplementedError):
        model.slope(covariates, wrt="flow")
    pipe.steps = steps
    assert np.all(np.isfinite(model.slope(covariates, wrt="flow")["mean"].values))
    model.dm.target_pipeline.steps = [(n, st) for n, st in model.dm.target_pipeline.steps if n != "scaler"]
    with pytest.raises(NotImplementedError):
        model.slope(covariates)
