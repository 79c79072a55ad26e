"""Posterior decomposition into the covariance's additive parts (``MarginalHIP.decompose``, ``components``) on CPU: the host
logic -- names, the deterministic ``mean`` component, scaling, merging from the packed covariance, the lognormal factors --
with the device plan replaced by an oracle-backed double whose parts come from the oracle's own Gram with the other
outputscales zeroed (tests/terms_helpers.py); and the new C entries' queries and argument checks without a device."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.stats import norm

from discontinuum_amd import _lib
from discontinuum_amd.components import merge_matrix, unpack_cov
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.loads import target_transform
from discontinuum_amd.rating_gp import RatingGP
from oracle import gp_oracle as orc
from tests.helpers import loadest_dataset, rating_dataset
from tests.terms_helpers import NAMES, TermsOraclePlan, model_reference, outputscale_indices, pack_cov, terms_reference
from tests.test_gpu_stages import make_case


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(TermsOraclePlan))
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


@pytest.mark.parametrize("model,d,n", [("loadest", 3, 300), ("loadest", 3, 1000), ("rating", 2, 300), ("rating", 2, 1000)])
def test_reference_parts_sum_to_the_oracle_posterior(model, d, n):
    """The construction every bound rests on: the parts' means sum to ``orc.posterior``'s mean and their C x C covariance to
    its variance (measured: <= 1.3e-13 of max |mean|, <= 6e-15 of the prior variance)."""
    X, r, noise, theta = make_case(model, d, n, seed=1, perturb=0.3)
    Xs = make_case(model, d, 200, seed=8)[0]
    mean, cov, scale = terms_reference(orc.GRAMS[model], outputscale_indices(model, d), X, r, noise, theta, Xs)
    mu, var = orc.posterior(model, X, r, noise, theta, Xs)
    assert mean.shape == (len(NAMES[model]), 200) and cov.shape == (len(NAMES[model]),) * 2 + (200,)
    e_m = ((mean.sum(0) - mu).abs().max() / mu.abs().max().clamp(min=1.0)).item()
    e_v = ((cov.sum((0, 1)) - var).abs().max() / scale).item()
    print(f"reference sums {model} n={n}: mean {e_m:.2e} var {e_v:.2e}")
    assert e_m < 1e-12 and e_v < 1e-13
    assert torch.equal(cov, cov.transpose(0, 1))


def test_nterms_query_without_a_device():
    lib = _lib.load()
    assert lib.dgp_model_nterms(_lib.MODEL_LOADEST, 3) == 3 and lib.dgp_model_nterms(_lib.MODEL_LOADEST, 6) == 3
    assert lib.dgp_model_nterms(_lib.MODEL_RATING, 2) == 5
    assert lib.dgp_model_nterms(_lib.MODEL_LOADEST, 1) < 0 and lib.dgp_model_nterms(_lib.MODEL_LOADEST, 7) < 0
    assert lib.dgp_model_nterms(_lib.MODEL_RATING, 3) < 0
    assert lib.dgp_model_nterms(7, 2) < 0 and lib.dgp_model_nterms(-1, 2) < 0
    spec = [2, 2, 1, 1, 0, 0, 0, 1, 0, 0, 2, 1, 3, 0, 1, 1, 0, 0, 0, 1, 1]  # rbf(0) + unscaled matern32(1) * rbf(1)
    arr, mid = (C.c_int * len(spec))(*spec), C.c_int()
    assert lib.dgp_composite_define(arr, len(spec), C.byref(mid)) == 0
    assert lib.dgp_model_nterms(mid.value, 2) == 2 and lib.dgp_model_nterms(mid.value, 3) < 0


def test_predict_terms_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.dgp_plan_create(_lib.MODEL_RATING, _lib.F64, 1000, 2, C.byref(h)) == 0
    N, M = lib.dgp_padded_n(1000), lib.dgp_padded_n(300)
    assert lib.dgp_predict_terms_workspace_bytes(None, 300) == 0
    assert lib.dgp_predict_terms_workspace_bytes(h, 0) == 0 and lib.dgp_predict_terms_workspace_bytes(h, -5) == 0
    need = lib.dgp_predict_terms_workspace_bytes(h, 300)
    assert need >= 8 * (2 * 5 * N * M + 5 * M)  # the five cross Grams and V, side by side
    assert need > 4 * lib.dgp_predict_workspace_bytes(h, 300)
    p = C.c_void_p(256)  # never dereferenced: every call below fails its host-side checks
    th = (C.c_double * 16)(*([1.0] * 16))
    assert lib.dgp_predict_terms(None, th, p, 300, p, need, p, p, None) == -1 and b"null plan" in lib.dgp_last_error()
    assert lib.dgp_predict_terms(h, None, p, 300, p, need, p, p, None) == -1
    assert lib.dgp_predict_terms(h, th, None, 300, p, need, p, p, None) == -1
    assert lib.dgp_predict_terms(h, th, p, 300, None, need, p, p, None) == -1
    assert lib.dgp_predict_terms(h, th, p, 300, p, need, None, p, None) == -1
    assert lib.dgp_predict_terms(h, th, p, 0, p, need, p, p, None) == -1 and b"m <= 0" in lib.dgp_last_error()
    assert lib.dgp_predict_terms(h, th, p, -3, p, need, p, None, None) == -1
    assert lib.dgp_predict_terms(h, th, p, 300, p, need, p, None, None) == -3 and b"workspace" in lib.dgp_last_error()  # none yet
    assert lib.dgp_plan_destroy(h) == 0


def test_merge_matrix_and_unpack():
    names = NAMES["rating"]
    merged, G = merge_matrix(names, None)
    assert merged == names and np.array_equal(G, np.eye(5))
    merged, G = merge_matrix(names, {"shift": ("shift_1", "shift_2")})
    assert merged == ("shift", "bend", "base", "periodic")
    assert G.tolist() == [[1, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 1, 0], [0, 0, 0, 0, 1]]
    merged, G = merge_matrix(names, {"stable": ("base", "bend"), "moving": ("periodic", "shift_2", "shift_1")})
    assert merged == ("moving", "stable") and G.tolist() == [[1, 1, 0, 0, 1], [0, 0, 1, 1, 0]]
    merged, _ = merge_matrix(names, {"base": ("base", "bend")})  # a group may take a member's name
    assert merged == ("shift_1", "shift_2", "base", "periodic")
    for bad in ({"a": ("shift_1", "nope")}, {"a": ("base",), "b": ("base",)}, {"a": ("bend", "bend")}, {"mean": ("base",)},
                {"base": ("bend",)}, {"a": ()}):
        with pytest.raises(ValueError):
            merge_matrix(names, bad)
    cov = torch.randn(3, 3, 7, dtype=torch.float64)
    cov = cov + cov.transpose(0, 1)
    assert np.array_equal(unpack_cov(pack_cov(cov).numpy()), cov.numpy())
    with pytest.raises(ValueError):
        unpack_cov(np.zeros((4, 2)))


@pytest.mark.parametrize("kind", ["loadest", "rating"])
def test_decompose_names_mean_component_and_sums(kind):
    model, covariates = _fitted(kind)
    names = NAMES[kind]
    assert type(model).component_names == names
    ds = model.decompose(covariates, return_cov=True)
    time = np.asarray(covariates.coords["time"].values)
    assert list(ds.coords["component"].values) == list(names) + ["mean"]
    assert list(ds.coords["component_2"].values) == list(names) + ["mean"]
    assert np.array_equal(ds.coords["time"].values, time)
    C, m = len(names), len(time)
    mean, se, cov = (np.asarray(ds[k].values) for k in ("mean", "se", "cov"))
    assert mean.shape == (C + 1, m) and se.shape == (C + 1, m) and cov.shape == (C + 1, C + 1, m)
    mode, s, t = target_transform(model.dm)
    Xnew = torch.tensor(model.dm.Xnew(covariates), dtype=torch.float64)
    ref_mean, ref_cov, _scale = model_reference(model, Xnew)
    scale = max(1.0, float(np.abs(ref_mean.numpy()).max()))
    assert np.abs(mean[:C] - s * ref_mean.numpy()).max() <= 1e-10 * abs(s) * scale
    assert np.abs(cov[:C, :C] - s * s * ref_cov.numpy()).max() <= 1e-10 * s * s
    # the deterministic component: the prior mean function through the target scaler, no uncertainty
    with torch.no_grad():
        prior = model.model.prior_mean(Xnew).numpy().reshape(-1) * np.ones(m)
    assert np.allclose(mean[C], s * prior + t, rtol=0, atol=1e-12) and np.all(se[C] == 0.0)
    assert np.all(cov[C] == 0.0) and np.all(cov[:, C] == 0.0)
    assert np.all(se >= 0.0) and np.allclose(se[:C] ** 2, np.einsum("aam->am", cov[:C, :C]).clip(0), rtol=1e-12, atol=0)
    # the components add up to the transformed prediction
    target, _se = model.predict(covariates)
    predicted = np.asarray(target.values, dtype=np.float64).reshape(-1)
    total = mean.sum(0)
    if mode == 1:
        assert np.abs(total - np.log(predicted)).max() < 1e-10
        z = norm.ppf(0.975)
        f, lo, hi = (np.asarray(ds[k].values) for k in ("factor", "factor_lower", "factor_upper"))
        assert np.all(lo <= f) and np.all(f <= hi)
        assert np.allclose(f, np.exp(mean), rtol=1e-14) and np.allclose(lo, np.exp(mean - z * se), rtol=1e-14)
        assert np.allclose(hi, np.exp(mean + z * se), rtol=1e-14) and np.array_equal(lo[C], hi[C])
        assert np.allclose(np.prod(f, axis=0), predicted, rtol=1e-9)
        narrow = model.decompose(covariates, ci=0.5)
        assert np.all(narrow["factor_upper"].values[:C] <= hi[:C]) and np.all(narrow["factor_lower"].values[:C] >= lo[:C])
    else:
        assert np.abs(total - predicted).max() < 1e-10 * max(1.0, np.abs(predicted).max())
        assert "factor" not in ds
    assert "cov" not in model.decompose(covariates)


@pytest.mark.parametrize("kind", ["loadest", "rating"])
def test_groups_merge_from_the_full_covariance(kind):
    model, covariates = _fitted(kind)
    names = NAMES[kind]
    C = len(names)
    full = model.decompose(covariates, return_cov=True)
    mean, cov = np.asarray(full["mean"].values), np.asarray(full["cov"].values)
    pair = names[:2]
    ds = model.decompose(covariates, groups={"both": pair}, return_cov=True)
    assert list(ds.coords["component"].values) == ["both"] + list(names[2:]) + ["mean"]
    assert np.allclose(ds["mean"].values[0], mean[0] + mean[1], rtol=0, atol=1e-13)
    var = cov[0, 0] + cov[1, 1] + 2 * cov[0, 1]
    assert np.allclose(ds["se"].values[0] ** 2, var.clip(0), rtol=1e-10, atol=1e-18)
    assert np.allclose(ds["mean"].values[1:], mean[2:], rtol=0, atol=0) and np.allclose(ds["se"].values[1:], full["se"].values[2:])
    assert np.allclose(ds["cov"].values[0, 1], cov[0, 2] + cov[1, 2], rtol=1e-12, atol=1e-18)
    # the parts are correlated a posteriori: the merged variance is not the sum of the members' variances
    assert np.abs(cov[0, 1]).max() > 0
    # everything merged reproduces predict's model-space posterior
    one = model.decompose(covariates, groups={"all": names})
    assert list(one.coords["component"].values) == ["all", "mean"]
    _mode, s, t = target_transform(model.dm)
    Xnew = torch.tensor(model.dm.Xnew(covariates), dtype=torch.float64)
    mu, v = model._model_space_predict(Xnew)
    with torch.no_grad():
        latent = v - model.likelihood.predictive_noise(Xnew.shape[0], Xnew.device, torch.float64)
    assert np.allclose(one["se"].values[0] ** 2, s * s * latent.numpy(), rtol=1e-8, atol=1e-12 * s * s)
    assert np.allclose(one["mean"].values.sum(0), s * mu.numpy() + t, rtol=0, atol=1e-10)
    if kind == "rating":
        shift = model.decompose(covariates, groups={"shift": ("shift_1", "shift_2")})
        assert list(shift.coords["component"].values) == ["shift", "bend", "base", "periodic", "mean"]


def test_decompose_error_cases():
    model, covariates = _fitted("loadest")
    for bad in ({"x": ("seasonal", "trend")}, {"x": ("seasonal",), "y": ("seasonal",)}, {"mean": ("residual",)}):
        with pytest.raises(ValueError):
            model.decompose(covariates, groups=bad)
    for ci in (0.0, 1.0, -0.2):
        with pytest.raises(ValueError):
            model.decompose(covariates, ci=ci)
    with pytest.raises(RuntimeError, match="hasn't been fitted"):
        LoadestGP().decompose(covariates)
    model.dm.target_pipeline.steps = [(name, step) for name, step in model.dm.target_pipeline.steps if name != "scaler"]
    with pytest.raises(NotImplementedError):
        model.decompose(covariates)
