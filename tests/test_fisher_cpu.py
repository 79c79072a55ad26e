"""Host half of the hyperparameter-uncertainty product (``discontinuum_amd/hyperpar.py``) without a GPU: the engine runs on
``FisherOraclePlan`` (dense, through the oracle), and everything is checked against F_raw built entirely from the model
oracles -- forward-mode derivatives of raw -> (K^, mu), then 1/2 tr(S d_a K^ S d_b K^) + d_a mu^T S d_b mu.  Also: the
Fisher matrix IS the covariance of the gradient under the model (Monte Carlo), and the C ABI of ``dgp_fisher``."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from discontinuum_amd import hyperpar as hp
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.rating_gp import RatingGP
from oracle import gp_oracle as orc
from tests.fisher_helpers import (FisherOraclePlan, dense_fisher, fisher_from_directions, gram_directions, oracle_information,
                                  oracle_prior_hessian, oracle_view, scaled_error)
from tests.helpers import loadest_dataset, rating_dataset
from tests.test_gpu_stages import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(FisherOraclePlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)


def fitted(kind, n=None, iterations=8):
    if kind == "loadest":
        covariates, target = loadest_dataset(n=n or 40, seed=1)
        model = LoadestGP()
        model.fit(covariates, target, iterations=iterations)
    else:
        covariates, target, unc = rating_dataset(n=n or 36, seed=2)
        model = RatingGP()
        model.fit(covariates, target, target_unc=unc, iterations=iterations)
    return model


@pytest.mark.parametrize("kind", ["loadest", "rating"])
def test_host_algebra_against_the_oracle_route(kind, cpu_engine):
    engine = fitted(kind)
    ds = engine.hyperparameter_uncertainty(ci=0.9, prior=True)
    o, raw, perm, X, fixed = oracle_view(engine, kind)
    F_ref = oracle_information(o, kind, raw, X, fixed)[perm][:, perm]
    F = torch.as_tensor(ds["information"].values)
    assert bool(np.all(ds["active"].values))
    assert scaled_error(F, F_ref) <= 1e-10
    H_ref = oracle_prior_hessian(o, kind, raw)[perm][:, perm]
    H = hp.prior_hessian(engine)
    assert (H - H_ref).abs().max() <= 1e-10 * max(1.0, H_ref.abs().max().item())
    cov_ref = torch.linalg.inv(F_ref + H_ref)
    cov = torch.as_tensor(ds["cov_raw"].values)
    assert ds.attrs["positive_definite"] and ds.attrs["n_eff"] == raw.numel() and ds["unidentified"].values.shape[0] == 0
    assert ((cov - cov_ref).abs().max() / cov_ref.abs().max()).item() <= 1e-6
    se_raw = ds["se_raw"].values
    assert np.allclose(se_raw, np.sqrt(np.diag(cov_ref.numpy())), rtol=1e-6)
    assert np.allclose(np.diag(ds["corr"].values), 1.0)
    # estimate / se / interval: the constraint of every leaf, by the oracle's transforms
    z = 1.6448536269514722  # Phi^-1(0.95)
    flat = raw[perm]
    if kind == "loadest":
        f = [lambda v: v] + [orc.positive] * (flat.numel() - 1)
        bounds = [(-np.inf, np.inf)] + [(0.0, np.inf)] * (flat.numel() - 1)
    else:
        gate = lambda v: orc.interval(v, o.b_lo, o.b_hi)  # noqa: E731
        f = [lambda v: orc.greater_than(v, 1e-4)] + [lambda v: v] * 3 + [gate] + [orc.positive] * 15
        bounds = [(1e-4, np.inf)] + [(-np.inf, np.inf)] * 3 + [(o.b_lo, o.b_hi)] + [(0.0, np.inf)] * 15
    for k in range(flat.numel()):
        v = flat[k].clone().requires_grad_(True)
        (g,) = torch.autograd.grad(f[k](v), v)
        s = torch.as_tensor(se_raw[k])
        est, lo, up = ds["estimate"].values[k], ds["lower"].values[k], ds["upper"].values[k]
        assert abs(est - f[k](flat[k]).item()) <= 1e-12 * max(1.0, abs(est))
        assert abs(ds["se"].values[k] - abs(g.item()) * se_raw[k]) <= 1e-10 * max(1.0, ds["se"].values[k])
        assert abs(lo - f[k](flat[k] - z * s).item()) <= 1e-9 * max(1.0, abs(lo))
        assert abs(up - f[k](flat[k] + z * s).item()) <= 1e-9 * max(1.0, abs(up))
        assert bounds[k][0] <= lo < est < up <= bounds[k][1]
    # without the prior: the same information, the inverse of F alone
    ds0 = engine.hyperparameter_uncertainty(prior=False)
    assert np.array_equal(ds0["information"].values, ds["information"].values)
    if ds0.attrs["positive_definite"]:
        c0 = torch.linalg.inv(F_ref)
        assert ((torch.as_tensor(ds0["cov_raw"].values) - c0).abs().max() / c0.abs().max()).item() <= 1e-5


def test_a_parameter_on_its_clamp_is_inactive(cpu_engine):
    engine = fitted("rating")
    with torch.no_grad():
        engine.model.powerlaw.b.fill_(2.5)
    ds = engine.hyperparameter_uncertainty(prior=False)
    names = list(ds["parameter"].values)
    k = names.index("powerlaw.b")
    active = ds["active"].values
    assert not active[k] and active.sum() == len(names) - 1
    for key in ("se", "se_raw", "lower", "upper"):
        assert np.isnan(ds[key].values[k]) and np.all(np.isfinite(np.delete(ds[key].values, k)))
    assert ds["estimate"].values[k] == 2.5
    info = ds["information"].values
    assert np.all(info[k] == 0.0) and np.all(info[:, k] == 0.0)
    o, raw, perm, X, fixed = oracle_view(engine, "rating")
    F_ref = oracle_information(o, "rating", raw, X, fixed)[perm][:, perm]
    keep = [i for i in range(len(names)) if i != k]
    assert scaled_error(torch.as_tensor(info)[keep][:, keep], F_ref[keep][:, keep]) <= 1e-10
    cov = ds["cov_raw"].values
    assert np.all(np.isnan(cov[k])) and np.all(np.isfinite(cov[np.ix_(keep, keep)]))
    assert ds.attrs["n_eff"] == len(names) - 1 - ds["unidentified"].values.shape[0]
    # c on ITS clamp (the smallest training stage) as well
    with torch.no_grad():
        engine.model.powerlaw.c.fill_(1e9)
    ds2 = engine.hyperparameter_uncertainty(prior=True)
    assert not ds2["active"].values[names.index("powerlaw.c")] and not ds2["active"].values[k]
    assert ds2["active"].values.sum() == len(names) - 2


def test_a_duplicated_direction_is_reported_not_inverted():
    """Two equal diagonal directions: the information is singular along their difference."""
    model, d, n = "loadest", 2, 50
    X, r, noise, theta = make_case(model, d, n, seed=2, perturb=0.2)
    ones = torch.ones(2, n, dtype=torch.float64)
    F_dev = dense_fisher(model, X, noise, theta, ones).numpy()
    R = F_dev.shape[0]
    F_raw, active = hp.assemble(F_dev, np.eye(R), np.zeros((n, R)), np.zeros(R, dtype=bool))
    assert active.all() and np.allclose(F_raw, F_dev)
    cov, unident, lam_min, pd = hp.invert_information(F_raw, active)
    assert not pd and unident.shape == (1, R) and abs(lam_min) < 1e-10
    u = unident[0]
    assert np.allclose(np.abs(u[-2:]), np.sqrt(0.5), atol=1e-6) and u[-1] * u[-2] < 0 and np.abs(u[:-2]).max() < 1e-6
    assert np.all(np.isfinite(cov))
    assert np.abs(F_raw @ cov @ F_raw - F_raw).max() <= 1e-8 * np.abs(F_raw).max()  # a pseudo-inverse
    assert np.abs(cov @ unident[0] * np.sqrt(np.diag(F_raw))).max() < 1e-6 * np.abs(cov).max()
    # all rows inactive: nothing to invert, nothing raised
    cov0, un0, _lam, pd0 = hp.invert_information(F_raw, np.zeros(R, dtype=bool))
    assert np.all(np.isnan(cov0)) and un0.shape[0] == 0 and not pd0


def test_fisher_is_the_covariance_of_the_gradient():
    """20 000 seeded draws y ~ N(m, K^) at n = 60 (loadest): the sample covariance of the analytic theta-gradient of the NLL
    agrees with F entrywise within 5 Monte Carlo standard errors, the standard errors from the draws' own fourth moments."""
    model, d, n, draws = "loadest", 2, 60, 20000
    X, r, noise, theta = make_case(model, d, n, seed=5, perturb=0.3)
    Khat = orc.GRAMS[model](X, X, theta) + torch.diag(noise)
    dirs = gram_directions(model, X, theta)
    F = fisher_from_directions(Khat, dirs)
    S = torch.linalg.inv(Khat)
    L = torch.linalg.cholesky(Khat)
    Z = torch.randn(n, draws, dtype=torch.float64, generator=torch.Generator().manual_seed(11))
    A = S @ (L @ Z)  # alpha of every draw (residuals r = L z)
    G = torch.stack([0.5 * (S * D).sum() - 0.5 * (A * (D @ A)).sum(0) for D in dirs])  # (P, draws)
    _, g_ref, _, _ = orc.nll_data_and_grads(model, X, (L @ Z)[:, 0], noise, theta)  # the oracle's own gradient, one draw
    assert (G[:, 0] - g_ref).abs().max() <= 1e-9 * g_ref.abs().max()
    Gc = G - G.mean(1, keepdim=True)
    prod = Gc[:, None, :] * Gc[None, :, :]
    C_hat = prod.mean(-1)
    se = (prod.var(-1, unbiased=True) / draws).sqrt()
    worst = ((C_hat - F).abs() / se).max().item()
    ratio = torch.diagonal(C_hat) / torch.diagonal(F)
    print(f"gradient covariance vs Fisher: worst deviation {worst:.2f} standard errors, diagonal ratios {ratio.min():.3f} .. {ratio.max():.3f}")
    assert worst <= 5.0
    assert (G.mean(1).abs() <= 5.0 * G.std(1) / np.sqrt(draws)).all()  # the score has mean zero


def test_abi_of_dgp_fisher():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "dgp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\b(dgp_fisher\w*)\s*\(([^;]*?)\)\s*;", text)}
    assert decl["dgp_fisher_workspace_bytes"] == "const dgp_plan* plan, int ndiag"
    assert decl["dgp_fisher"] == ("dgp_plan* plan, const double* theta_host, const void* diag_dev, int ndiag, void* work_dev, "
                                  "size_t work_bytes, double* fisher_dev, void* stream")
    vp, i, sz, dp = C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_double)
    assert _lib.SIGNATURES["dgp_fisher_workspace_bytes"] == (sz, [vp, i])
    assert _lib.SIGNATURES["dgp_fisher"] == (i, [vp, dp, vp, i, vp, sz, vp, vp])
    assert hasattr(lib, "dgp_fisher") and hasattr(lib, "dgp_fisher_workspace_bytes")
    # queries and argument checks need no device
    h = C.c_void_p()
    assert lib.dgp_plan_create(_lib.MODEL_RATING, _lib.F32, 300, 2, C.byref(h)) == 0
    N, P = 384, 16
    tiles = (N // 64) * (N // 64 + 1) // 2
    for E in (0, 1, 8):
        nd = P + E
        assert lib.dgp_fisher_workspace_bytes(h, E) == (nd + 1) * N * N * 4 + (tiles * nd * nd * 8 + 255) // 256 * 256
    assert lib.dgp_fisher_workspace_bytes(h, 9) == 0 and lib.dgp_fisher_workspace_bytes(h, -1) == 0
    assert lib.dgp_fisher_workspace_bytes(None, 0) == 0
    theta = (C.c_double * P)(*([1.0] * P))
    fake = C.c_void_p(256)  # never dereferenced: every call below fails its checks first
    assert lib.dgp_fisher(None, theta, None, 0, fake, 1 << 40, fake, None) == -1
    assert lib.dgp_fisher(h, None, None, 0, fake, 1 << 40, fake, None) == -1
    assert lib.dgp_fisher(h, theta, None, 0, fake, 1 << 40, None, None) == -1
    assert lib.dgp_fisher(h, theta, fake, 9, fake, 1 << 40, fake, None) == -1 and b"ndiag" in lib.dgp_last_error()
    assert lib.dgp_fisher(h, theta, None, 1, fake, 1 << 40, fake, None) == -1
    assert lib.dgp_fisher(h, theta, None, 0, fake, 1 << 40, fake, None) == -3  # a plan without workspace
    assert lib.dgp_plan_destroy(h) == 0


def test_many_sites_through_one_batched_plan(cpu_engine, monkeypatch):
    """``hyperparameter_uncertainty_many``: one ragged batched plan for all sites gives what every engine gives alone."""
    from discontinuum_amd import multisite_fit

    monkeypatch.setattr(multisite_fit, "GPPlan", FisherOraclePlan)
    engines = [fitted("rating", n=30, iterations=3), fitted("rating", n=36, iterations=4)]
    many = multisite_fit.hyperparameter_uncertainty_many(engines, ci=0.9, prior=True)
    for engine, ds in zip(engines, many):
        alone = engine.hyperparameter_uncertainty(ci=0.9, prior=True)
        assert list(ds["parameter"].values) == list(alone["parameter"].values)
        for key in ("information", "cov_raw", "estimate", "se", "lower", "upper"):
            a, b = np.asarray(ds[key].values), np.asarray(alone[key].values)
            assert np.allclose(a, b, rtol=1e-9, atol=1e-12 * np.abs(b).max()), key
        assert ds.attrs["n_eff"] == alone.attrs["n_eff"]
    with pytest.raises(ValueError):
        multisite_fit.hyperparameter_uncertainty_many([])
    with pytest.raises(ValueError):
        multisite_fit.hyperparameter_uncertainty_many([engines[0], fitted("loadest", n=30, iterations=2)])
