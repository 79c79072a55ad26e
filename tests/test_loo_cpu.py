"""The leave-one-out training objective without a GPU: the closed-form gradient the device code implements against autograd and
central differences, the dense restatement against brute-force deletion, and the host paths (``fit(objective="loo")``,
``fit_many(objective="loo")``, checkpoints, the censored refusal) on the oracle-backed plan double of tests/loo_helpers.py."""
import io

import numpy as np
import pytest
import torch

from discontinuum_amd import multisite_fit
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.rating_gp import RatingGP
from oracle import gp_oracle as orc
from tests.helpers import loadest_dataset, rating_dataset
from tests.loo_helpers import LooOraclePlan, brute_force_loo, closed_form, khat, loo_from_khat, loo_value_and_grads


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(LooOraclePlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    monkeypatch.setattr(multisite_fit, "GPPlan", LooOraclePlan)
    torch.manual_seed(0)


def _dense_case(n=40, seed=0):
    X, y = orc.synth_loadest(n, 3, seed)
    X, y = torch.tensor(X), torch.tensor(y)
    theta = torch.full((orc.loadest_ntheta(3),), 0.7, dtype=torch.float64) + 0.1 * torch.rand(
        orc.loadest_ntheta(3), dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    noise = 0.01 + 0.02 * torch.rand(n, dtype=torch.float64, generator=torch.Generator().manual_seed(seed + 1))
    return X, y, noise, theta


def test_closed_form_gradient_matches_autograd_and_central_differences():
    """dL/dK^ = M - 1/2 (b alpha^T + alpha b^T), dL/dr = b, dL/dnoise_i = M_ii - b_i alpha_i: the formulas of dgp_loo.hip.  Bounds:
    autograd differentiates the same fp64 expression (1e-10 of the largest entry); a central difference of step h = 1e-6 carries
    O(h^2) truncation plus eps / h rounding (1e-6 relative)."""
    X, r, noise, theta = _dense_case()
    Kh = khat("loadest", X, theta, noise).requires_grad_(True)
    rr = r.clone().requires_grad_(True)
    val = loo_from_khat(Kh, rr)
    gK, gr = torch.autograd.grad(val, (Kh, rr))
    gK = 0.5 * (gK + gK.T)
    v, M, b, alpha, _k = closed_form(Kh.detach(), r)
    assert abs(v - val.detach()) <= 1e-13 * abs(v)
    G = M - 0.5 * (torch.outer(b, alpha) + torch.outer(alpha, b))
    assert (G - gK).abs().max() <= 1e-10 * gK.abs().max()
    assert (b - gr).abs().max() <= 1e-10 * gr.abs().max()
    # through the kernel, as the device contracts it: dL/dtheta_p = sum_ij G_ij dK_ij/dtheta_p; dL/dnoise = diag G
    _val, g_theta, g_r, g_noise = loo_value_and_grads("loadest", X, r, noise, theta)
    th = theta.clone().requires_grad_(True)
    K = orc.GRAMS["loadest"](X, X, th)
    (contr,) = torch.autograd.grad((K * G).sum(), th)
    assert (contr - g_theta).abs().max() <= 1e-10 * g_theta.abs().max()
    assert (torch.diagonal(G) - g_noise).abs().max() <= 1e-10 * g_noise.abs().max()
    h = 1e-6
    for p in range(theta.numel()):
        e = torch.zeros_like(theta)
        e[p] = h
        fd = (loo_from_khat(khat("loadest", X, theta + e, noise), r) - loo_from_khat(khat("loadest", X, theta - e, noise), r)) / (2 * h)
        assert abs(fd - contr[p]) <= 1e-6 * max(1.0, contr.abs().max().item()), (p, fd, contr[p])
    for i in (0, 7, 39):
        e = torch.zeros_like(r)
        e[i] = h
        fd = (loo_from_khat(Kh.detach(), r + e) - loo_from_khat(Kh.detach(), r - e)) / (2 * h)
        assert abs(fd - b[i]) <= 1e-6 * b.abs().max()
        fd = (loo_from_khat(khat("loadest", X, theta, noise + e), r) - loo_from_khat(khat("loadest", X, theta, noise - e), r)) / (2 * h)
        assert abs(fd - G[i, i]) <= 1e-6 * torch.diagonal(G).abs().max()


def test_restatement_matches_brute_force_deletion():
    X, r, noise, theta = _dense_case(n=12, seed=3)
    Kh = khat("loadest", X, theta, noise)
    a, b = loo_from_khat(Kh, r), brute_force_loo(Kh, r)
    assert abs(a - b) <= 1e-11 * abs(b)


def _fit(family, objective, explicit, iterations, monkeypatch, **kw):
    monkeypatch.setattr(MarginalHIP, "explicit_host_algebra", explicit)
    torch.manual_seed(123)
    trace = []
    if family == "loadest":
        cov, tgt = loadest_dataset(45, seed=4)
        m = LoadestGP()
        args = dict(covariates=cov, target=tgt)
    else:
        cov, tgt, unc = rating_dataset(40, seed=4)
        m = RatingGP()
        args = dict(covariates=cov, target=tgt, target_unc=unc, monotonic_penalty_weight=0.5, grid_size=16)
    import tqdm

    real = tqdm.std.tqdm.set_postfix_str

    def spy(self, s="", refresh=True):
        trace.append(float(s.split("obj=")[1].split(",")[0]))
        return real(self, s, refresh)

    monkeypatch.setattr(tqdm.std.tqdm, "set_postfix_str", spy)
    if objective == "default":
        m.fit(iterations=iterations, learning_rate=0.1, scheduler=False, **args, **kw)
    else:
        m.fit(iterations=iterations, learning_rate=0.1, scheduler=False, objective=objective, **args, **kw)
    return m, trace


@pytest.mark.parametrize("family", ["loadest", "rating"])
def test_engine_fit_on_the_double(family, monkeypatch):
    """``fit(objective="loo")`` decreases its objective; the closed-form and the autograd host paths agree to 1e-12 over 20
    iterations (the same arithmetic in a different order); the default and "mll" never touch ``loo_fit_step``."""
    torch.manual_seed(5)  # the penalty grids of rating-gp draw from the global generator
    ma, ta = _fit(family, "loo", True, 20, monkeypatch)
    assert ma.objective_ == "loo" and ma._plan.loo_calls >= 20 and ma._plan.calls == 0
    assert ta[-1] < ta[0]
    torch.manual_seed(5)
    mb, _tb = _fit(family, "loo", False, 20, monkeypatch)
    pa = torch.cat([p.detach().reshape(-1) for p in ma.model.parameters()])
    pb = torch.cat([p.detach().reshape(-1) for p in mb.model.parameters()])
    assert mb._plan.loo_calls >= 20 and mb._plan.calls == 0
    assert (pa - pb).abs().max() <= 1e-12 * max(1.0, pb.abs().max().item()), (pa - pb).abs().max()
    for objective in ("default", "mll", None):
        for explicit in (True, False):
            m, _ = _fit(family, objective, explicit, 3, monkeypatch)
            assert m.objective_ == "mll" and m._plan.loo_calls == 0 and m._plan.calls >= 3
    with pytest.raises(ValueError, match="objective"):
        LoadestGP().fit(*loadest_dataset(20), iterations=1, objective="cv")


def test_checkpoint_round_trip():
    cov, tgt = loadest_dataset(30)
    m = LoadestGP()
    m.fit(cov, tgt, iterations=3, objective="loo")
    buf = io.BytesIO()
    m.save(buf)
    buf.seek(0)
    record = torch.load(io.BytesIO(buf.getvalue()), map_location="cpu", weights_only=True)
    assert record["objective"] == "loo"
    m2 = LoadestGP.load(buf, cov, tgt)
    assert m2.objective_ == "loo"
    d = LoadestGP()
    d.fit(cov, tgt, iterations=3)
    buf = io.BytesIO()
    d.save(buf)
    record = torch.load(io.BytesIO(buf.getvalue()), map_location="cpu", weights_only=True)
    assert "objective" not in record  # a default fit's checkpoint is what it was
    buf.seek(0)
    assert LoadestGP.load(buf, cov, tgt).objective_ == "mll"


@pytest.mark.parametrize("closed_form", [True, False])
def test_fit_many_equals_single_fits(closed_form, monkeypatch):
    """Three ragged sites through ``fit_many(objective="loo")`` against three single ``fit(objective="loo")`` runs: the same
    optimiser, clipping and scheduler on the same step rows, the host algebra in a different order -- parameters and final
    objectives to 1e-9 after 6 iterations (rounding differences of a few ulp, amplified by six Adam steps of a normalised
    gradient)."""
    sizes = (31, 44, 27)
    data = [loadest_dataset(n, seed=10 + i) for i, n in enumerate(sizes)]
    singles = []
    for i, (cov, tgt) in enumerate(data):
        torch.manual_seed(i)
        m = LoadestGP()
        m.fit(cov, tgt, iterations=6, objective="loo")
        singles.append(m)
    many = [LoadestGP() for _ in sizes]
    objs = multisite_fit.fit_many(many, data, iterations=6, site_seeds=list(range(len(sizes))), objective="loo", closed_form=closed_form)
    assert bool(torch.isfinite(objs).all())
    for a, b in zip(many, singles):
        assert a.objective_ == "loo"
        pa = torch.cat([p.detach().reshape(-1) for _, p in sorted(a.model.named_parameters())])
        pb = torch.cat([p.detach().reshape(-1) for _, p in sorted(b.model.named_parameters())])
        assert (pa - pb).abs().max() <= 1e-9 * max(1.0, pb.abs().max().item()), (pa - pb).abs().max()
    dflt = [LoadestGP() for _ in sizes]
    multisite_fit.fit_many(dflt, data, iterations=2, site_seeds=list(range(len(sizes))), closed_form=closed_form)
    assert all(m.objective_ == "mll" for m in dflt)


def test_censored_fits_are_refused():
    cov, tgt = loadest_dataset(30)
    mask = np.zeros(30, dtype=bool)
    mask[3] = True
    with pytest.raises(NotImplementedError, match="not samples"):
        LoadestGP().fit(cov, tgt, iterations=1, objective="loo", censored=mask)
    with pytest.raises(NotImplementedError, match="not samples"):
        multisite_fit.fit_many([LoadestGP(), LoadestGP()], [loadest_dataset(20, seed=1), loadest_dataset(25, seed=2)], iterations=1,
                               objective="loo", censored=[None, np.arange(25) == 4])
    m = LoadestGP()
    m.fit(cov, tgt, iterations=1, objective="loo", censored=np.zeros(30, dtype=bool))  # no censored row: the plain LOO fit
    assert m.objective_ == "loo"
