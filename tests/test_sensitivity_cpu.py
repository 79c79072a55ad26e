"""CPU checks of the hyperparameter sensitivities: the two dense references against each other on every case of the GPU file,
and the host algebra of ``discontinuum_amd.hyperpar`` / ``loads`` on the plan double (``SensitivityOraclePlan``)."""
import pytest
import torch

from tests import sensitivity_helpers as sh


@pytest.mark.parametrize("model,d,n,m", sh.CASES)
def test_formulas_against_jvp_through_the_posterior(model, d, n, m):
    """(a) The formulas the device implements against forward-mode jvp through ``oracle.posterior``: <= 1e-10, two orders inside
    the GPU bound of 1e-8.  Worst measured over these cases: mean 1.2e-11, variance 4.0e-12 (every figure is printed)."""
    name, X, r, noise, theta, Xs = sh.build_case(model, d, n, m)
    diag, rhs = sh.columns(sh.E_MAX, sh.C_MAX, n)
    Jm, Jv = sh.reference(model, d, n, m)
    Fm, Fv = sh.formula_sensitivity(name, X, r, noise, theta, Xs, diag, rhs)
    P = theta.numel()
    assert tuple(Jm.shape) == (P + sh.E_MAX + sh.C_MAX, m) and tuple(Jv.shape) == (P + sh.E_MAX, m)
    em, ev = sh.scaled_rows(Fm, Jm).max().item(), sh.scaled_rows(Fv, Jv).max().item()
    print(f"sensitivity references {model} d={d} n={n} m={m}: mean {em:.2e}, variance {ev:.2e}")
    assert em <= 1e-10 and ev <= 1e-10, (em, ev)


# ---------------------------------------------------------------------------------------------------- the engine on the plan double
import numpy as np  # noqa: E402

from discontinuum_amd import hyperpar as hp  # noqa: E402
from discontinuum_amd.engines.base import ModelConfig  # noqa: E402
from discontinuum_amd.engines.hip import MarginalHIP  # noqa: E402
from discontinuum_amd.loadest_gp import LoadestGP  # noqa: E402
from discontinuum_amd.loads import period_groups, target_transform  # noqa: E402
from discontinuum_amd.rating_gp import RatingGP  # noqa: E402
from oracle import gp_oracle as orc  # noqa: E402
from tests.fisher_helpers import oracle_view  # noqa: E402
from tests.flux_helpers import FluxOraclePlan, daily_loadest, daily_rating  # noqa: E402


class EnginePlan(sh.SensitivityOraclePlan, FluxOraclePlan):
    """The plan double of these tests: ``fisher`` / ``whiten`` / ``predict_sensitivity`` and ``aggregate``'s dense entries."""


@pytest.fixture()
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(EnginePlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)


def fitted(kind, transform=None, iterations=8):
    """-> (engine, daily record): 60 / 40 observations in 2012-2014, about 110 prediction days (every 10th day)."""
    if kind == "loadest":
        cov_obs, target, daily = daily_loadest(n_obs=60, seed=1, step_days=10)
        engine = LoadestGP() if transform is None else LoadestGP(model_config=ModelConfig(transform=transform))
        engine.fit(cov_obs, target, iterations=iterations)
    else:
        cov_obs, target, unc, daily = daily_rating(n_obs=40, seed=2)
        t = daily.coords["time"].values[::10]
        daily = type(daily)({"stage": ("time", np.asarray(daily["stage"].values)[::10])}, coords={"time": t})
        engine = RatingGP()
        engine.fit(cov_obs, target, target_unc=unc, iterations=iterations)
    return engine, daily


def oracle_posterior(engine, kind, daily, pred_noise):
    """-> (f, raw, perm): ``f(raw)`` = (mu, var) of ``LoadestOracle.predict`` / ``RatingOracle.predict`` at the daily points as
    a function of the ORACLE's raw vector; ``perm[k]`` = the oracle position of the engine's raw value k.  The rating
    oracle's prediction always includes the learned noise: ``pred_noise=False`` takes it off again."""
    x = torch.tensor(engine.dm.Xnew(daily), dtype=torch.float64)
    engine._eval_ready(x.to(engine.device, engine.dtype))
    o, raw, perm, X, fixed = oracle_view(engine, kind)
    y = engine._train_y.double().cpu()
    if kind == "loadest":
        assert torch.allclose(fixed.expand(X.shape[0]), o.noise(raw, X.shape[0]))
    assert x.shape[0] != X.shape[0]  # (at m == n the oracles re-add the training noise)

    def f(v):
        mu, var = o.predict(v, X, y, x, None if kind == "loadest" else fixed)
        if kind == "rating" and not pred_noise:
            var = var - o.second_noise(v)
        return mu, var

    return f, raw, perm, x


def oracle_jacobian(f, raw, perm):
    """Forward-mode Jacobians of ``f`` in the ENGINE's raw order -> (J_mu (m, R), J_var (m, R)) numpy."""
    cols_m, cols_v = [], []
    for k in range(raw.numel()):
        e = torch.zeros_like(raw)
        e[perm[k]] = 1.0
        tm, tv = sh._jvp(f, raw.clone(), e)
        cols_m.append(tm)
        cols_v.append(tv)
    return torch.stack(cols_m, 1).numpy(), torch.stack(cols_v, 1).numpy()


def _cols(J, J_ref):
    return sh.scaled_rows(torch.as_tensor(J).T, torch.as_tensor(J_ref).T).max().item()


@pytest.mark.parametrize("kind", ["loadest", "rating"])
@pytest.mark.parametrize("pred_noise", [False, True])
def test_prediction_jacobians_against_the_oracles(kind, pred_noise, cpu_engine):
    """(b) ``prediction_jacobians`` -- device directions mapped to raw space, right-hand sides, the prior mean at the test rows,
    the predictive noise -- against forward-mode jvp through the model oracles' ``predict``."""
    engine, daily = fitted(kind)
    f, raw, perm, x = oracle_posterior(engine, kind, daily, pred_noise)
    J_mu, J_var = hp.prediction_jacobians(engine, x, pred_noise=pred_noise)
    R_mu, R_var = oracle_jacobian(f, raw, perm)
    assert J_mu.shape == R_mu.shape == (x.shape[0], raw.numel()) and J_var.shape == R_var.shape
    em, ev = _cols(J_mu, R_mu), _cols(J_var, R_var)
    print(f"prediction_jacobians {kind} pred_noise={pred_noise}: mean {em:.2e}, variance {ev:.2e}")
    assert em <= 1e-9 and ev <= 1e-9, (em, ev)
    assert np.abs(R_mu).max(axis=0).min() > 0  # every raw value moves the mean: no direction is trivially right


def _condition(engine, kind):
    o, raw, _perm, X, fixed = oracle_view(engine, kind)
    noise = fixed + (o.second_noise(raw) if kind == "rating" else 0.0)
    ev = torch.linalg.eigvalsh(orc.GRAMS[kind](X, X, o.constrained(raw)) + torch.diag(noise.expand(X.shape[0])))
    return (ev[-1] / ev[0]).item()


@pytest.mark.parametrize("kind,k", [("loadest", 4), ("rating", 7)])
def test_one_direction_by_central_differences(kind, k, cpu_engine):
    """(c) The only step size of this file, by the usual cube-root rule for central differences: h = eps_f^(1/3) max(1, |raw_k|)
    with eps_f = cond(K^) eps the relative precision of ONE evaluation of the posterior (a Cholesky solve), not the machine
    epsilon.  The quotient D(h) has a truncation error of h^2 / 6 times the third derivative, which D(2h) - D(h) estimates
    three times over, plus rounding of about eps_f |f| / h: the analytic column must agree with D(h) within
    |D(2h) - D(h)| + 4 eps_f max|f| / h."""
    engine, daily = fitted(kind)
    f, raw, perm, x = oracle_posterior(engine, kind, daily, False)
    J_mu, J_var = hp.prediction_jacobians(engine, x)
    eps_f = _condition(engine, kind) * np.finfo(np.float64).eps
    h = eps_f ** (1.0 / 3.0) * max(1.0, abs(float(raw[perm[k]])))

    def D(step):
        e = torch.zeros_like(raw)
        e[perm[k]] = step
        with torch.no_grad():
            (m1, v1), (m0, v0) = f(raw + e), f(raw - e)
        return ((m1 - m0) / (2 * step)).numpy(), ((v1 - v0) / (2 * step)).numpy()

    with torch.no_grad():
        mu0, var0 = f(raw.clone())
    (dm1, dv1), (dm2, dv2) = D(h), D(2 * h)
    for J, d1, d2, f0, what in ((J_mu[:, k], dm1, dm2, mu0, "mean"), (J_var[:, k], dv1, dv2, var0, "variance")):
        bound = np.abs(d2 - d1).max() + 4 * eps_f * float(f0.abs().max()) / h
        err = np.abs(J - d1).max()
        print(f"central differences {kind} raw {k} {what}: h {h:.1e}, |J - D(h)| {err:.2e}, bound {bound:.2e}, scale {np.abs(d1).max():.2e}")
        assert err <= bound and bound < 1e-4 * np.abs(d1).max(), (what, err, bound)


@pytest.mark.parametrize("kind,transform", [("loadest", None), ("loadest", "standard"), ("rating", None)])
def test_period_jacobian_against_the_oracles(kind, transform, cpu_engine):
    """(d) The period Jacobian G of ``aggregate(hyperparameters=True)`` against jvp of the period means -- sum w exp(s mu + t +
    s^2 sigma^2 / 2) for a log target (mode 1), sum w (s mu + t) for a standardised one (mode 0) -- through the oracle; and
    what ``aggregate`` makes of it."""
    engine, daily = fitted(kind, transform)
    mode, s, t = target_transform(engine.dm)
    assert mode == (0 if transform == "standard" else 1)
    rng = np.random.default_rng(5)
    w = rng.uniform(0.5, 2.0, len(daily.coords["time"].values))
    ds, pcov, cov_hyper = engine.aggregate(daily, w, freq="YE", return_cov=True, hyperparameters=True, prior=True)
    f, raw, perm, x = oracle_posterior(engine, kind, daily, False)
    order, groups, labels, _n, _d = period_groups(daily.coords["time"].values, w, "YE")
    A = torch.zeros(len(labels), len(w), dtype=torch.float64)
    A[torch.as_tensor(groups, dtype=torch.int64), torch.as_tensor(order)] = 1.0
    wt = torch.as_tensor(w)

    def means(v):
        mu, var = f(v)
        return A @ (wt * (torch.exp(s * mu + t + 0.5 * s * s * var) if mode == 1 else s * mu + t))

    G_ref = torch.stack([sh._jvp(means, raw.clone(), torch.eye(raw.numel(), dtype=torch.float64)[perm[k]]) for k in range(raw.numel())], 1)
    with torch.no_grad():
        assert np.allclose(ds["mean"].values, means(raw).numpy(), rtol=1e-9)
        mu, var = f(raw)
    a = (wt * (torch.exp(s * mu + t + 0.5 * s * s * var) if mode == 1 else 1.0)).numpy()
    time_groups = np.empty(len(w), dtype=np.int64)
    time_groups[order] = groups
    cov_h2, G = hp.period_hyper_covariance(engine, x, a, time_groups, len(labels), mode, s, prior=True)
    err = _cols(G, G_ref.numpy())
    print(f"period Jacobian {kind} mode {mode}: {err:.2e}")
    assert err <= 1e-9, err
    _params, cov_raw, _active, _un = hp.raw_covariance(engine, prior=True, x=x)
    ref = G_ref.numpy() @ cov_raw @ G_ref.numpy().T
    assert np.allclose(cov_hyper, ref, rtol=1e-7, atol=1e-12 * np.abs(ref).max()) and np.allclose(cov_h2, cov_hyper, rtol=1e-12)
    assert np.allclose(ds["se_hyper"].values, np.sqrt(np.diag(cov_hyper)))
    assert np.allclose(ds["se_total"].values, np.sqrt(ds["se"].values ** 2 + ds["se_hyper"].values ** 2))
    assert np.all(ds["se_hyper"].values > 0) and np.all(ds["lower_total"].values <= ds["lower"].values)
    assert np.all(ds["upper_total"].values >= ds["upper"].values)
    assert ds["se_total"].attrs["order"] == "first (delta method)"


def test_identities(cpu_engine):
    """(e) var_hyper = J Sigma J^T with Sigma = ``hyperparameter_uncertainty``'s ``cov_raw``; a clamped raw value contributes
    exactly 0; ``se_plugin`` is ``predict``'s standard error, bitwise."""
    engine, daily = fitted("rating")
    ds = engine.predict_marginalized(daily, ci=0.9, prior=True)
    x = torch.tensor(engine.dm.Xnew(daily), dtype=torch.float64)
    J_mu, _ = hp.prediction_jacobians(engine, x)
    unc = engine.hyperparameter_uncertainty(prior=True)
    Sigma = np.nan_to_num(unc["cov_raw"].values, nan=0.0)
    params, cov_raw, active, unident = hp.raw_covariance(engine, prior=True, x=x)
    assert np.array_equal(cov_raw, Sigma) and np.array_equal(active, unc["active"].values)
    assert np.allclose(ds["var_hyper"].values, np.einsum("ik,kl,il->i", J_mu, Sigma, J_mu), rtol=1e-12)
    target, se = engine.predict(daily)
    assert np.array_equal(ds["se_plugin"].values, np.asarray(se.values).reshape(-1))
    assert np.array_equal(ds["mean"].values, np.asarray(target.values).reshape(-1))
    assert np.all(ds["var_hyper"].values > 0) and np.all(ds["inflation"].values > 1)
    assert np.allclose(ds["inflation"].values, (ds["var_plugin"].values + ds["var_hyper"].values) / ds["var_plugin"].values)
    assert np.all(ds["se"].values >= ds["se_plugin"].values) and np.all(ds["lower"].values < ds["mean"].values)
    assert np.all(ds["mean"].values < ds["upper"].values)
    assert ds.attrs["order"] == "first (delta method)" and ds.attrs["ci"] == 0.9 and ds.attrs["prior"] is True
    assert ds.attrs["n_eff"] == unc.attrs["n_eff"] and ds.attrs["n_unidentified"] == unc["unidentified"].values.shape[0]
    # b on its clamp: its column of both Jacobians and its row / column of Sigma are exactly zero
    names = list(unc["parameter"].values)
    k = names.index("powerlaw.b")
    with torch.no_grad():
        engine.model.powerlaw.b.fill_(2.5)
    J2, V2 = hp.prediction_jacobians(engine, x)
    _p, cov2, active2, _u = hp.raw_covariance(engine, prior=True, x=x)
    assert np.all(J2[:, k] == 0.0) and np.all(V2[:, k] == 0.0) and not active2[k]
    assert np.all(cov2[k] == 0.0) and np.all(cov2[:, k] == 0.0) and np.all(np.isfinite(cov2))
    ds2 = engine.predict_marginalized(daily)
    keep = [i for i in range(len(names)) if i != k]
    assert np.allclose(ds2["var_hyper"].values, np.einsum("ik,kl,il->i", J2[:, keep], cov2[np.ix_(keep, keep)], J2[:, keep]), rtol=1e-12)


def test_a_test_stage_below_the_training_minimum_fixes_c(cpu_engine):
    """The rating model's c-clamp sees [X; X*]: a test stage below the fitted c resets c onto the clamp.  Its column of the
    Jacobians is zero AND Sigma_raw is the covariance of the other parameters with c fixed (the inverse of the information
    without c's row and column), not their marginal with c free."""
    from discontinuum_amd.rating_gp.models import STAGE

    engine, daily = fitted("rating")
    x = torch.tensor(engine.dm.Xnew(daily), dtype=torch.float64)
    names = [n for n, _p in hp.leaves(engine)]
    k = names.index("powerlaw.c")
    _p0, cov_free, active_free, _u0 = hp.raw_covariance(engine, prior=True, x=x)
    assert active_free[k] and cov_free[k, k] > 0
    x[0, STAGE] = float(engine.model.powerlaw.c.detach()) - 0.1
    J_mu, J_var = hp.prediction_jacobians(engine, x)
    params, cov, active, _un = hp.raw_covariance(engine, prior=True, x=x)
    assert float(engine.model.powerlaw.c.detach()) <= float(x[0, STAGE]) - 1e-6 + 1e-12  # reset onto the clamp
    assert not active[k] and active.sum() == len(names) - 1
    assert np.all(J_mu[:, k] == 0.0) and np.all(J_var[:, k] == 0.0) and np.all(cov[k] == 0.0) and np.all(cov[:, k] == 0.0)
    keep = [i for i in range(len(names)) if i != k]
    _p, F_raw, _a = hp.raw_information(engine, x)
    M = (F_raw + hp.prior_hessian(engine, params).numpy())[np.ix_(keep, keep)]
    fixed = np.linalg.inv(M)
    assert np.allclose(cov[np.ix_(keep, keep)], fixed, rtol=1e-6, atol=1e-10 * np.abs(fixed).max())
    _p1, F_tr, a_tr = hp.raw_information(engine)  # judged on the training rows alone, c would still count as free
    assert a_tr[k]


def test_aggregate_without_hyperparameters_is_unchanged(cpu_engine):
    """(f) ``hyperparameters=False`` returns exactly the variables it always did, and the same numbers as the shared ones of
    ``hyperparameters=True``."""
    engine, daily = fitted("loadest")
    plain = engine.annual_flux(daily, freq="YE")
    assert sorted(plain) == ["lower", "mean", "n_points", "se", "upper"]
    res = engine.annual_flux(daily, freq="YE", return_cov=True)
    assert isinstance(res, tuple) and len(res) == 2
    full = engine.annual_flux(daily, freq="YE", hyperparameters=True)
    assert sorted(full) == ["lower", "lower_total", "mean", "n_points", "se", "se_hyper", "se_total", "upper", "upper_total"]
    for key in plain:
        assert np.array_equal(np.asarray(plain[key].values), np.asarray(full[key].values)), key


def test_abi_of_dgp_predict_sensitivity_without_a_device():
    """The work-area query and every argument check of ``dgp_predict_sensitivity`` answer before any device is touched."""
    import ctypes as C

    from discontinuum_amd import _lib

    lib = _lib.load()
    h = C.c_void_p()
    assert lib.dgp_plan_create(_lib.MODEL_RATING, _lib.F32, 300, 2, C.byref(h)) == 0
    N, P, M = 384, 16, 256  # m = 130 pads to 256
    al = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for E, Cn in ((0, 0), (1, 3), (8, 8)):
        R = P + E + Cn
        want = (al(4 * M * 2) + P * N * N * 4 + 3 * al(4 * N * M) + al(8 * R * N) + al(8 * 32 * 2 * P * M) + al(8 * 32 * (R + E) * M)
                + al(8 * P * (N // 64) * M))
        assert lib.dgp_predict_sensitivity_workspace_bytes(h, 130, E, Cn) == want
    for bad in ((0, 0, 0), (130, 9, 0), (130, 0, 9), (130, -1, 0)):
        assert lib.dgp_predict_sensitivity_workspace_bytes(h, *bad) == 0
    assert lib.dgp_predict_sensitivity_workspace_bytes(None, 130, 0, 0) == 0
    theta = (C.c_double * P)(*([1.0] * P))
    fake = C.c_void_p(256)  # never dereferenced: every call below fails its checks first
    big = 1 << 40
    assert lib.dgp_predict_sensitivity(None, theta, fake, 130, None, 0, None, 0, fake, big, fake, fake, None) == -1
    assert lib.dgp_predict_sensitivity(h, None, fake, 130, None, 0, None, 0, fake, big, fake, fake, None) == -1
    assert lib.dgp_predict_sensitivity(h, theta, fake, 130, None, 0, None, 0, fake, big, None, fake, None) == -1
    assert lib.dgp_predict_sensitivity(h, theta, fake, 0, None, 0, None, 0, fake, big, fake, fake, None) == -1
    assert lib.dgp_predict_sensitivity(h, theta, fake, 130, fake, 9, None, 0, fake, big, fake, fake, None) == -1 and b"ndiag" in lib.dgp_last_error()
    assert lib.dgp_predict_sensitivity(h, theta, fake, 130, None, 0, fake, 9, fake, big, fake, fake, None) == -1 and b"nrhs" in lib.dgp_last_error()
    assert lib.dgp_predict_sensitivity(h, theta, fake, 130, None, 1, None, 0, fake, big, fake, fake, None) == -1
    assert lib.dgp_predict_sensitivity(h, theta, fake, 130, None, 0, None, 1, fake, big, fake, fake, None) == -1
    assert lib.dgp_predict_sensitivity(h, theta, fake, 130, None, 0, None, 0, fake, big, fake, None, None) == -3  # a plan without workspace
    assert lib.dgp_plan_destroy(h) == 0
