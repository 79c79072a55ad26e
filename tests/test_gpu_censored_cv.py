"""GPU parity of ``dgp_laplace_cross_validate`` (cross-validation of a censored fit by Laplace cavity folds) against dense
DELETION on the CPU in the W-form (tests/censored_cv_helpers.py) -- an independent route: the device never deletes anything, it
uses V_c = G_F^-1 diag(W_F) Sigma_FF from the held factorisation.

Bounds: the project's fp64 cross-validation bound (tests/test_gpu_crossval.py), 1e-8 -- ``MU`` relative to its max-norm, ``VAR``
PER ROW relative (the check the subtraction form C_ii - n~_i misses by four orders on the capped rows), ``LPD`` / ``TILT``
1e-8 max(1, |value|), ``PLO`` / ``PHI`` 1e-8 absolute, ``DLP`` relative to its max-norm.  The two CPU routes agree to 1e-10 on
these very datasets and folds (tests/test_censored_cv_cpu.py), so the reference stays two orders inside.  Every printed figure
is a measurement, the assertions are the bounds."""
import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from oracle import gp_oracle as orc
from tests import censored_cv_helpers as cvh
from tests import censored_helpers as ch
from tests.test_censored_cv_cpu import PLAN_CASES, _theta, plan_schemes
from tests.test_gpu_stages import plan_for

pytestmark = pytest.mark.gpu
TOL = 1e-11
SHIFT = 0.8


def _dev(dev, *arrays):
    return [torch.as_tensor(a, dtype=torch.int32 if np.asarray(a).dtype.kind == "i" else torch.float64).to(dev).contiguous() for a in arrays]


def _fitted_plan(n, seed, dev):
    X, _ = orc.synth_loadest(n, 2, seed=seed)
    y, side, v, m, upper = cvh.censored_fixture(X, seed)
    theta = _theta()
    plan = plan_for("loadest", 2, n, torch.tensor(X), torch.float64, dev)
    yd, vd, md, sd, ud = _dev(dev, y, v, m, side, np.where(np.isnan(upper), 0.0, upper))
    out, f_hat, stat = plan.laplace_factorize(theta, yd, md, vd, sd, tol=TOL, upper=ud)
    assert int(out[_lib.OUT_INFO].item()) == 0
    K = ch.gram("loadest", torch.tensor(X), theta)
    return plan, X, (y, side, v, m, upper), (yd, md, vd, sd, ud), theta, K, f_hat, stat


_CACHE = {}


def _case(n, seed, dev):
    """One factorised plan and its dense Gram matrix per dataset, shared by the tests (the plan is only read by them)."""
    if (n, seed) not in _CACHE:
        _CACHE[(n, seed)] = _fitted_plan(n, seed, dev)
    return _CACHE[(n, seed)]


def _errors(got, ref, held):
    mu, var = got["mu"][held], got["var"][held]
    rel = lambda k: float(np.max(np.abs(got[k] - ref[k])[held] / np.maximum(1.0, np.abs(ref[k][held]))))  # noqa: E731
    return {
        "mu": float(np.max(np.abs(mu - ref["mu"][held])) / np.max(np.abs(ref["mu"][held]))),
        "var": float(np.max(np.abs(var - ref["var"][held]) / ref["var"][held])),
        "lpd": rel("lpd"),
        "tilt": rel("tilt"),
        "pit_lower": float(np.max(np.abs(got["pit_lower"] - ref["pit_lower"])[held])),
        "pit_upper": float(np.max(np.abs(got["pit_upper"] - ref["pit_upper"])[held])),
        "dlp": float(np.max(np.abs(got["dlp"] - ref["dlp"])[held]) / np.max(np.abs(ref["dlp"][held]))),
    }


@pytest.mark.parametrize("n,seed", PLAN_CASES)
def test_parity_with_dense_deletion(n, seed, gpu_device):
    plan, X, (y, side, v, m, upper), (yd, md, vd, sd, ud), theta, K, f_hat, stat = _case(n, seed, gpu_device)
    assert stat[3] == 5, stat  # the cap is really exercised
    assert sorted(set(side.tolist())) == [-1, 0, 1, 2]
    f = f_hat.cpu().numpy()
    Xs = torch.tensor(X[:17]).to(gpu_device).contiguous()
    before = plan.predict(theta, Xs)
    for name, groups in plan_schemes(n).items():
        held = groups >= 0
        ref = cvh.dense_cavity_cv(K, y, side, v, m, f, groups, upper, SHIFT)
        res = plan.laplace_cross_validate(theta, yd, md, vd, sd, f_hat, groups, upper=ud, shift=SHIFT)
        got = {k: t.cpu().numpy() for k, t in res.items()}
        errs = _errors(got, ref, held)
        capped = held & (side == -1) & (y > ch.curve(X) + 7.0 * 0.1)
        e_cap = float(np.max(np.abs(got["var"] - ref["var"])[capped] / ref["var"][capped]))
        print(f"laplace cv n={n} {name}: " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()) + f" | var on the capped rows {e_cap:.2e}")
        assert all(e <= 1e-8 for e in errs.values()), (name, errs)
        assert bool((got["info"] == 0).all()) and got["info"].shape[0] == int(groups.max()) + 1
        for k in cvh.PLANES:  # rows that no fold holds are 0 in every plane
            assert np.all(got[k][~held] == 0.0), (name, k)
        again = plan.laplace_cross_validate(theta, yd, md, vd, sd, f_hat, groups, upper=ud, shift=SHIFT)
        assert all(torch.equal(res[k], again[k]) for k in res), name
        if name == "mod7":  # shift == 0: TILT is exactly 0, everything else keeps its bits
            zero = plan.laplace_cross_validate(theta, yd, md, vd, sd, f_hat, groups, upper=ud)
            assert bool((zero["tilt"] == 0).all()) and all(torch.equal(zero[k], res[k]) for k in res if k != "tilt")
    after = plan.predict(theta, Xs)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


def test_all_observed_is_the_plain_cross_validation(gpu_device):
    dev = gpu_device
    n = 130
    X, _ = orc.synth_loadest(n, 2, seed=3)
    y, _side, v, m = ch.synth(X, 0.3, 3)
    side = np.zeros(n, dtype=np.int32)
    theta = _theta()
    plan = plan_for("loadest", 2, n, torch.tensor(X), torch.float64, dev)
    yd, vd, md, sd = _dev(dev, y, v, m, side)
    _out, f_hat, _stat = plan.laplace_factorize(theta, yd, md, vd, sd, tol=TOL)
    for name, groups in (("loo", np.arange(n)), ("mod7", np.arange(n) % 7), ("mod2", np.arange(n) % 2)):
        res = {k: t.cpu().numpy() for k, t in plan.laplace_cross_validate(theta, yd, md, vd, sd, f_hat, groups, shift=SHIFT).items()}
        resid, var, _lpd, _info = (t.cpu().numpy() for t in plan.cross_validate(groups))
        e_mu = float(np.max(np.abs(res["mu"] - (y - resid))) / np.max(np.abs(y - resid)))
        e_var = float(np.max(np.abs(res["var"] - var) / var))
        sd_ = np.sqrt(res["var"])
        gauss = -0.5 * ((y - res["mu"]) / sd_) ** 2 - 0.5 * np.log(2 * np.pi * res["var"])
        e_lpd = float(np.max(np.abs(res["lpd"] - gauss) / np.maximum(1.0, np.abs(gauss))))
        print(f"laplace cv, all observed, {name}: mu {e_mu:.2e} var {e_var:.2e} lpd {e_lpd:.2e}")
        assert e_mu <= 1e-10 and e_var <= 1e-10 and e_lpd <= 1e-10, name
        assert np.array_equal(res["pit_lower"], res["pit_upper"]) and np.all(res["tilt"] == 0.0)
        assert np.allclose(res["dlp"], (y - res["mu"]) / res["var"], rtol=1e-12)


def test_error_paths(gpu_device):
    from discontinuum_amd.backend import GPPlan

    dev = gpu_device
    n, seed = PLAN_CASES[0]
    plan, X, (y, side, v, m, upper), (yd, md, vd, sd, ud), theta, K, f_hat, stat = _case(n, seed, dev)
    groups = np.arange(n) % 7
    Xs = torch.tensor(X[:9]).to(dev).contiguous()
    before = plan.predict(theta, Xs)
    with pytest.raises(_lib.DGPError) as err:  # a row of side 2 and no upper
        plan.laplace_cross_validate(theta, yd, md, vd, sd, f_hat, groups)
    assert err.value.code == _lib.E_ARG and "upper_dev" in str(err.value)
    bad = ud.clone()
    bad[int(np.flatnonzero(side == 2)[0])] = float("nan")
    with pytest.raises(_lib.DGPError) as err:
        plan.laplace_cross_validate(theta, yd, md, vd, sd, f_hat, groups, upper=bad)
    assert err.value.code == _lib.E_ARG and "bracket" in str(err.value)
    fresh = plan_for("loadest", 2, n, torch.tensor(X), torch.float64, dev)
    with pytest.raises(_lib.DGPError) as err:
        fresh.laplace_cross_validate(theta, yd, md, vd, sd, f_hat, groups, upper=ud)
    assert err.value.code == _lib.E_STATE and "factorisation" in str(err.value)
    with pytest.raises(ValueError, match="float64"):
        plan_for("loadest", 2, n, torch.tensor(X), torch.float32, dev).laplace_cross_validate(theta, yd, md, vd, sd, f_hat, groups, upper=ud)
    batched = GPPlan("loadest", n, 2, dtype=torch.float64, device=dev, batch=2)
    with pytest.raises(NotImplementedError, match="batched"):
        batched.laplace_cross_validate(theta, yd, md, vd, sd, f_hat, groups, upper=ud)
    # the C entry refuses both plans itself, and the workspace query answers 0
    lib = plan.lib
    for p in (batched, plan_for("loadest", 2, n, torch.tensor(X), torch.float32, dev)):
        assert int(lib.dgp_laplace_cross_validate_workspace_bytes(p._h, 7, 20)) == 0
        rc = lib.dgp_laplace_cross_validate(p._h, (_lib.C.c_double * p.ntheta)(), None, None, None, None, None, None, None, None, 7, 20, 0.0,
                                            None, 0, None, None, None)
        assert rc == _lib.E_ARG
    with pytest.raises(ValueError):
        plan.laplace_cross_validate(theta, yd, md, vd, sd, f_hat, np.full(n, -1), upper=ud)
    after = plan.predict(theta, Xs)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    # and the plan stays usable
    res = plan.laplace_cross_validate(theta, yd, md, vd, sd, f_hat, groups, upper=ud)
    assert bool(torch.isfinite(res["lpd"]).all())


def test_engine_cross_validate_and_flux_bias_on_the_device(gpu_device):
    """``LoadestGP.fit(censored=, target_upper=)`` on the GPU, then ``cross_validate("YE", laplace="cavity")`` and
    ``flux_bias(laplace="cavity")`` against the dense helper fed from the engine's own state: rtol 1e-7 in data space, as the
    engine-level test of the uncensored product (tests/test_gpu_crossval.py)."""
    from discontinuum_amd.loadest_gp import LoadestGP, censoring_from_bounds
    from discontinuum_amd.loads import target_transform
    from discontinuum_amd.validation import cv_folds
    from tests.helpers import loadest_dataset

    cov, target = loadest_dataset(n=120, seed=3)
    vals = np.asarray(target.values, dtype=np.float64)
    rng = np.random.default_rng(5)
    order = np.argsort(vals)
    low, high = vals.copy(), vals.copy()
    low[order[:14]], high[order[:14]] = 0.0, vals[order[14]]       # "< limit"
    low[order[-6:]], high[order[-6:]] = vals[order[-7]], np.nan     # "> limit"
    for i in rng.choice(order[14:-6], size=16, replace=False):      # brackets
        w = rng.uniform(0.1, 0.6)
        low[i], high[i] = vals[i] * (1 - 0.4 * w), vals[i] * (1 + 0.6 * w)
    wrap = lambda a: type(target)(a, dims=target.dims, coords=target.coords, name=target.name, attrs=target.attrs)  # noqa: E731
    tgt, codes, upper = censoring_from_bounds(wrap(low), wrap(high))
    assert (codes != 0).sum() == 36 and (codes == 2).sum() == 16
    model = LoadestGP()
    model.fit(cov, tgt, iterations=3, censored=codes, target_upper=upper)
    with pytest.raises(NotImplementedError, match="not available for a fit with censored observations"):
        model.cross_validate("YE")
    groups, labels = cv_folds(tgt.coords["time"].values, "YE")
    ds, per_fold = model.cross_validate("YE", return_folds=True, laplace="cavity")
    mode, s, t = target_transform(model.dm)
    with torch.no_grad():
        spec = model._prior()
        th = torch.as_tensor(spec.theta).detach().cpu().double()
        mean, noise = spec.mean.detach().cpu().numpy(), spec.noise.detach().cpu().numpy()
        Xtr, ytr = model._train_x.detach().cpu().double(), model._train_y.detach().cpu().numpy()
        cs = model._censor
        side, f, up = cs.side.cpu().numpy(), cs.f.cpu().numpy(), cs.upper.cpu().numpy()
    K = ch.gram("loadest", Xtr, th)

    def check(ds, groups, what):
        ref = cvh.dense_cavity_cv(K, ytr, side, noise, mean, f, groups, up, s)
        assert np.allclose(ds["predicted"].values, model.dm.y_t(ref["mu"]).values, rtol=1e-7, atol=0), what
        assert np.allclose(ds["se"].values, model.dm.error_pipeline.inverse_transform(ref["var"]).values, rtol=1e-7, atol=0), what
        assert np.allclose(ds["lpd"].values, ref["lpd"], rtol=1e-7, atol=0), what
        assert ds.attrs["elpd"] == pytest.approx(ref["lpd"].sum(), rel=1e-7), what
        return ref

    check(ds, groups, "YE")
    assert ds.attrs["n_folds"] == len(labels) and ds.attrs["approximation"] == "laplace-cavity" and ds.attrs["n_censored"] == 36
    assert per_fold["lpd"].values.sum() == pytest.approx(ds.attrs["elpd"], rel=1e-12)
    loo = model.cross_validate("loo", laplace="cavity")
    ref = check(loo, np.arange(120), "loo")
    flow = np.asarray(cov["flow"].values, dtype=np.float64)
    P = np.exp(s * ref["mu"] + t + 0.5 * s * s * ref["var"])
    O = np.where(side != 0, np.exp(s * ref["mu"] + t + 0.5 * s * s * ref["var"] + ref["tilt"]), np.asarray(tgt.values, dtype=np.float64))
    direct = ((P * flow).sum() - (O * flow).sum()) / (P * flow).sum()
    got = model.flux_bias(cv=loo, laplace="cavity")
    print(f"engine laplace cv: flux bias {got:.6e} (dense {direct:.6e})")
    assert got == pytest.approx(direct, rel=1e-7, abs=1e-9) and model.flux_bias(laplace="cavity") == got
