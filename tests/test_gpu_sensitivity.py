"""GPU parity of ``dgp_predict_sensitivity`` -- the exact Jacobians of the posterior mean and variance with respect to the
hyperparameter directions, from the held factorisation -- against forward-mode differentiation through the oracle's posterior
(tests/sensitivity_helpers.py: it shares nothing with the device's route), and of the engine-level first-order propagation
(``predict_marginalized``, ``annual_flux(hyperparameters=True)``) against the same algebra on the CPU plan double.

Error measure (scale-free, per direction): max_j |J - J_ref| / max_j |J_ref| (``scaled_rows``).  Bounds: fp64 plans 1e-8, the
project's gradient / variance tolerance (tests/test_sensitivity_cpu.py holds the reference itself to 1e-10 on every case used
here); a site in a batch against its single-site plan 1e-11 (tests/test_gpu_fisher.py's bound); fp32 plans:
see ``test_accuracy_fp32``.  Every printed figure is a measurement, the assertions are the bounds."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sensitivity_helpers as sh
from tests.sensitivity_helpers import dense_sensitivity, scaled_rows
from tests.test_gpu_bigtile import force_big_tiles
from tests.test_gpu_stages import make_case, plan_for

pytestmark = pytest.mark.gpu


def _held(model, d, n, X, r, noise, theta, dtype, dev, fit=False):
    from discontinuum_amd import _lib

    p = plan_for(model, d, n, X, dtype, dev)
    call = p.fit_step if fit else p.factorize
    out = call(theta, r.to(dev, dtype), noise.to(dev, dtype))
    out = out[0] if fit else out
    assert int(out[_lib.OUT_INFO]) == 0
    return p


def _dev(t, dev, dtype=torch.float64):
    return None if t is None else t.to(dev, dtype).contiguous()


@pytest.mark.parametrize("model,d,n,m", sh.CASES)
def test_accuracy_fp64(model, d, n, m, gpu_device):
    """Every (E, C) in {0, 1, 2} x {0, 1, 3} and the means-only call (``dvar_dev`` = NULL) against ONE dense reference per case.
    Measured on MI355X, worst scaled error over all 105 cases and every (E, C): mean 4.1e-11, variance 6.6e-12."""
    dev = gpu_device
    name, X, r, noise, theta, Xs = sh.build_case(model, d, n, m)
    ref = sh.reference(model, d, n, m)
    p = _held(name, d, n, X, r, noise, theta, torch.float64, dev)
    P, xs = theta.numel(), Xs.to(dev)
    worst_m = worst_v = 0.0
    for E in (0, 1, 2):
        for Cn in (0, 1, 3):
            diag, rhs = sh.columns(E, Cn, n)
            Jm, Jv = p.predict_sensitivity(theta, xs, _dev(diag, dev), _dev(rhs, dev))
            assert Jm.dtype == torch.float64 and tuple(Jm.shape) == (P + E + Cn, m)
            assert Jv.dtype == torch.float64 and tuple(Jv.shape) == (P + E, m)
            Rm, Rv = sh.reference_rows(ref, P, E, Cn)
            em, ev = scaled_rows(Jm, Rm).max().item(), scaled_rows(Jv, Rv).max().item()
            print(f"sensitivity fp64 {model} d={d} n={n} m={m} E={E} C={Cn}: mean {em:.2e}, variance {ev:.2e}")
            worst_m, worst_v = max(worst_m, em), max(worst_v, ev)
            assert em <= 1e-8 and ev <= 1e-8, (model, d, n, m, E, Cn, em, ev)
            if (E, Cn) == (2, 3):  # means only: the same numbers, no variance
                Jm0, none = p.predict_sensitivity(theta, xs, _dev(diag, dev), _dev(rhs, dev), return_var=False)
                assert none is None and torch.equal(Jm0, Jm)
    print(f"sensitivity fp64 {model} d={d} n={n} m={m}: worst mean {worst_m:.2e}, worst variance {worst_v:.2e}")


def _ragged(model, d, sizes, m, dev, seed0, big=False):
    """A ragged batch (NaN in the unused tails) held on the device -> (plan, cases, theta, Xs, diag, rhs), the last four batched."""
    from discontinuum_amd import _lib
    from discontinuum_amd.backend import GPPlan

    B, n = len(sizes), max(sizes)
    cases = [[torch.nan_to_num(t, nan=0.3) for t in make_case(model, d, nb, seed=seed0 + b, perturb=0.2)] for b, nb in enumerate(sizes)]
    X = torch.full((B, n, d), float("nan"), dtype=torch.float64)
    r = torch.full((B, n), float("nan"), dtype=torch.float64)
    noise = torch.full((B, n), float("nan"), dtype=torch.float64)
    dg = torch.full((B, 2, n), float("nan"), dtype=torch.float64)
    rh = torch.full((B, 3, n), float("nan"), dtype=torch.float64)
    for b, (nb, c) in enumerate(zip(sizes, cases)):
        X[b, :nb], r[b, :nb], noise[b, :nb] = c[0], c[1], c[2]
        dg[b, :, :nb], rh[b, :, :nb] = sh.columns(2, 3, nb, seed=b)
    theta = torch.stack([c[3] for c in cases])
    Xs = torch.stack([make_case(model, d, m, seed=seed0 + 50 + b)[0] for b in range(B)])
    pb = GPPlan(model, n, d, device=dev, lookahead=1, batch=B)
    if big:
        force_big_tiles(pb)
    pb.set_site_sizes(sizes)
    pb.set_inputs(X.to(dev).contiguous())
    out = pb.factorize(theta, r.to(dev).contiguous(), noise.to(dev).contiguous())
    assert bool((out[:, _lib.OUT_INFO] == 0).all())
    return pb, cases, theta, Xs, dg, rh


def test_large_tile_path_ragged(gpu_device):
    """n = 1300 / 1000 in one ragged batch with the tile selectors of test_gpu_bigtile.py, m = 300: the 128 x 128 direct-to-LDS
    core of beta = T^T V and of the quadratic forms' products (11 block rows, the shorter site with a ragged pad), each site
    against the dense reference.  Measured on MI355X: mean 6.4e-13 / 2.1e-13, variance 1.0e-13 / 4.4e-14."""
    dev, model, d, sizes, m = gpu_device, "loadest", 3, [1300, 1000], 300
    pb, cases, theta, Xs, dg, rh = _ragged(model, d, sizes, m, dev, seed0=40, big=True)
    Jm, Jv = pb.predict_sensitivity(theta, Xs.to(dev), _dev(dg[:, :1], dev), _dev(rh[:, :1], dev))
    for b, (nb, c) in enumerate(zip(sizes, cases)):
        Rm, Rv = dense_sensitivity(model, c[0], c[1], c[2], c[3], Xs[b], dg[b, :1, :nb], rh[b, :1, :nb])
        em, ev = scaled_rows(Jm[b], Rm).max().item(), scaled_rows(Jv[b], Rv).max().item()
        print(f"sensitivity fp64 128-tile core, site of n={nb} in N=1408, m={m}: mean {em:.2e}, variance {ev:.2e}")
        assert em <= 1e-8 and ev <= 1e-8, (nb, em, ev)


@pytest.mark.parametrize("model,d,sizes", [("loadest", 3, [300, 129, 257]),
                                           ("rating", 2, [129, 64, 200, 1, 2, 127, 128, 130, 77, 150, 199, 33])])
def test_ragged_batches_match_single_site_plans(model, d, sizes, gpu_device):
    """3 sites, and 12 (more than 8: the hyperparameters travel through the plan's scratch), different theta, test points and
    columns per site; the unused tails hold NaN.  Each site against its own single-site plan; the work area's previous content
    does not matter; a repeated call is bitwise identical."""
    dev, m = gpu_device, 130
    pb, cases, theta, Xs, dg, rh = _ragged(model, d, sizes, m, dev, seed0=60)
    xs, dgd, rhd = Xs.to(dev), _dev(dg, dev), _dev(rh, dev)
    Jm, Jv = pb.predict_sensitivity(theta, xs, dgd, rhd)
    ws = pb._sens_ws.view(torch.float64)
    half = ws.numel() // 2
    ws[:half] = float("nan")
    ws[half:] = 1e30
    dirty = pb.predict_sensitivity(theta, xs, dgd, rhd)
    ws.zero_()
    clean = pb.predict_sensitivity(theta, xs, dgd, rhd)
    for other in (dirty, clean, pb.predict_sensitivity(theta, xs, dgd, rhd)):
        assert torch.equal(Jm, other[0]) and torch.equal(Jv, other[1])
    assert bool(torch.isfinite(Jm).all()) and bool(torch.isfinite(Jv).all())
    worst = 0.0
    for b, (nb, c) in enumerate(zip(sizes, cases)):
        p1 = _held(model, d, nb, c[0], c[1], c[2], c[3], torch.float64, dev)
        Sm, Sv = p1.predict_sensitivity(c[3], xs[b], _dev(dg[b, :, :nb], dev), _dev(rh[b, :, :nb], dev))
        worst = max(worst, scaled_rows(Jm[b], Sm).max().item(), scaled_rows(Jv[b], Sv).max().item())
    print(f"sensitivity fp64 {model} ragged batch of {len(sizes)}: worst scaled difference to the single-site plans {worst:.2e}")
    assert worst <= 1e-11, worst
    Rm, Rv = dense_sensitivity(model, cases[0][0], cases[0][1], cases[0][2], cases[0][3], Xs[0], dg[0, :, :sizes[0]], rh[0, :, :sizes[0]])
    assert scaled_rows(Jm[0], Rm).max().item() <= 1e-8 and scaled_rows(Jv[0], Rv).max().item() <= 1e-8


def test_repeatable_and_chunked(gpu_device):
    """Two calls are bitwise identical, and so are a chunked and an unchunked call: the chunks' columns are independent."""
    dev, model, d, n, m = gpu_device, "loadest", 3, 300, 300
    name, X, r, noise, theta, Xs = sh.build_case(model, d, n, m)
    p = _held(name, d, n, X, r, noise, theta, torch.float64, dev)
    diag, rhs = sh.columns(2, 3, n)
    args = (theta, Xs.to(dev), _dev(diag, dev), _dev(rhs, dev))
    Jm, Jv = p.predict_sensitivity(*args)
    Jm2, Jv2 = p.predict_sensitivity(*args)
    assert torch.equal(Jm, Jm2) and torch.equal(Jv, Jv2)
    Jm3, Jv3 = p.predict_sensitivity(*args, chunk=128)
    assert torch.equal(Jm, Jm3) and torch.equal(Jv, Jv3)


def test_the_held_fit_survives(gpu_device):
    """fit_step, then predict_sensitivity: A, T, K^^-1, alpha and a following predict, gradient and fisher are bitwise what they
    are without the call."""
    from discontinuum_amd import _lib

    dev, model, d, n = gpu_device, "rating", 2, 300
    X, r, noise, theta = make_case(model, d, n, seed=4, perturb=0.2)
    Xs, *_ = make_case(model, d, 77, seed=5)
    p = _held(model, d, n, X, r, noise, theta, torch.float64, dev, fit=True)
    diag, rhs = sh.columns(2, 3, n)
    bufs = (_lib.BUF_A, _lib.BUF_T, _lib.BUF_S, _lib.BUF_ALPHA, _lib.BUF_XT)
    before = [p.buffer(w).clone() for w in bufs]
    pred0 = [t.clone() for t in p.predict(theta, Xs.to(dev))]
    grad0 = p.stage_grad(theta).clone()
    F0 = p.fisher(theta, _dev(diag, dev)).clone()
    p.predict_sensitivity(theta, Xs.to(dev), _dev(diag, dev), _dev(rhs, dev))
    p.predict_sensitivity(theta, Xs.to(dev), return_var=False)
    for w, b0 in zip(bufs, before):
        assert torch.equal(p.buffer(w), b0), w
    pred1 = p.predict(theta, Xs.to(dev))
    assert torch.equal(pred0[0], pred1[0]) and torch.equal(pred0[1], pred1[1])
    assert torch.equal(grad0, p.stage_grad(theta))
    assert torch.equal(F0, p.fisher(theta, _dev(diag, dev)))


# fp32 plans against the fp64 plan on the same (float32-rounded) inputs, E = 2, C = 3, m = 300, worst direction, asserted in the
# project's form c cond(K^) eps32 (tests/test_gpu_fp32.py).  Measured on MI355X, in units of cond(K^) eps32 (mean / variance):
#   loadest n = 300  (cond 8.6e2): 0.144 / 0.184        loadest n = 1300 (cond 1.8e4): 0.061 / 0.018
#   rating  n = 300  (cond 2.1e4): 0.095 / 0.095        rating  n = 1300 (cond 9.9e4): 0.434 / 0.154
# Worst 0.434: c = 2 is the smallest power of two that leaves at least a factor 4 over it (4.6) -- the factor that covers the
# box-to-box and seed-to-seed spread this project has recorded for fp32.  (Seeds 7, 8, 9 with other test points, same sizes:
# 0.011 ... 0.82, worst rating n = 1300 variance -- inside the bound)
EPS32 = 2.0 ** -24
FP32_C = 2.0


@pytest.mark.parametrize("model,d", [("loadest", 3), ("rating", 2)])
@pytest.mark.parametrize("n", [300, 1300])
def test_accuracy_fp32(model, d, n, gpu_device):
    from oracle import gp_oracle as orc

    dev, m = gpu_device, 300
    X, r, noise, theta = (t.float().double() for t in make_case(model, d, n, seed=7, perturb=0.1))
    Xs = make_case(model, d, m, seed=8)[0].float().double()
    diag, rhs = (t.float().double() for t in sh.columns(2, 3, n))
    ev = torch.linalg.eigvalsh(orc.GRAMS[model](X, X, theta) + torch.diag(noise))
    cond = (ev[-1] / ev[0]).item()
    p64 = _held(model, d, n, X, r, noise, theta, torch.float64, dev)
    Rm, Rv = p64.predict_sensitivity(theta, Xs.to(dev), _dev(diag, dev), _dev(rhs, dev))
    p32 = _held(model, d, n, X, r, noise, theta, torch.float32, dev)
    Jm, Jv = p32.predict_sensitivity(theta, Xs.to(dev, torch.float32), _dev(diag, dev, torch.float32), _dev(rhs, dev, torch.float32))
    assert Jm.dtype == torch.float64 and Jv.dtype == torch.float64
    em, evr = scaled_rows(Jm, Rm).max().item(), scaled_rows(Jv, Rv).max().item()
    unit = cond * EPS32
    print(f"sensitivity fp32 {model} n={n}: cond {cond:.3e}, mean {em:.2e} = {em / unit:.2e} cond eps32, variance {evr:.2e} = "
          f"{evr / unit:.2e} cond eps32")
    assert em <= FP32_C * unit and evr <= FP32_C * unit, (model, n, em / unit, evr / unit)


def test_loud_failures(gpu_device):
    """Error codes and Python exceptions, never a fault; nothing is launched on a refused call."""
    from discontinuum_amd import _lib
    from discontinuum_amd.backend import _ptr, _stream, _theta_array

    E_ARG, E_WORKSPACE, E_STATE = -1, -3, -4
    dev, model, d, n, m = gpu_device, "loadest", 2, 200, 70
    X, r, noise, theta = make_case(model, d, n, seed=6)
    Xs = make_case(model, d, m, seed=7)[0].to(dev)
    p = plan_for(model, d, n, X, torch.float64, dev)
    lib, th, P = p.lib, _theta_array(theta, p.ntheta), p.ntheta
    need = int(lib.dgp_predict_sensitivity_workspace_bytes(p._h, m, 2, 3))
    assert need >= (P * p.N * p.N + 3 * p.N * 128) * 8
    for bad in ((0, 2, 3), (-1, 2, 3), (m, 9, 0), (m, -1, 0), (m, 0, 9), (m, 0, -1)):
        assert int(lib.dgp_predict_sensitivity_workspace_bytes(p._h, *bad)) == 0
    assert int(lib.dgp_predict_sensitivity_workspace_bytes(None, m, 0, 0)) == 0
    work = torch.empty(need + 512, dtype=torch.uint8, device=dev)
    base = work.data_ptr()
    aligned = base + (-base) % 256
    dmean = torch.full((P + 5, m), 7.0, dtype=torch.float64, device=dev)
    dvar = torch.full((P + 2, m), 7.0, dtype=torch.float64, device=dev)
    diag, rhs = (_dev(t, dev) for t in sh.columns(2, 3, n))

    def call(h=p._h, xs=Xs, mm=m, dg=diag, E=2, rh=rhs, Cn=3, wp=aligned, bytes_=need, out=dmean):
        with torch.cuda.device(dev):
            return int(lib.dgp_predict_sensitivity(h, th, _ptr(xs), mm, _ptr(dg), E, _ptr(rh), Cn, C.c_void_p(wp), bytes_, _ptr(out),
                                                   _ptr(dvar), _stream()))

    assert call() == E_STATE  # no factorisation yet
    with pytest.raises(_lib.DGPError):
        p.predict_sensitivity(theta, Xs)
    assert int(p.factorize(theta, r.to(dev), noise.to(dev))[_lib.OUT_INFO]) == 0
    assert call(h=None) == E_ARG and call(out=None) == E_ARG and call(xs=None) == E_ARG
    assert call(mm=0) == E_ARG and call(mm=-3) == E_ARG
    assert call(E=9) == E_ARG and call(E=-1) == E_ARG and call(Cn=9) == E_ARG and call(Cn=-1) == E_ARG
    assert call(dg=None) == E_ARG and call(rh=None) == E_ARG
    assert call(bytes_=need - 1) == E_WORKSPACE and call(wp=None) == E_WORKSPACE
    assert call(wp=aligned + 8) == E_ARG  # misaligned
    assert bool((dmean == 7.0).all()) and bool((dvar == 7.0).all())  # nothing was launched
    assert call() == 0 and bool(torch.isfinite(dmean).all()) and bool(torch.isfinite(dvar).all())
    with pytest.raises(ValueError):
        p.predict_sensitivity(theta, Xs, torch.ones(9, n, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        p.predict_sensitivity(theta, Xs, None, torch.ones(1, n + 1, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        p.predict_sensitivity(theta, Xs, torch.ones(1, n, dtype=torch.float32, device=dev))
    # a plan whose factorisation failed: an indefinite matrix
    Xb = X.clone()
    Xb[150] = Xb[149]
    pb = plan_for(model, d, n, Xb, torch.float64, dev)
    bad = pb.fit_step(theta, r.to(dev), torch.full((n,), -0.5, dtype=torch.float64, device=dev))[0]
    assert int(bad[_lib.OUT_INFO]) >= 1
    with pytest.raises(_lib.DGPError) as ei:
        pb.predict_sensitivity(theta, Xs)
    assert ei.value.code == E_STATE


# ---- the engine: predict_marginalized / annual_flux(hyperparameters=True) on the device against the CPU route of
# tests/test_sensitivity_cpu.py -- Jacobians by forward-mode jvp through the model oracles, Sigma_raw from the model oracles
def _record(kind, m=110, seed=9):
    """A prediction record that is not the training record: m days, 20 days apart, inside the training period."""
    from discontinuum_amd.xr_compat import Dataset

    rng = np.random.default_rng(seed)
    time = (np.datetime64("2010-01-05") + 20 * np.arange(m).astype("timedelta64[D]")).astype("datetime64[ns]")
    if kind == "loadest":
        return Dataset({"flow": ("time", np.exp(rng.standard_normal(m)) * 10, {"units": "cubic meters per second"})}, coords={"time": time})
    return Dataset({"stage": ("time", 1.0 + 3.0 * rng.beta(2, 5, m))}, coords={"time": time})


@pytest.mark.parametrize("kind,n", [("loadest", 200), ("rating", 150)])
def test_engine_propagation_against_the_oracles(kind, n, gpu_device):
    """Bounds.  The raw-space Jacobians: 1e-7, the bound of the engine's information in tests/test_gpu_fisher.py (device
    Jacobians at 1e-8, mapped through the same forward-mode host Jacobians).  var_hyper and cov_hyper with the ENGINE's own
    Sigma_raw and the oracle's Jacobians: 1e-6 (the Jacobians enter twice; Sigma_raw is shared).  With Sigma_raw from the model
    oracles as well: 1e-4 -- tests/test_gpu_fisher.py holds cov_raw to 1e-6 of its largest entry, and the contraction J Sigma J^T
    cancels: measured amplification below 30 (printed)."""
    from discontinuum_amd import hyperpar as hp
    from discontinuum_amd.loads import period_groups, target_transform
    from tests.fisher_helpers import oracle_information, oracle_prior_hessian, oracle_view
    from tests.test_gpu_fisher import _fitted_engine
    from tests.test_sensitivity_cpu import _cols, oracle_jacobian, oracle_posterior

    engine, record = _fitted_engine(kind, n), _record(kind)
    ds = engine.predict_marginalized(record, ci=0.95, prior=True)
    f, raw, perm, x = oracle_posterior(engine, kind, record, False)
    R_mu, R_var = oracle_jacobian(f, raw, perm)
    J_mu, J_var = hp.prediction_jacobians(engine, x)
    em, ev = _cols(J_mu, R_mu), _cols(J_var, R_var)
    unc = engine.hyperparameter_uncertainty(prior=True)
    Sigma = np.nan_to_num(unc["cov_raw"].values, nan=0.0)
    ref = np.einsum("ik,kl,il->i", R_mu, Sigma, R_mu)
    e_own = np.abs(ds["var_hyper"].values - ref).max() / ref.max()
    o, raw_o, perm_o, X, fixed = oracle_view(engine, kind)
    F_ref = oracle_information(o, kind, raw_o, X, fixed)[perm_o][:, perm_o]
    H_ref = oracle_prior_hessian(o, kind, raw_o)[perm_o][:, perm_o]
    Sigma_ref = np.nan_to_num(hp.invert_information((F_ref + H_ref).numpy(), np.ones(raw_o.numel(), dtype=bool))[0], nan=0.0)
    ref2 = np.einsum("ik,kl,il->i", R_mu, Sigma_ref, R_mu)
    e_all = np.abs(ds["var_hyper"].values - ref2).max() / ref2.max()
    print(f"engine {kind} n={n}: raw Jacobians mean {em:.2e} variance {ev:.2e}; var_hyper against the oracle Jacobians {e_own:.2e}, "
          f"with the oracle's Sigma_raw too {e_all:.2e}; inflation {ds['inflation'].values.min():.3f} .. {ds['inflation'].values.max():.3f}")
    assert em <= 1e-7 and ev <= 1e-7, (em, ev)
    assert e_own <= 1e-6 and e_all <= 1e-4, (e_own, e_all)
    target, se = engine.predict(record)
    assert np.array_equal(ds["se_plugin"].values, np.asarray(se.values).reshape(-1))
    assert np.array_equal(ds["mean"].values, np.asarray(target.values).reshape(-1))
    assert np.all(ds["inflation"].values > 1) and ds.attrs["order"] == "first (delta method)"
    assert ds.attrs["n_eff"] == unc.attrs["n_eff"]
    # period sums: annual_flux for the load model, aggregate with unit weights for the rating model; dense and streamed path
    mode, s, t = target_transform(engine.dm)
    if kind == "loadest":
        from discontinuum_amd.loads import flux_weights, _target_attrs

        w = flux_weights(record, _target_attrs(engine.dm))
        call = lambda **k: engine.annual_flux(record, freq="YE", return_cov=True, hyperparameters=True, **k)  # noqa: E731
    else:
        w = np.ones(len(record.coords["time"].values))
        call = lambda **k: engine.aggregate(record, w, freq="YE", return_cov=True, hyperparameters=True, **k)  # noqa: E731
    agg, pcov, cov_hyper = call()
    order, groups, labels, _n, _d = period_groups(record.coords["time"].values, w, "YE")
    A = torch.zeros(len(labels), len(w), dtype=torch.float64)
    A[torch.as_tensor(groups, dtype=torch.int64), torch.as_tensor(order)] = 1.0
    wt = torch.as_tensor(w)

    def means(v):
        mu, var = f(v)
        return A @ (wt * (torch.exp(s * mu + t + 0.5 * s * s * var) if mode == 1 else s * mu + t))

    G_ref = torch.stack([sh._jvp(means, raw.clone(), torch.eye(raw.numel(), dtype=torch.float64)[perm[k]]) for k in range(raw.numel())], 1).numpy()
    ref_h = G_ref @ Sigma @ G_ref.T
    e_h = np.abs(cov_hyper - ref_h).max() / np.abs(ref_h).max()
    streamed = call(max_bytes=1)
    e_s = np.abs(streamed[2] - cov_hyper).max() / np.abs(cov_hyper).max()
    print(f"engine {kind} n={n}: cov_hyper against the oracle's period Jacobian {e_h:.2e}; streamed against dense path {e_s:.2e}; "
          f"se_hyper / se {np.min(agg['se_hyper'].values / agg['se'].values):.2f} .. {np.max(agg['se_hyper'].values / agg['se'].values):.2f}")
    assert e_h <= 1e-6 and e_s <= 1e-9, (e_h, e_s)
    assert np.allclose(agg["se_total"].values, np.sqrt(agg["se"].values ** 2 + np.diag(cov_hyper)))
