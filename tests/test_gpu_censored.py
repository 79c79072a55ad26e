"""Censored observations on the device: ``dgp_laplace_fit_step`` / ``dgp_laplace_factorize`` stage by stage against the
dense restatement of tests/censored_helpers.py, the pointwise functions against a 500-digit fixture, the bilinear
derivative sweep alone, the plan state the products read, the engine surface and the error paths.

Measured on an MI355X (EXPERIMENTS.md, "Censored observations"), the worst case over every case below against the dense
restatement: |f - f_ref| 1.35e-14, NLL 2.82e-15 relative, dtheta 2.54e-13 and dr 1.29e-13 of their largest entry (all
four in the composite case; loadest: 5.8e-15, 9.0e-16, 3.0e-14, 3.0e-14).  The committed bounds are ten times those
figures.  Pointwise functions on [-40, 8] against the 500-digit fixture: log Phi 8.8e-15 and h 1.8e-15 relative, h (z + h)
1.9e-12 relative, h [1 - (z + h)(z + 2 h)] 7.4e-11 absolute (no asymptotic branch: the issue's bounds stand)."""
import ctypes as C
import functools
import io

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from oracle import gp_oracle as orc
from tests import censored_helpers as ch
from tests import composite_helpers as comp

pytestmark = pytest.mark.gpu

LN2 = 0.6931471805599453
TOL = 1e-12
# ten times the measured worst case of each quantity (module docstring); the starting point was dgp_fit_step's 1e-10 / 1e-8
F_BOUND, NLL_BOUND, DTHETA_BOUND, DR_BOUND = 1.4e-13, 2.9e-14, 2.6e-12, 1.3e-12
COMPOSITE = "one column three kinds d=2"


def _plan(model, n, d, dev, dtype=torch.float64, batch=1):
    from discontinuum_amd.backend import GPPlan

    return GPPlan(model, n, d, dtype=dtype, device=dev, batch=batch)


@functools.lru_cache(maxsize=None)
def _case(kind, n, d, frac, seed):
    """-> (model name, X, y, side, v, m, theta) of a fixture, shared between tests and never modified."""
    if kind == "loadest":
        model = "loadest"
        X = torch.tensor(orc.synth_loadest(n, d, seed=seed)[0])
        theta = torch.full((orc.loadest_ntheta(d),), LN2, dtype=torch.float64)
        theta = theta * torch.linspace(0.8, 1.3, theta.numel(), dtype=torch.float64)
    else:
        index = comp.by_name(COMPOSITE)
        model = comp.define(comp.CASES[index].spec)
        X, theta = comp.data(index, n)[0], comp.CASES[index].theta
    y, side, v, m = ch.synth(X.numpy(), frac, seed)
    return model, X, y, side, v, m, theta


@functools.lru_cache(maxsize=None)
def _reference(kind, n, d, frac, seed):
    model, X, y, side, v, m, theta = _case(kind, n, d, frac, seed)
    return ch.laplace(model, X, y, side, v, m, theta, tol=TOL)


def _dev(dev, *arrays):
    return tuple(torch.as_tensor(a, dtype=torch.int32 if np.asarray(a).dtype.kind == "i" else torch.float64).to(dev).contiguous()
                 for a in arrays)


def _fit_step(plan, dev, case, f=None, maxit=50, tol=TOL):
    _model, X, y, side, v, m, theta = case
    plan.set_inputs(X.to(dev).contiguous())
    yd, vd, md, sd = _dev(dev, y, v, m, side)
    fd = None if f is None else torch.as_tensor(f, dtype=torch.float64).to(dev)
    out, dr, f_hat, stat = plan.laplace_fit_step(theta, yd, md, vd, sd, f=fd, maxit=maxit, tol=tol)
    return out.cpu(), dr.cpu(), f_hat.cpu(), stat


def _errors(out, dr, f_hat, ref, ntheta):
    nll = abs(float(out[_lib.OUT_NLL]) - ref["nll"]) / abs(ref["nll"])
    dth = np.abs(out[_lib.OUT_DTHETA:_lib.OUT_DTHETA + ntheta].numpy() - ref["dtheta"]).max() / np.abs(ref["dtheta"]).max()
    drr = np.abs(dr.numpy() - ref["dr"]).max() / np.abs(ref["dr"]).max()
    return float(np.abs(f_hat.numpy() - ref["f"]).max()), nll, float(dth), float(drr)


def _check_against(out, dr, f_hat, stat, ref, ntheta, label):
    ef, enll, edth, edr = _errors(out, dr, f_hat, ref, ntheta)
    print(f"censored {label}: |f - ref| {ef:.2e}, NLL rel {enll:.2e}, dtheta {edth:.2e}, dr {edr:.2e}, "
          f"iterations {stat[0]:.0f} (ref {ref['iterations']}), halvings {stat[2]:.0f}, capped {stat[3]:.0f}")
    assert int(out[_lib.OUT_INFO]) == 0
    assert ef <= F_BOUND and enll <= NLL_BOUND and edth <= DTHETA_BOUND and edr <= DR_BOUND, (ef, enll, edth, edr)
    assert abs(stat[0] - ref["iterations"]) <= 1 and stat[0] <= 30 and stat[1] <= TOL
    assert abs(float(out[_lib.OUT_SUM_DR]) - ref["dr"].sum()) <= DR_BOUND * np.abs(ref["dr"]).max() * len(ref["dr"])


def test_pointwise_functions_against_the_500_digit_fixture(gpu_device):
    import os

    data = np.load(os.path.join(os.path.dirname(__file__), "golden", "censored_terms.npy"))  # rows: z, the four functions
    z, ref = data[0], data[1:]
    plan = _plan("loadest", 8, 2, gpu_device)
    got = plan.censored_terms(torch.tensor(z).to(gpu_device)).cpu().numpy()
    near, far = slice(0, len(z) - 3), slice(len(z) - 3, len(z))
    assert z[near].min() == -40.0 and z[near].max() == 8.0 and z[far].tolist() == [-100.0, -300.0, -1000.0]
    rel = [float(np.max(np.abs(got[k][near] - ref[k][near]) / np.abs(ref[k][near]))) for k in range(3)]
    abs3 = float(np.max(np.abs(got[3][near] - ref[3][near])))
    print(f"censored terms on [-40, 8]: log Phi rel {rel[0]:.2e}, h rel {rel[1]:.2e}, h(z+h) rel {rel[2]:.2e}, "
          f"h[1-(z+h)(z+2h)] abs {abs3:.2e}")
    assert rel[0] <= 1e-13 and rel[1] <= 1e-13 and rel[2] <= 1e-11 and abs3 <= 1e-9
    assert np.all(np.isfinite(got[:, far])) and np.all((got[2][far] > 0) & (got[2][far] < 1))
    for k in range(2):
        assert np.max(np.abs(got[k][far] - ref[k][far]) / np.abs(ref[k][far])) <= 1e-13


def test_no_censoring_is_the_plain_fit_step_bitwise(gpu_device):
    n, d = 200, 3
    model, X, y, _side, v, m, theta = _case("loadest", n, d, 0.2, 1)
    plan = _plan(model, n, d, gpu_device)
    plan.set_inputs(X.to(gpu_device).contiguous())
    yd, vd, md = _dev(gpu_device, y, v, m)
    side = torch.zeros(n, dtype=torch.int32, device=gpu_device)
    out0, dr0, _dn = plan.fit_step(theta, (yd - md).contiguous(), vd)
    alpha0 = plan.buffer(_lib.BUF_ALPHA).clone()
    out0, dr0 = out0.clone(), dr0.clone()
    out1, dr1, f_hat, stat = plan.laplace_fit_step(theta, yd, md, vd, side, tol=TOL)
    assert torch.equal(out0, out1) and torch.equal(dr0, dr1) and torch.equal(alpha0, plan.buffer(_lib.BUF_ALPHA))
    assert stat == (0.0, 0.0, 0.0, 0.0)
    # f = m + K alpha = y - v alpha: the posterior mean at the samples
    assert torch.allclose(f_hat, yd - vd * dr1, rtol=0, atol=1e-14)
    outf = plan.factorize(theta, (yd - md).contiguous(), vd).clone()
    outl, _f, stat = plan.laplace_factorize(theta, yd, md, vd, side, tol=TOL)
    assert torch.equal(outf, outl) and stat[0] == 0.0


EDGE = [("loadest", n, 2, 0.2, n) for n in (1, 2, 127, 128, 129, 257)]
CASES = EDGE + [("loadest", 64, 2, 1.0, 7), ("loadest", 129, 3, 0.2, 11), ("loadest", 257, 3, 0.2, 12), ("composite", 129, 2, 0.2, 13)]


@pytest.mark.parametrize("kind,n,d,frac,seed", CASES, ids=[f"{c[0]}-n{c[1]}-d{c[2]}-{c[3]}" for c in CASES])
def test_stages_against_the_dense_restatement(gpu_device, kind, n, d, frac, seed):
    case = _case(kind, n, d, frac, seed)
    ref = _reference(kind, n, d, frac, seed)
    side = case[3]
    assert ref["converged"] and ref["capped"] == 0 and ref["iterations"] <= 30
    if n > 2:
        assert side[0] != 0 and side[-1] != 0 and (side == -1).any() and (side == 1).any()
    if frac == 1.0:
        assert (side != 0).all()
    plan = _plan(case[0], n, d, gpu_device)
    out, dr, f_hat, stat = _fit_step(plan, gpu_device, case)
    _check_against(out, dr, f_hat, stat, ref, plan.ntheta, f"{kind} n={n} d={d}")
    assert stat[3] == 0
    if n == 1:  # the mode solves a scalar equation
        k = float(ref["K"][0, 0])
        root = ch.scalar_mode(k, float(case[2][0]), int(side[0]), float(case[4][0]), float(case[5][0]))
        assert abs(float(f_hat[0]) - root) <= 1e-11
    # the value-only entry: same mode, same NLL, no gradient
    _m, X, y, side, v, m, theta = case
    yd, vd, md, sd = _dev(gpu_device, y, v, m, side)
    outf, ff, statf = plan.laplace_factorize(theta, yd, md, vd, sd, tol=TOL)
    outf = outf.cpu()
    assert abs(float(outf[_lib.OUT_NLL]) - ref["nll"]) <= NLL_BOUND * abs(ref["nll"]) and statf[0] == stat[0]
    assert torch.all(outf[_lib.OUT_DTHETA:] == 0) and float((ff.cpu() - f_hat).abs().max()) <= F_BOUND


def test_capped_row(gpu_device):
    """One left-censored limit 10 sigma above the data says nothing: the row is capped, the helper applies the same cap, and
    the predictions are those of the fit without the row."""
    n, d = 129, 2
    model, X, y, side, v, m, theta = _case("loadest", n, d, 0.2, 21)
    y, side = y.copy(), side.copy()
    row = 60
    y[row], side[row] = ch.curve(X.numpy())[row] + 1.0, -1
    case = (model, X, y, side, v, m, theta)
    ref = ch.laplace(model, X, y, side, v, m, theta, tol=TOL)
    assert ref["capped"] == 1
    plan = _plan(model, n, d, gpu_device)
    out, dr, f_hat, stat = _fit_step(plan, gpu_device, case)
    assert stat[3] == 1
    _check_against(out, dr, f_hat, stat, ref, plan.ntheta, "capped row n=129")
    Xs = torch.tensor(orc.synth_loadest(50, d, seed=99)[0]).to(gpu_device)
    mu, var = (t.cpu().clone() for t in plan.predict(theta, Xs))
    keep = np.arange(n) != row
    small = _plan(model, n - 1, d, gpu_device)
    _fit_step(small, gpu_device, (model, X[keep], y[keep], side[keep], v[keep], m[keep], theta))
    mu1, var1 = (t.cpu() for t in small.predict(theta, Xs))
    print(f"capped row: prediction against the fit without it: mean {float((mu - mu1).abs().max()):.2e}, var {float((var - var1).abs().max()):.2e}")
    assert float((mu - mu1).abs().max()) <= 1e-9 and float((var - var1).abs().max()) <= 1e-9


def test_warm_start(gpu_device):
    kind, n, d, frac, seed = "loadest", 257, 3, 0.2, 12
    case = _case(kind, n, d, frac, seed)
    plan = _plan(case[0], n, d, gpu_device)
    out, _dr, f_hat, stat = _fit_step(plan, gpu_device, case)
    out2, _dr2, f2, stat2 = _fit_step(plan, gpu_device, case, f=f_hat)
    assert stat[0] >= 2 and stat2[0] in (0.0, 1.0), (stat, stat2)
    assert abs(float(out2[_lib.OUT_NLL]) - float(out[_lib.OUT_NLL])) <= 1e-13 * abs(float(out[_lib.OUT_NLL]))
    assert float((f2 - f_hat).abs().max()) <= TOL


def test_plan_state_is_the_laplace_posterior(gpu_device):
    kind, n, d, frac, seed = "loadest", 257, 3, 0.2, 12
    case = _case(kind, n, d, frac, seed)
    ref = _reference(kind, n, d, frac, seed)
    plan = _plan(case[0], n, d, gpu_device)
    _fit_step(plan, gpu_device, case)
    theta = case[6]
    Xs = torch.tensor(orc.synth_loadest(50, d, seed=98)[0])
    ref_mu, ref_cov = ch.posterior(case[0], case[1], ref, Xs, full_cov=True)
    mu, var = (t.cpu() for t in plan.predict(theta, Xs.to(gpu_device)))
    mu2, cov = (t.cpu() for t in plan.posterior_cov(theta, Xs.to(gpu_device)))
    cov = torch.tril(cov[:50, :50])
    errs = (float((mu - ref_mu).abs().max()), float((var - torch.diagonal(ref_cov)).abs().max()), float((cov - torch.tril(ref_cov)).abs().max()))
    print(f"censored plan state: mean {errs[0]:.2e}, variance {errs[1]:.2e}, covariance {errs[2]:.2e}")
    assert max(errs) <= 1e-9 and torch.equal(mu, mu2)


@pytest.mark.parametrize("kind,n,d", [("loadest", 129, 3), ("loadest", 300, 2), ("composite", 129, 2), ("composite", 300, 2)])
def test_bilinear_sweep_alone(gpu_device, kind, n, d):
    model, X, _y, _side, _v, _m, theta = _case(kind, n, d, 0.2, 31)
    rng = np.random.default_rng(n)
    u, a = rng.standard_normal(n), rng.standard_normal(n)
    plan = _plan(model, n, d, gpu_device)
    plan.set_inputs(X.to(gpu_device).contiguous())
    ud, ad = _dev(gpu_device, u, a)
    got = plan.bilinear(theta, ud, ad).cpu()
    again = plan.bilinear(theta, ud, ad).cpu()
    ref = ch.bilinear(model, X, theta, u, a)
    err = float(np.abs(got.numpy() - ref).max() / np.abs(ref).max())
    print(f"bilinear sweep {kind} n={n}: {err:.2e} of the largest entry")
    assert err <= 1e-10 and torch.equal(got, again)


def _raw(plan, dev, case, f="cold", maxit=50, work_bytes=None, side=None, with_grad=True):
    """``dgp_laplace_fit_step`` through ctypes, as it is: -> (return code, out, stat, error text)."""
    _model, X, y, side0, v, m, theta = case
    lib = plan.lib
    yd, vd, md, sd = _dev(dev, y, v, m, side0 if side is None else side)
    fd = md.clone() if f == "cold" else f
    th = (C.c_double * len(theta))(*theta.tolist())
    need = max(int(lib.dgp_laplace_workspace_bytes(plan._h)), 1 << 16)
    work = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    base = work.data_ptr() + (-work.data_ptr()) % 256
    out = torch.zeros(_lib.OUT_LEN, dtype=torch.float64, device=dev)
    dr = torch.zeros(len(y), dtype=torch.float64, device=dev)
    stat = (C.c_double * 4)()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    with torch.cuda.device(dev):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.dgp_laplace_fit_step(plan._h, th, ptr(yd), ptr(md), ptr(vd), ptr(sd), ptr(fd), maxit, TOL, C.c_void_p(base),
                                      need if work_bytes is None else work_bytes, ptr(out), ptr(dr), stat, s)
        torch.cuda.synchronize(dev)
    return rc, out.cpu(), tuple(stat), lib.dgp_last_error().decode()


def test_error_paths(gpu_device):
    n, d = 129, 2
    case = _case("loadest", n, d, 0.2, 129)
    ref = _reference("loadest", n, d, 0.2, 129)
    plan = _plan("loadest", n, d, gpu_device)
    plan.set_inputs(case[1].to(gpu_device).contiguous())
    rc, _o, _s, msg = _raw(plan, gpu_device, case, f=None)
    assert rc == _lib.E_ARG and "f_dev" in msg
    rc, _o, _s, msg = _raw(plan, gpu_device, case, work_bytes=1024)
    assert rc == _lib.E_WORKSPACE
    bad = case[3].copy()
    bad[5] = 2
    rc, _o, _s, msg = _raw(plan, gpu_device, case, side=bad)
    assert rc == _lib.E_ARG and "side" in msg
    for other in (_plan("loadest", n, d, gpu_device, dtype=torch.float32), _plan("loadest", n, d, gpu_device, batch=2)):
        rc, _o, _s, msg = _raw(other, gpu_device, case)
        assert rc == _lib.E_ARG and "float64 single-site" in msg
    # too few iterations is a return code; the results are filled and the plan stays usable
    rc, out, stat, msg = _raw(plan, gpu_device, case, maxit=1)
    assert rc == _lib.E_NOCONV and "converge" in msg and stat[0] == 1.0 and stat[1] > TOL and np.isfinite(float(out[_lib.OUT_NLL]))
    with pytest.raises(_lib.DGPError) as err:
        _fit_step(plan, gpu_device, case, maxit=1)
    assert err.value.code == _lib.E_NOCONV and plan.laplace_stat[0] == 1.0
    out, dr, f_hat, stat = _fit_step(plan, gpu_device, case)
    _check_against(out, dr, f_hat, stat, ref, plan.ntheta, "after E_NOCONV")


def test_engine_fit_with_non_detects(gpu_device):
    """``LoadestGP.fit(censored=mask)`` at n = 300 with 15 % non-detects: predict, annual_flux and exceedance run, differ from
    the fit that takes the detection limits for samples, and equal the same products computed by the CPU engine over the dense
    restatement at the fitted hyperparameters (restored from the checkpoint, which carries the mask)."""
    from discontinuum_amd.loadest_gp import LoadestGP
    from tests.exceedance_helpers import ExceedOraclePlan
    from tests.flux_helpers import daily_loadest

    class RefPlan(ch.LaplaceOraclePlan, ExceedOraclePlan):
        pass

    class CpuRef(LoadestGP):
        _plan_factory = staticmethod(RefPlan)
        device = "cpu"

    cov_obs, target, daily = daily_loadest(n_obs=300, end="2014-01-01", seed=5)
    vals = np.asarray(target.values, dtype=np.float64)
    order = np.argsort(vals)
    mask = np.zeros(300, dtype=bool)
    mask[order[:45]] = True
    reported = vals.copy()
    reported[mask] = vals[order[45]]  # one detection limit: the 45 lowest samples are reported as "< limit"
    reported = type(target)(reported, dims=target.dims, coords=target.coords, name=target.name, attrs=target.attrs)
    model = LoadestGP()
    model.fit(cov_obs, reported, iterations=30, censored=mask)
    it, dmax, _halvings, capped = model.laplace_status_
    print(f"engine fit with 15 % non-detects: last mode search {it:.0f} Newton iterations, max |df| {dmax:.1e}, capped {capped:.0f}")
    assert it <= 30 and dmax <= model.laplace_tol
    tau = float(np.quantile(vals, 0.6))
    got = (model.predict(daily)[0].values, model.annual_flux(daily)["mean"].values, model.exceedance(daily, threshold=tau)["mean"].values)
    buf = io.BytesIO()
    model.save(buf)
    plain = LoadestGP()
    plain.fit(cov_obs, reported, iterations=30)
    sub = (plain.predict(daily)[0].values, plain.annual_flux(daily)["mean"].values, plain.exceedance(daily, threshold=tau)["mean"].values)
    buf.seek(0)
    cpu = CpuRef.load(buf, cov_obs, reported)
    assert cpu._censor is not None and int((cpu._censor.side != 0).sum()) == 45
    ref = (cpu.predict(daily)[0].values, cpu.annual_flux(daily)["mean"].values, cpu.exceedance(daily, threshold=tau)["mean"].values)
    points = np.asarray(model.exceedance(daily, threshold=tau)["n_points"].values, dtype=np.float64)
    for name, g, s, r, scale in (("predict", got[0], sub[0], ref[0], None), ("annual_flux", got[1], sub[1], ref[1], None),
                                 ("exceedance", got[2], sub[2], ref[2], points)):
        err = float(np.max(np.abs(g - r) / (np.abs(r) if scale is None else scale)))
        moved = float(np.max(np.abs(g - s) / (np.abs(s) if scale is None else scale)))
        print(f"engine {name}: against the dense restatement {err:.2e}, against substituting the limits {moved:.2e}")
        assert err <= 1e-8 and moved > 1e-4
