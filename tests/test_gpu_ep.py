"""Expectation propagation for censored fits on the device: ``GPPlan.ep_fit_step`` / ``ep_factorize`` / ``ep_diag`` against the dense
restatement of tests/ep_helpers.py (which is the definition), the bitwise properties, warm start, the error rules and the engine.

Sizes: n in {2, 127, 130, 257} -- one tile, just under and over a 128 boundary, three tiles (and two row chunks of the diagonal pass).
Records: ``interval_helpers.synth`` (one-sided rows of both signs and brackets), 30 % and 80 % censored, both sides run cold to
tol 1e-12.

Bounds.  The starting point is what the Laplace entries are held to (test_gpu_censored.py): the mode's bound for the sites and the
posterior means, and its bounds for NLL, dtheta and dr.  A quantity that misses its bound gets ten times its measured worst case,
never looser than 1e-6 ("Expectation propagation for censored fits", lists the measurements).  k against
2 dnoise + alpha^2 of the fit step: 1e-12 relative."""
import ctypes as C
import functools
import io

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from oracle import gp_oracle as orc
from tests import censored_helpers as ch
from tests import ep_helpers as eh
from tests import interval_helpers as ih
from tests import test_gpu_censored as base
from tests import test_gpu_interval as ivt

pytestmark = pytest.mark.gpu

TOL = 1e-12
# sites and means (absolute, relative to max(1, |reference|); n~ relative), NLL (relative), dtheta and dr (of the largest entry)
SITE_BOUND, MU_BOUND, NLL_BOUND, DTHETA_BOUND, DR_BOUND = base.F_BOUND, base.F_BOUND, base.NLL_BOUND, base.DTHETA_BOUND, base.DR_BOUND
SIZES = (2, 127, 130, 257)
CASES = [(n, 2 + (n % 2), frac, 300 + n) for n in SIZES for frac in (0.3, 0.8)]


@functools.lru_cache(maxsize=None)
def _reference(n, d, frac, seed):
    model, X, y, side, v, m, theta, upper = ivt._case(n, d, frac, seed)
    return eh.ep_fit(model, X, y, side, v, m, theta, upper=upper, tol=TOL)


def _dev(dev, *arrays):
    return base._dev(dev, *arrays)


def _call(plan, dev, case, sites=None, tol=TOL, maxit=100, damping=1.0, with_grad=True):
    _model, X, y, side, v, m, theta, upper = case
    plan.set_inputs(X.to(dev).contiguous())
    yd, vd, md, sd, ud = _dev(dev, y, v, m, side, upper)
    fn = plan.ep_fit_step if with_grad else plan.ep_factorize
    return fn(theta, yd, md, vd, sd, sites=sites, maxit=maxit, tol=tol, damping=damping, upper=ud)


def _errors(out, dr, sites, ref, ntheta):
    yt, nt = (t.cpu().numpy() for t in sites)
    e_y = float(np.max(np.abs(yt - ref["yt"]) / np.maximum(1.0, np.abs(ref["yt"]))))
    e_n = float(np.max(np.abs(nt - ref["nt"]) / ref["nt"]))
    a = dr.cpu().numpy()
    e_mu = float(np.max(np.abs((yt - nt * a) - ref["mu"]) / np.maximum(1.0, np.abs(ref["mu"]))))
    out = out.cpu()
    e_nll = abs(float(out[_lib.OUT_NLL]) - ref["nll"]) / abs(ref["nll"])
    e_dth = float(np.abs(out[_lib.OUT_DTHETA:_lib.OUT_DTHETA + ntheta].numpy() - ref["dtheta"]).max() / np.abs(ref["dtheta"]).max())
    e_dr = float(np.abs(a - ref["dr"]).max() / np.abs(ref["dr"]).max())
    return e_y, e_n, e_mu, e_nll, e_dth, e_dr


@pytest.mark.parametrize("n,d,frac,seed", CASES, ids=[f"n{c[0]}-{c[2]}" for c in CASES])
def test_device_against_the_oracle(gpu_device, n, d, frac, seed):
    case = ivt._case(n, d, frac, seed)
    ref = _reference(n, d, frac, seed)
    side = case[3]
    assert ref["converged"] and ref["stat"][4] == 0 and ref["stat"][0] <= 60
    assert (side == 2).any() and (side != 0).sum() >= min(n, round(frac * n))
    if n > 2:
        assert (side == -1).any() and (side == 1).any()
    plan = base._plan(case[0], n, d, gpu_device)
    out, dr, sites, stat = _call(plan, gpu_device, case)
    aux = {k: t.cpu().numpy() for k, t in plan.ep_aux.items()}
    e_y, e_n, e_mu, e_nll, e_dth, e_dr = _errors(out, dr, sites, ref, plan.ntheta)
    e_cav = max(float(np.max(np.abs(aux["cav_mean"] - ref["cav_mean"]))), float(np.max(np.abs(aux["cav_var"] - ref["cav_var"]) / ref["cav_var"])),
                float(np.max(np.abs(aux["logz"] - ref["logz"])[side != 0])))
    print(f"ep n={n} frac={frac}: y~ {e_y:.2e}, n~ {e_n:.2e}, mu {e_mu:.2e}, NLL rel {e_nll:.2e}, dtheta {e_dth:.2e}, dr {e_dr:.2e}, "
          f"cavities / log Z {e_cav:.2e}; sweeps {stat[0]:.0f} (oracle {ref['stat'][0]:.0f}), d_mu {stat[1]:.1e}, d_tau {stat[2]:.1e}")
    assert int(out.cpu()[_lib.OUT_INFO]) == 0
    assert stat[5] == float((side != 0).sum()) and stat[4] == 0 and stat[3] == ref["stat"][3]
    assert abs(stat[0] - ref["stat"][0]) <= 1 and stat[1] <= TOL and stat[2] <= TOL
    assert max(e_y, e_n) <= SITE_BOUND and e_mu <= MU_BOUND and e_nll <= NLL_BOUND and e_dth <= DTHETA_BOUND and e_dr <= DR_BOUND, (
        e_y, e_n, e_mu, e_nll, e_dth, e_dr)
    assert e_cav <= 1e-8
    assert abs(float(out.cpu()[_lib.OUT_SUM_DR]) - ref["dr"].sum()) <= DR_BOUND * np.abs(ref["dr"]).max() * n
    # a second call repeats bitwise; the value-only entry: the same sites and value, no gradient
    out2, dr2, sites2, stat2 = _call(plan, gpu_device, case)
    assert torch.equal(out, out2) and torch.equal(dr, dr2) and stat == stat2
    assert torch.equal(sites[0], sites2[0]) and torch.equal(sites[1], sites2[1])
    outf, sitesf, statf = _call(plan, gpu_device, case, with_grad=False)
    assert statf == stat and torch.equal(sitesf[0], sites[0]) and torch.equal(sitesf[1], sites[1])
    assert abs(float(outf.cpu()[_lib.OUT_NLL]) - ref["nll"]) <= NLL_BOUND * abs(ref["nll"]) and torch.all(outf.cpu()[_lib.OUT_DTHETA:] == 0)


@pytest.mark.parametrize("n", SIZES)
def test_diagonal_pass_against_the_fit_step_and_the_oracle(gpu_device, n):
    d, frac, seed = 2 + (n % 2), 0.3, 300 + n
    case = ivt._case(n, d, frac, seed)
    ref = _reference(n, d, frac, seed)
    theta, m = case[6], case[5]
    plan = base._plan(case[0], n, d, gpu_device)
    _out, _dr, sites, _stat = _call(plan, gpu_device, case)
    k_ep = plan.ep_diag().cpu().numpy()  # from the factorisation the EP call left
    (md,) = _dev(gpu_device, m)
    _o, alpha, dnoise = plan.fit_step(theta, (sites[0] - md).contiguous(), sites[1])
    k = plan.ep_diag().cpu().numpy()
    k_step = (2.0 * dnoise + alpha * alpha).cpu().numpy()
    e_step, e_ref = float(np.max(np.abs(k - k_step) / k_step)), float(np.max(np.abs(k - ref["k"]) / ref["k"]))
    print(f"ep_diag n={n}: against 2 dnoise + alpha^2 {e_step:.2e}, against the oracle's diag {e_ref:.2e}")
    assert np.array_equal(k, k_ep)
    assert e_step <= 1e-12 and e_ref <= 1e-9


def test_no_censored_row_is_the_plain_step_bitwise(gpu_device):
    n, d = 130, 2
    model, X, y, _side, v, m, theta, _upper = ivt._case(n, d, 0.3, 430)
    side = np.zeros(n, dtype=np.int32)
    case = (model, X, y, side, v, m, theta, np.full(n, np.nan))
    plan = base._plan(model, n, d, gpu_device)
    out, dr, sites, stat = _call(plan, gpu_device, case)
    alpha_buf = plan.buffer(_lib.BUF_ALPHA).clone()
    yd, vd, md = _dev(gpu_device, y, v, m)
    out0, dr0, _dn = plan.fit_step(theta, (yd - md).contiguous(), vd)
    assert stat == (0.0,) * 6
    assert torch.equal(out, out0) and torch.equal(dr, dr0) and torch.equal(alpha_buf, plan.buffer(_lib.BUF_ALPHA))
    assert torch.equal(sites[0], yd) and torch.equal(sites[1], vd)
    outf, _s, _st = _call(plan, gpu_device, case, with_grad=False)
    assert torch.equal(outf, plan.factorize(theta, (yd - md).contiguous(), vd))


def test_warm_start_at_the_converged_sites(gpu_device):
    """The sites converged to 1e-12 pass the default test (1e-10) in the first sweep, and come back untouched."""
    n, d, frac, seed = 257, 3, 0.3, 557
    case = ivt._case(n, d, frac, seed)
    plan = base._plan(case[0], n, d, gpu_device)
    out, _dr, sites, stat = _call(plan, gpu_device, case)
    out2, _dr2, sites2, stat2 = _call(plan, gpu_device, case, sites=sites, tol=1e-10)
    print(f"ep warm start: cold {stat[0]:.0f} sweeps, warm {stat2[0]:.0f} (first-sweep tests {stat2[1]:.1e}, {stat2[2]:.1e})")
    assert stat[0] >= 3 and stat2[0] == 1.0
    assert torch.equal(sites2[0], sites[0]) and torch.equal(sites2[1], sites[1]) and torch.equal(out2, out)


def _raw(plan, dev, case, maxit=100, damping=1.0, tol=TOL):
    """``dgp_ep_fit_step`` through ctypes, as it is: -> (return code, out, sites, stat, error text)."""
    _model, _X, y, side, v, m, theta, upper = case
    lib = plan.lib
    yd, vd, md, sd, ud = _dev(dev, y, v, m, side, upper)
    yt, nt = torch.zeros_like(yd), torch.zeros_like(yd)
    th = (C.c_double * len(theta))(*theta.tolist())
    need = max(int(lib.dgp_ep_workspace_bytes(plan._h)), 1 << 16)
    work = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    wbase = work.data_ptr() + (-work.data_ptr()) % 256
    out = torch.zeros(_lib.OUT_LEN, dtype=torch.float64, device=dev)
    dr = torch.zeros(len(y), dtype=torch.float64, device=dev)
    stat = (C.c_double * 6)()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with torch.cuda.device(dev):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.dgp_ep_fit_step(plan._h, th, ptr(yd), ptr(md), ptr(vd), ptr(sd), ptr(ud), ptr(yt), ptr(nt), 1, maxit, tol, damping,
                                 C.c_void_p(wbase), need, ptr(out), ptr(dr), stat, None, None, None, s)
        torch.cuda.synchronize(dev)
    return rc, out.cpu(), (yt.cpu(), nt.cpu()), tuple(stat), lib.dgp_last_error().decode()


def test_error_rules(gpu_device):
    n, d, frac, seed = 130, 2, 0.3, 430
    case = ivt._case(n, d, frac, seed)
    ref = _reference(n, d, frac, seed)
    plan = base._plan("loadest", n, d, gpu_device)
    plan.set_inputs(case[1].to(gpu_device).contiguous())
    for other in (base._plan("loadest", n, d, gpu_device, dtype=torch.float32), base._plan("loadest", n, d, gpu_device, batch=2)):
        rc, _o, _s, _st, msg = _raw(other, gpu_device, case)
        assert rc == _lib.E_ARG and "float64 single-site" in msg
    for bad in (0.0, 1.5, float("nan")):
        rc, _o, _s, _st, msg = _raw(plan, gpu_device, case, damping=bad)
        assert rc == _lib.E_ARG and "damping" in msg
    up = case[7].copy()
    row = int(np.flatnonzero(case[3] == 2)[0])
    up[row] = case[2][row] - 1.0  # not above y
    rc, _o, _s, _st, msg = _raw(plan, gpu_device, case[:7] + (up,))
    assert rc == _lib.E_ARG and "bracket" in msg
    sd = case[3].copy()
    sd[3] = 5
    rc, _o, _s, _st, msg = _raw(plan, gpu_device, case[:3] + (sd,) + case[4:])
    assert rc == _lib.E_ARG and "side" in msg
    # one sweep from cold is not enough: a return code, everything filled, the sites are the ones that were factorised
    rc, out, sites, stat, msg = _raw(plan, gpu_device, case, maxit=1)
    cold_y, cold_n, _c = eh.cold_sites(case[2], case[3], case[4], case[5], case[7])
    assert rc == _lib.E_NOCONV and "converge" in msg and stat[0] == 1.0 and max(stat[1], stat[2]) > TOL
    assert np.isfinite(float(out[_lib.OUT_NLL])) and int(out[_lib.OUT_INFO]) == 0 and stat[5] == float((case[3] != 0).sum())
    assert float(np.max(np.abs(sites[0].numpy() - cold_y))) <= 1e-12 and float(np.max(np.abs(sites[1].numpy() - cold_n) / cold_n)) <= 1e-10
    with pytest.raises(_lib.DGPError) as err:
        _call(plan, gpu_device, case, maxit=1)
    assert err.value.code == _lib.E_NOCONV and plan.ep_stat[0] == 1.0
    out, dr, sites, stat = _call(plan, gpu_device, case)  # the plan stays usable
    assert max(_errors(out, dr, sites, ref, plan.ntheta)) <= 1e-6
    # damped sweeps reach the same fixed point
    outd, drd, sitesd, statd = _call(plan, gpu_device, case, damping=0.8, tol=1e-10)
    print(f"ep damping 0.8: {statd[0]:.0f} sweeps against {stat[0]:.0f}")
    # (both stopped when their means moved by less than tol per sweep: at a linear rate rho < 0.999 that is within 1e3 tol of the fixed point)
    mu, mud = sites[0] - sites[1] * dr, sitesd[0] - sitesd[1] * drd
    assert float((mud - mu).abs().max()) <= 1e-7 and abs(float(outd[0]) - float(out[0])) <= 1e-7 * abs(float(out[0]))


def test_uninformative_row_is_capped(gpu_device):
    """A left-censored limit 12 sigma above the fit says nothing: its site sits at the cap, it is counted, and the predictions are
    those of the record without the row.  Under EP a row is judged at the standard deviation of its TILTED argument,
    s = sqrt(v + v_c) (here v_c is about 125 v: 12 noise sigma would be one s, an informative limit), so sigma is taken as the
    prior predictive standard deviation sqrt(K_ii + v), which bounds s from above."""
    n, d = 130, 2
    model, X, y, side, v, m, theta, upper = ivt._case(n, d, 0.3, 430)
    y, side, upper = y.copy(), side.copy(), upper.copy()
    row = 60
    sigma = float(np.sqrt(ch.gram(model, X, theta)[row, row] + v[row]))
    y[row], side[row], upper[row] = ch.curve(X.numpy())[row] + 12.0 * sigma, -1, np.nan
    case = (model, X, y, side, v, m, theta, upper)
    ref = eh.ep_fit(model, X, y, side, v, m, theta, upper=upper, tol=TOL)
    assert ref["converged"] and ref["stat"][3] == 1.0
    plan = base._plan(model, n, d, gpu_device)
    out, dr, sites, stat = _call(plan, gpu_device, case)
    assert stat[3] == 1.0 and stat[4] == 0.0
    assert abs(float(sites[1][row]) * ch.CAP / float(v[row]) - 1.0) <= 1e-12
    Xs = torch.tensor(orc.synth_loadest(50, d, seed=99)[0]).to(gpu_device)
    mu, var = (t.cpu().clone() for t in plan.predict(theta, Xs))
    keep = np.arange(n) != row
    small = base._plan(model, n - 1, d, gpu_device)
    _call(small, gpu_device, (model, X[keep], y[keep], side[keep], v[keep], m[keep], theta, upper[keep]))
    mu1, var1 = (t.cpu() for t in small.predict(theta, Xs))
    print(f"ep capped row: prediction against the fit without it: mean {float((mu - mu1).abs().max()):.2e}, var {float((var - var1).abs().max()):.2e}")
    assert float((mu - mu1).abs().max()) <= 1e-8 and float((var - var1).abs().max()) <= 1e-8


def test_engine_fit_with_expectation_propagation(gpu_device):
    """``LoadestGP.fit(approximation="ep", iterations=5)`` on 60 observations with 20 non-detects against the same fit on the dense
    restatement (``EPOraclePlan``): parameters and ``predict`` within the bound of the censored engine test (1e-8); ``predict``
    equals ``GPPlan.predict`` on the returned sites bitwise."""
    from discontinuum_amd.loadest_gp import LoadestGP
    from tests.flux_helpers import daily_loadest

    class CpuRef(LoadestGP):
        _plan_factory = staticmethod(eh.EPOraclePlan)
        device = "cpu"

    cov_obs, target, daily = daily_loadest(n_obs=60, end="2013-01-01", seed=7)
    vals = np.asarray(target.values, dtype=np.float64)
    order = np.argsort(vals)
    mask = np.zeros(60, dtype=bool)
    mask[order[:20]] = True
    reported = vals.copy()
    reported[mask] = vals[order[20]]
    reported = type(target)(reported, dims=target.dims, coords=target.coords, name=target.name, attrs=target.attrs)
    torch.manual_seed(0)
    model = LoadestGP()
    model.fit(cov_obs, reported, iterations=5, censored=mask, approximation="ep")
    sweeps, dmu, dtau, _capped, held, ncens = model.ep_status_
    print(f"engine EP fit: last call {sweeps:.0f} sweeps, d_mu {dmu:.1e}, d_tau {dtau:.1e}")
    assert ncens == 20 and held == 0 and sweeps <= 30 and max(dmu, dtau) <= model.laplace_tol and model.laplace_status_ is None
    torch.manual_seed(0)
    cpu = CpuRef()
    cpu.fit(cov_obs, reported, iterations=5, censored=mask, approximation="ep")
    pg = torch.cat([p.detach().reshape(-1) for p in model.model.parameters()])
    pc = torch.cat([p.detach().reshape(-1) for p in cpu.model.parameters()])
    e_par = float(((pg - pc).abs() / pc.abs().clamp_min(1.0)).max())
    got, ref = model.predict(daily)[0].values, cpu.predict(daily)[0].values
    e_pred = float(np.max(np.abs(got - ref) / np.abs(ref)))
    print(f"engine EP fit against the dense restatement: parameters {e_par:.2e}, predict {e_pred:.2e}")
    assert e_par <= 1e-8 and e_pred <= 1e-8
    # the held factorisation IS the regression on the returned sites
    x = torch.tensor(model.dm.Xnew(daily), dtype=model.dtype).to(gpu_device).contiguous()
    mu, var = model._model_space_predict(x)
    yt, nt = model._censor.sites
    spec = model._prior()
    plain = base._plan("loadest", 60, x.shape[1], gpu_device)
    plain.set_inputs(model._train_x)
    plain.factorize(model._factor_theta, (yt - spec.mean.detach()).contiguous(), nt)
    kmean, kvar = plain.predict(model._factor_theta, x)
    assert torch.equal(mu, kmean + model.model.prior_mean(x))
    assert torch.equal(var, kvar + model.likelihood.predictive_noise(x.shape[0], x.device, model.dtype))
    buf = io.BytesIO()
    model.save(buf)
    buf.seek(0)
    again = LoadestGP.load(buf, cov_obs, reported)
    assert again._censor.approximation == "ep"  # (a cold start there: the same fixed point to the tolerance, not bitwise)
    assert float(np.max(np.abs(again.predict(daily)[0].values - got) / np.abs(got))) <= 1e-7
