"""The leave-one-out training objective on the device (``dgp_loo_fit_step`` / ``dgp_loo_value``) against its dense restatement
(tests/loo_helpers.py: torch fp64 on the oracle's Gram matrix, gradients by autograd).  The bounds are the ones
tests/test_gpu_stages.py holds ``dgp_fit_step`` to against the oracle: value relative 1e-10, dtheta 1e-8 of its max-norm, dr /
dnoise relative 1e-8, the reduced slots 1e-8 of their absolute sums."""
import ctypes as C

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from tests import composite_helpers as ch
from tests.loo_helpers import LooOraclePlan, loo_value_and_grads
from tests.test_gpu_stages import make_case, plan_for

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 127, 130, 257)
PLAN_CASES = [(m, d, n) for m, d in (("loadest", 2), ("loadest", 3), ("rating", 2)) for n in SIZES]


def _case(model, d, n, seed=0):
    X, r, noise, theta = make_case(model, d, n, seed=seed, perturb=0.2)
    return X, torch.nan_to_num(r, nan=0.3), noise, theta  # (y is standardised: undefined for one observation)


def _weights(n, seed=1):
    return 0.2 + torch.rand(2, n, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def _check(model, X, r, noise, theta, w, out, dr, dnoise, label=""):
    """-> the worst error per column, each asserted against its bound."""
    val, g_theta, g_r, g_noise = loo_value_and_grads(model, X, r, noise, theta)
    out, dr, dnoise = out.cpu(), dr.cpu(), dnoise.cpu()
    P, n = theta.numel(), r.numel()
    errs = {
        "value": (abs(out[_lib.OUT_NLL] - val) / abs(val)).item(),
        "dtheta": ((out[_lib.OUT_DTHETA:_lib.OUT_DTHETA + P] - g_theta).abs().max() / g_theta.abs().max()).item(),
        "dr": ((dr[:n] - g_r).abs().max() / g_r.abs().max()).item(),
        "dnoise": ((dnoise[:n] - g_noise).abs().max() / g_noise.abs().max()).item(),
        "sum_dr": (abs(out[_lib.OUT_SUM_DR] - g_r.sum()) / g_r.abs().sum()).item(),
        "dr_w0": (abs(out[_lib.OUT_DR_W0] - (g_r * w[0]).sum()) / (g_r * w[0]).abs().sum()).item(),
        "dr_w1": (abs(out[_lib.OUT_DR_W0 + 1] - (g_r * w[1]).sum()) / (g_r * w[1]).abs().sum()).item(),
        "sum_dnoise": (abs(out[_lib.OUT_SUM_DNOISE] - g_noise.sum()) / g_noise.abs().sum()).item(),
    }
    print("loo errors", label, {k: f"{v:.2e}" for k, v in errs.items()})
    assert int(out[_lib.OUT_INFO]) == 0
    assert errs["value"] < 1e-10, errs
    for k in ("dtheta", "dr", "dnoise", "sum_dr", "dr_w0", "dr_w1", "sum_dnoise"):
        assert errs[k] < 1e-8, (k, errs)
    assert bool((out[_lib.OUT_DTHETA + P:_lib.OUT_SUM_DR] == 0).all())
    return errs


@pytest.mark.parametrize("model,d,n", PLAN_CASES)
def test_plan_level_against_the_restatement(model, d, n, gpu_device):
    """Measured on MI355X, worst over these cases: value 2.1e-14, dtheta 4.5e-14, dr 5.1e-13, dnoise 1.3e-12, reduced slots 1.0e-13
    ("Leave-one-out training objective")."""
    dev = gpu_device
    X, r, noise, theta = _case(model, d, n)
    w = _weights(n)
    p = plan_for(model, d, n, X, torch.float64, dev)
    p.set_dr_weights(w.to(dev).contiguous())
    out, dr, dnoise = p.loo_fit_step(theta, r.to(dev), noise.to(dev))
    _check(model, X, r, noise, theta, w, out, dr, dnoise, f"{model} d={d} n={n}")


@pytest.mark.parametrize("max_tiles", [0, 1000000])
def test_both_tile_cores_at_three_by_three_tiles(max_tiles, gpu_device):
    """n = 257 (N = 384): the 128 x 128 direct-to-LDS core (selector 0) and the 64 x 64 register-staged one, forced."""
    dev = gpu_device
    X, r, noise, theta = _case("loadest", 3, 257, seed=4)
    w = _weights(257)
    p = plan_for("loadest", 3, 257, X, torch.float64, dev)
    p.set_option(_lib.OPT_LAUUM64_MAX_TILES, max_tiles)
    p.set_dr_weights(w.to(dev).contiguous())
    out, dr, dnoise = p.loo_fit_step(theta, r.to(dev), noise.to(dev))
    _check("loadest", X, r, noise, theta, w, out, dr, dnoise, f"selector {max_tiles}")


def test_composite_tree(gpu_device):
    dev = gpu_device
    idx = ch.HAND_BUILT[0]
    case = ch.CASES[idx]
    name = ch.define(case.spec)
    n = 130
    X, r, noise = ch.data(idx, n)
    w = _weights(n)
    p = plan_for(name, case.d, n, X, torch.float64, dev)
    p.set_dr_weights(w.to(dev).contiguous())
    out, dr, dnoise = p.loo_fit_step(case.theta, r.to(dev), noise.to(dev))
    _check(name, X, r, noise, case.theta, w, out, dr, dnoise, case.name)


@pytest.mark.parametrize("sizes", [(130, 64, 257), (130, 64, 257, 1, 2, 127, 128, 129, 200, 33, 256)])
def test_ragged_batch_matches_single_site_plans(sizes, gpu_device):
    """3 sites, and 11 (hyperparameters from the device array); NaN in every unused tail."""
    from discontinuum_amd.backend import GPPlan

    dev = gpu_device
    model, d, B, n = "loadest", 3, len(sizes), max(sizes)
    cases = [_case(model, d, nb, seed=10 + b) for b, nb in enumerate(sizes)]
    X = torch.full((B, n, d), float("nan"), dtype=torch.float64)
    r = torch.full((B, n), float("nan"), dtype=torch.float64)
    noise = torch.full((B, n), float("nan"), dtype=torch.float64)
    w = torch.full((B, 2, n), float("nan"), dtype=torch.float64)
    ws = [_weights(nb, seed=b) for b, nb in enumerate(sizes)]
    for b, (nb, c) in enumerate(zip(sizes, cases)):
        X[b, :nb], r[b, :nb], noise[b, :nb], w[b, :, :nb] = c[0], c[1], c[2], ws[b]
    theta = torch.stack([c[3] for c in cases])
    pb = GPPlan(model, n, d, device=dev, lookahead=1, batch=B)
    pb.set_site_sizes(sizes)
    pb.set_inputs(X.to(dev).contiguous())
    pb.set_dr_weights(w.to(dev).contiguous())
    out, dr, dnoise = [t.cpu() for t in pb.loo_fit_step(theta, r.to(dev).contiguous(), noise.to(dev).contiguous())]
    val2 = pb.loo_value().cpu()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dr).all()) and bool(torch.isfinite(dnoise).all())
    P = pb.ntheta
    for b, (nb, c) in enumerate(zip(sizes, cases)):
        _check(model, c[0], c[1], c[2], c[3], ws[b], out[b], dr[b], dnoise[b], f"site {b} n={nb}")
        assert bool((dr[b, nb:] == 0).all()) and bool((dnoise[b, nb:] == 0).all())
        assert val2[b, 0] == out[b, _lib.OUT_NLL] and val2[b, 1] == 0
        p1 = plan_for(model, d, nb, c[0], torch.float64, dev, lookahead=1)
        p1.set_dr_weights(ws[b].to(dev).contiguous())
        o1, a1, n1 = [t.cpu() for t in p1.loo_fit_step(c[3], c[1].to(dev), c[2].to(dev))]
        assert abs(out[b, 0] - o1[0]) <= 1e-10 * abs(o1[0])
        assert (out[b, 4:4 + P] - o1[4:4 + P]).abs().max() <= 1e-10 * max(1.0, o1[4:4 + P].abs().max().item())
        assert (dr[b, :nb] - a1).abs().max() <= 1e-10 * a1.abs().max()
        assert (dnoise[b, :nb] - n1).abs().max() <= 1e-10 * n1.abs().max()


def test_repeatable_and_leaves_the_plan_as_fit_step_does(gpu_device):
    dev = gpu_device
    model, d, n = "rating", 2, 257
    X, r, noise, theta = _case(model, d, n, seed=2)
    Xs = X[:50].to(dev).contiguous()
    rd, nd = r.to(dev), noise.to(dev)
    p = plan_for(model, d, n, X, torch.float64, dev)
    f_out, _f_dr, _f_dn = [t.clone() for t in p.fit_step(theta, rd, nd)]
    alpha0 = p.buffer(_lib.BUF_ALPHA).clone()
    S0, T0 = p.buffer(_lib.BUF_S).clone(), p.buffer(_lib.BUF_T).clone()
    pred0 = [t.clone() for t in p.predict(theta, Xs)]
    first = [t.clone() for t in p.loo_fit_step(theta, rd, nd)]
    assert torch.equal(p.buffer(_lib.BUF_ALPHA), alpha0)
    assert torch.equal(torch.tril(p.buffer(_lib.BUF_S)[:n, :n]), torch.tril(S0[:n, :n]))
    assert torch.equal(torch.tril(p.buffer(_lib.BUF_T)[:n, :n]), torch.tril(T0[:n, :n]))
    pred1 = p.predict(theta, Xs)
    assert torch.equal(pred0[0], pred1[0]) and torch.equal(pred0[1], pred1[1])
    for k in (_lib.OUT_QUAD, _lib.OUT_LOGDET, _lib.OUT_INFO):
        assert first[0][k] == f_out[k]
    second = p.loo_fit_step(theta, rd, nd)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    cv = p.cross_validate(torch.arange(n))  # every other product still works on the plan
    assert bool(torch.isfinite(cv[2]).all())


@pytest.mark.parametrize("n", [130, 257])
def test_value_agrees_with_cross_validation(n, gpu_device):
    """Two independent device paths: loo_value = -sum lpd of the folds of one of dgp_cross_validate."""
    dev = gpu_device
    X, r, noise, theta = _case("loadest", 3, n, seed=5)
    p = plan_for("loadest", 3, n, X, torch.float64, dev)
    out = p.loo_fit_step(theta, r.to(dev), noise.to(dev))[0]
    val = p.loo_value().cpu()
    _resid, _var, lpd, info = p.cross_validate(torch.arange(n))
    ref = -lpd.sum().item()
    assert int(info.abs().max()) == 0 and val[1] == 0
    assert abs(val[0].item() - ref) <= 1e-10 * abs(ref)
    assert val[0] == out[_lib.OUT_NLL].cpu()
    out_f = p.fit_step(theta, r.to(dev), noise.to(dev))[0]  # ... and from the inverse a plain fit step leaves
    assert p.loo_value().cpu()[0] == val[0] and torch.isfinite(out_f[0])


def test_errors_and_a_site_that_is_not_positive_definite(gpu_device):
    from discontinuum_amd.backend import GPPlan

    dev = gpu_device
    model, d, n = "loadest", 3, 130
    X, r, noise, theta = _case(model, d, n, seed=6)
    p = plan_for(model, d, n, X, torch.float64, dev)
    lib = p.lib
    with pytest.raises(Exception, match="K\\^\\^-1|inverse"):  # no factorisation yet
        p.loo_value()
    p.factorize(theta, r.to(dev), noise.to(dev))  # a factorisation without S
    with pytest.raises(Exception, match="K\\^\\^-1|inverse"):
        p.loo_value()
    need = int(lib.dgp_loo_workspace_bytes(p._h))
    assert need >= 3 * p.N * p.N * 8
    work = torch.empty(need + 512, dtype=torch.uint8, device=dev)
    base = work.data_ptr() + (-work.data_ptr()) % 256
    out = torch.full((_lib.OUT_LEN,), 7.0, dtype=torch.float64, device=dev)
    th = (C.c_double * p.ntheta)(*theta.tolist())
    rd, nd = r.to(dev), noise.to(dev)

    def call(ptr, nbytes):
        with torch.cuda.device(dev):
            return lib.dgp_loo_fit_step(p._h, th, C.c_void_p(rd.data_ptr()), C.c_void_p(nd.data_ptr()), C.c_void_p(ptr), nbytes,
                                        C.c_void_p(out.data_ptr()), None, None, C.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert call(base, need - 1) == -3 and call(0, need) == -3  # DGP_E_WORKSPACE
    assert call(base + 8, need) == -1 and b"aligned" in lib.dgp_last_error()
    assert lib.dgp_loo_fit_step(p._h, None, None, None, C.c_void_p(base), need, None, None, None, None) == -1
    torch.cuda.synchronize(dev)
    assert bool((out == 7.0).all())  # nothing was launched
    assert call(base, need) == 0  # dr / dnoise are optional, as for dgp_fit_step
    torch.cuda.synchronize(dev)
    assert torch.equal(out, p.loo_fit_step(theta, rd, nd)[0])
    p32 = plan_for(model, d, n, X, torch.float32, dev)
    assert lib.dgp_loo_workspace_bytes(p32._h) == 0
    with pytest.raises(Exception, match="float64"):
        p32.loo_fit_step(theta, r.float().to(dev), noise.float().to(dev))
    # a matrix that is not positive definite, by the route of test_not_positive_definite_every_schedule_terminates: handled
    Xb = X.clone()
    Xb[40] = Xb[41]
    bad = noise.clone()
    bad[40] = bad[41] = -0.5
    pb = GPPlan(model, n, d, device=dev, lookahead=1, batch=2)
    pb.set_inputs(torch.stack([Xb, X]).to(dev).contiguous())
    o2, dr2, dn2 = pb.loo_fit_step(theta.repeat(2, 1), torch.stack([r, r]).to(dev).contiguous(), torch.stack([bad, noise]).to(dev).contiguous())
    o2 = o2.cpu()
    f2 = pb.fit_step(theta.repeat(2, 1), torch.stack([r, r]).to(dev).contiguous(), torch.stack([bad, noise]).to(dev).contiguous())[0].cpu()
    assert o2[0, _lib.OUT_INFO] >= 1 and o2[0, _lib.OUT_INFO] == f2[0, _lib.OUT_INFO] and not torch.isfinite(o2[0, _lib.OUT_NLL])
    good = p.loo_fit_step(theta, rd, nd)
    assert o2[1, _lib.OUT_INFO] == 0
    assert torch.equal(o2[1], good[0].cpu()) and torch.equal(dr2[1].cpu(), good[1].cpu()) and torch.equal(dn2[1].cpu(), good[2].cpu())


def test_engine_fit_against_the_double(gpu_device):
    from discontinuum_amd.loadest_gp import LoadestGP
    from tests.helpers import loadest_dataset

    cov, tgt = loadest_dataset(n=120, seed=3)[:2]
    traces = {}
    models = {}
    for kind in ("gpu", "double"):
        torch.manual_seed(0)
        m = LoadestGP()
        if kind == "double":
            m.device = "cpu"
            m._plan_factory = LooOraclePlan
        trace = []
        import discontinuum_amd.gp.explicit as ex

        orig = ex.ExplicitObjective.evaluate

        def spy(self, *a, _orig=orig, _trace=trace, **k):
            v = _orig(self, *a, **k)
            _trace.append(v)
            return v

        ex.ExplicitObjective.evaluate = spy
        try:
            m.fit(cov, tgt, iterations=5, objective="loo")
        finally:
            ex.ExplicitObjective.evaluate = orig
        traces[kind], models[kind] = np.asarray(trace), m
    assert len(traces["gpu"]) == 5 and models["gpu"].objective_ == "loo"
    np.testing.assert_allclose(traces["gpu"], traces["double"], rtol=1e-7)
    mu_g, se_g = models["gpu"].predict(cov)
    mu_d, se_d = models["double"].predict(cov)
    np.testing.assert_allclose(mu_g.values, mu_d.values, rtol=1e-7)
    np.testing.assert_allclose(se_g.values, se_d.values, rtol=1e-7)
    # -elpd of cross_validate("loo") at the final hyperparameters = the data term of an objective evaluated there
    m = models["gpu"]
    cv = m.cross_validate("loo")
    from discontinuum_amd.gp.mll import ExactMarginalLogLikelihood

    mll = ExactMarginalLogLikelihood(m.likelihood, m.model)
    with torch.no_grad():
        total = float(-mll(m._prior(), m._train_y)) * 120 + float(mll.log_prior())
    np.testing.assert_allclose(-cv.attrs["elpd"], total, rtol=1e-7)
