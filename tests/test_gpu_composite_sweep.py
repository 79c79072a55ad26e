"""Seeded random kernel trees (tests/composite_helpers.py) through every model-dependent kernel of the library on the generic
interpreted evaluator (``csrc/dgp_models.h::Composite``): Gram, fit step, prediction, additive parts, input slopes, Fisher
information, streamed period moments, the mean's VJP, batches of 10 ragged sites (hyperparameters through the device scratch),
float32 plans with and without the fp64 refinement, two structures in alternation, and the distributed slab path.

Bounds are the project's own.  fp64 (tests/test_gpu_stages.py, tests/test_gpu_sweep.py): Gram 1e-13 absolute, NLL 1e-10
relative, gradients / alpha / dnoise 1e-8 relative, posterior mean 1e-9, variance 1e-8, parts and slopes 1e-9 / 1e-8 of their
scales with the parts summing to ``predict`` at 1e-12 / 1e-11 (tests/test_gpu_terms.py, tests/test_gpu_slopes.py), Fisher
``scaled_error`` 1e-8 (tests/test_gpu_fisher.py), the mean's VJP 1e-7 (tests/test_gpu_composite.py).  fp32 (SURVEY section 8d
as used in tests/test_gpu_stages.py): NLL 1e-4 max(1, n / 1024) relative, gradients 1e-2 relative, mean and variance 1e-3.  A
site of a batch against its single-site plan: 1e-11 of scale in fp64, as in the existing ragged-batch tests; in fp32 the
batched factorisation may round differently from the single-site one (tests/test_gpu_stages.py
``test_batched_plan_fp32_matches_single_site_plans``), and both are within the fp32 bounds of the same exact answer, so the
sites are compared at those: 1e-3 of scale for means and (co)variances, 1e-2 for the Fisher information and the VJP.  A site
mix-up or a wrong scratch slot is an O(1) error under either.  Every printed figure is a measurement, the assertions are the
bounds."""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as orc
from tests import composite_helpers as H
from tests.fisher_helpers import dense_fisher, scaled_error
from tests.slopes_helpers import PRIORS, composite_prior
from tests.terms_helpers import pack_cov, unpack_cov
from tests.test_gpu_stages import make_case

pytestmark = pytest.mark.gpu

SIZES = (1, 300, 128, 129, 17, 257, 64, 200, 33, 130)  # a ragged batch of 10: more sites than the kernel arguments carry


def _nan_ws(p, attr, need):
    """Hand the plan a work area for one product whose every byte is 0xFF (NaN in both dtypes)."""
    setattr(p, attr, torch.full((int(need) + 256,), 255, dtype=torch.uint8, device=p.device))


def _nan_all(p, m, ncols, E=1, P=3):
    lib, h = p.lib, p._h
    _nan_ws(p, "_pred_ws", lib.dgp_predict_workspace_bytes(h, m))
    _nan_ws(p, "_terms_ws", lib.dgp_predict_terms_workspace_bytes(h, m))
    if ncols:
        _nan_ws(p, "_slopes_ws", lib.dgp_predict_slopes_workspace_bytes(h, m, ncols))
    _nan_ws(p, "_fisher_ws", lib.dgp_fisher_workspace_bytes(h, E))
    _nan_ws(p, "_vjp_ws", lib.dgp_mean_vjp_workspace_bytes(h, m))
    _nan_ws(p, "_ppm_ws", lib.dgp_posterior_period_moments_workspace_bytes(h, m, P))


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max()).item() if b.numel() and float(b.abs().max()) > 0 else float((a - b).abs().max())


def _plan(name, n, d, X, dtype, dev, lookahead=True):
    from discontinuum_amd.backend import GPPlan

    p = GPPlan(name, n, d, dtype=dtype, device=dev, lookahead=lookahead)
    p.set_inputs(X.to(dev, dtype).contiguous())
    return p


def _fit_errors(out, dr, dnoise, ref, P):
    """(NLL, dtheta, dr, dnoise) errors of one site's fit step, each relative to the reference's largest entry."""
    from discontinuum_amd import _lib

    val, g_theta, g_r, g_noise = ref
    out = out.cpu().double()
    assert out[_lib.OUT_INFO] == 0
    return (abs(out[_lib.OUT_NLL].item() - val.item()) / abs(val.item()),
            _rel(out[_lib.OUT_DTHETA:_lib.OUT_DTHETA + P], g_theta), _rel(dr, g_r), _rel(dnoise, g_noise))


def _fit_and_predict(i, n, m, dev, edge=False):
    """Gram, fit step at a lookahead level drawn per case, factorize and predict of case i against the oracle; -> (plan, ...)
    for the products that follow.  ``edge``: the duplicated and the period-shifted training rows, and eight test points that
    EQUAL training rows (those among them)."""
    from discontinuum_amd import _lib

    case = H.CASES[i]
    name, d, theta, P = H.define(case.spec), case.d, case.theta, case.ntheta
    X, r, noise = H.data(i, n, edge)
    Xs = H.query_points(i, m, coincide=min(8, m) if edge else 0, n=n, edge=edge)
    level = int(np.random.default_rng(i).integers(0, 3))
    p = _plan(name, n, d, X, torch.float64, dev, lookahead=level)
    assert p.ntheta == P and p.nterms == len(case.terms)
    tag = f"{case.name} n={n} m={m}{' edge' if edge else ''} lookahead={level}"
    p.stage_gram(theta, noise.to(dev))
    Khat = H.gram_of(case)(X, X, theta) + torch.diag(noise)
    e_k = (torch.tril(p.buffer(_lib.BUF_A)[:n, :n]).cpu() - torch.tril(Khat)).abs().max().item()
    print(f"sweep gram fp64 {tag}: {e_k:.2e}")
    assert e_k < 1e-13, (tag, e_k)
    ref = orc.nll_data_and_grads(name, X, r, noise, theta)
    out, dr, dnoise = p.fit_step(theta, r.to(dev), noise.to(dev))
    e = _fit_errors(out, dr, dnoise, ref, P)
    print(f"sweep fit_step fp64 {tag}: nll {e[0]:.2e} dtheta {e[1]:.2e} dr {e[2]:.2e} dnoise {e[3]:.2e}")
    assert e[0] <= 1e-10 and e[1] <= 1e-8 and e[2] <= 1e-8 and e[3] <= 1e-8, (tag, e)
    assert int(p.factorize(theta, r.to(dev), noise.to(dev)).cpu()[_lib.OUT_INFO]) == 0
    Xd = Xs.to(dev).contiguous()
    _nan_ws(p, "_pred_ws", p.lib.dgp_predict_workspace_bytes(p._h, m))
    mu_ref, var_ref = orc.posterior(name, X, r, noise, theta, Xs)
    mu, var = p.predict(theta, Xd)
    e_m = (mu.cpu() - mu_ref).abs().max().item()
    e_v = ((var.cpu() - var_ref).abs() / (var_ref.abs() + 1e-4)).max().item()
    print(f"sweep predict fp64 {tag}: mean {e_m:.2e} var {e_v:.2e}")
    assert e_m < 1e-9 and e_v < 1e-8, (tag, e_m, e_v)
    return p, case, name, X, r, noise, Xs, Xd, mu, var, mu_ref, tag


SINGLE = ([(i, 129 if i % 2 else 300, 130) for i in range(len(H.CASES))]
          + [(i, n, 130) for i in range(3) for n in (1, 63)] + [(3, 129, 1)])


@pytest.mark.parametrize("i,n,m", SINGLE, ids=[f"{H.CASES[i].name} n={n} m={m}" for i, n, m in SINGLE])
def test_single_site_fp64(i, n, m, gpu_device):
    dev = gpu_device
    p, case, name, X, r, noise, Xs, Xd, mu, var, mu_ref, tag = _fit_and_predict(i, n, m, dev)
    theta, d, P = case.theta, case.d, case.ntheta
    cols = H.differentiable_columns(case.spec)
    _nan_all(p, m, len(cols))
    # the additive parts, against one-term descriptions, and their sum against predict on the same plan
    ref_mean, ref_cov, scale = H.parts_reference(case, X, r, noise, Xs)
    mean, cov = p.predict_terms(theta, Xd)
    C = len(case.terms)
    assert mean.shape == (C, m) and cov.shape == (C * (C + 1) // 2, m)
    e_m = ((mean.cpu() - ref_mean).abs().max() / ref_mean.abs().max().clamp(min=1.0)).item()
    e_c = ((cov.cpu() - pack_cov(ref_cov)).abs().max() / scale).item()
    i_m = (mean.sum(0) - mu).abs().max().item() / max(1.0, ref_mean.abs().max().item())
    i_c = (unpack_cov(cov.cpu()).sum((0, 1)) - var.cpu()).abs().max().item() / scale
    print(f"sweep terms fp64 {tag}: mean {e_m:.2e} cov {e_c:.2e} | sum mean {i_m:.2e} sum cov {i_c:.2e}")
    assert e_m < 1e-9 and e_c < 1e-8 and i_m < 1e-12 and i_c < 1e-11, (tag, e_m, e_c, i_m, i_c)
    # value and slopes in every column the covariance is differentiable in; the others are refused
    for col in set(range(d)) - set(cols):
        with pytest.raises(ValueError, match="not differentiable"):
            p.predict_slopes(theta, Xd, [col])
    if cols:
        s_mean, s_cov, scales = H.slopes_ref(case, X, r, noise, Xs, cols)
        mean, cov = p.predict_slopes(theta, Xd, cols)
        e_m, e_c = H.plane_errors(mean, cov, s_mean, s_cov, scales)
        i_m = (mean[0] - mu).abs().max().item() / max(1.0, s_mean[0].abs().max().item())
        print(f"sweep slopes fp64 {tag} cols={cols}: mean {e_m:.2e} cov {e_c:.2e} | plane 0 vs predict {i_m:.2e}")
        assert e_m < 1e-9 and e_c < 1e-8 and i_m < 1e-12, (tag, e_m, e_c, i_m)
    # Fisher information with one diagonal direction
    dg = torch.ones(1, n, dtype=torch.float64)
    F = p.fisher(theta, dg.to(dev)).cpu()
    e_f = scaled_error(F, dense_fisher(name, X, noise, theta, dg))
    print(f"sweep fisher fp64 {tag}: {e_f:.2e}")
    assert tuple(F.shape) == (P + 1, P + 1) and torch.equal(F, F.T) and e_f <= 1e-8, (tag, e_f)
    # the mean's VJP against autograd through the oracle's posterior mean
    w = torch.randn(m, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    th, rr, nn = (t.clone().requires_grad_(True) for t in (theta, r, noise))
    gt, gr, gn = torch.autograd.grad((orc.posterior(name, X, rr, nn, th, Xs)[0] * w).sum(), (th, rr, nn))
    p.fit_step(theta, r.to(dev), noise.to(dev))  # the VJP needs K^^-1 as well: the fit step's state, not factorize's
    dtheta, dr, dn = p.mean_vjp(theta, Xd, w.to(dev))
    e = (_rel(dtheta, gt), _rel(dr, gr), _rel(dn, gn))
    print(f"sweep mean_vjp fp64 {tag}: dtheta {e[0]:.2e} dr {e[1]:.2e} dnoise {e[2]:.2e}")
    assert max(e) <= 1e-7, (tag, e)
    mu2, var2 = p.predict(theta, Xd)  # the products only read the plan
    assert torch.equal(mu2, mu) and torch.equal(var2, var)


EDGE = H.HAND_BUILT + H.RANDOM[1:6]


@pytest.mark.parametrize("i", EDGE, ids=[H.CASES[i].name for i in EDGE])
def test_edge_rows_fp64(i, gpu_device):
    """A duplicated training row, two training points exactly one period apart, and test points that equal training rows."""
    _fit_and_predict(i, 129 if i % 2 else 300, 130, gpu_device, edge=True)


FP32 = [1, 3, 5, 8, 11, 15, 25, H.BIGGEST]


@pytest.mark.parametrize("i", FP32, ids=[H.CASES[i].name for i in FP32])
def test_float32(i, gpu_device):
    """fp32 plans at n = 300: the fit step with the fp64 refinement (the fp64 evaluator and its own hyperparameter scratch)
    and without, then prediction, parts and slopes from the refined step's factorisation."""
    from discontinuum_amd import _lib

    dev, n, m, f32 = gpu_device, 300, 130, torch.float32
    case = H.CASES[i]
    name, d, theta, P = H.define(case.spec), case.d, case.theta, case.ntheta
    X, r, noise = H.data(i, n)
    Xs = H.query_points(i, m)
    ref = orc.nll_data_and_grads(name, X, r, noise, theta)
    p = _plan(name, n, d, X, f32, dev)
    assert p.get_option(_lib.OPT_REFINE) == 1
    for refine in (0, 1):
        p.set_option(_lib.OPT_REFINE, refine)
        out, dr, dnoise = p.fit_step(theta, r.to(dev, f32), noise.to(dev, f32))
        e = _fit_errors(out, dr, dnoise, ref, P)
        print(f"sweep fit_step fp32 {case.name} refine={refine}: nll {e[0]:.2e} dtheta {e[1]:.2e} dr {e[2]:.2e} dnoise {e[3]:.2e}")
        assert e[0] <= 1e-4 * max(1.0, n / 1024) and max(e[1:]) <= 1e-2, (case.name, refine, e)
    Xd = Xs.to(dev, f32).contiguous()
    cols = H.differentiable_columns(case.spec)
    _nan_all(p, m, len(cols))
    mu_ref, var_ref = orc.posterior(name, X, r, noise, theta, Xs)
    mu, var = p.predict(theta, Xd)
    e_m, e_v = (mu.cpu().double() - mu_ref).abs().max().item(), (var.cpu().double() - var_ref).abs().max().item()
    print(f"sweep predict fp32 {case.name}: mean {e_m:.2e} var {e_v:.2e}")
    assert e_m <= 1e-3 and e_v <= 1e-3, (case.name, e_m, e_v)
    ref_mean, ref_cov, scale = H.parts_reference(case, X, r, noise, Xs)
    mean, cov = p.predict_terms(theta, Xd)
    assert mean.dtype == f32 and cov.dtype == f32
    e_m = (mean.cpu().double() - ref_mean).abs().max().item()
    e_c = (cov.cpu().double() - pack_cov(ref_cov)).abs().max().item() / scale
    print(f"sweep terms fp32 {case.name}: mean {e_m:.2e} cov {e_c:.2e}")
    assert e_m <= 1e-3 and e_c <= 1e-3, (case.name, e_m, e_c)
    if cols:
        s_mean, s_cov, scales = H.slopes_ref(case, X, r, noise, Xs, cols)
        mean, cov = p.predict_slopes(theta, Xd, cols)
        e_m, e_c = H.plane_errors(mean, cov, s_mean, s_cov, scales)
        print(f"sweep slopes fp32 {case.name} cols={cols}: mean {e_m:.2e} cov {e_c:.2e}")
        assert e_m <= 1e-3 and e_c <= 1e-3, (case.name, e_m, e_c)


# ---- batches of 10 ragged sites ---------------------------------------------------------------------------------------------
def _products(p, theta, r, noise, Xs, cols, w, dg, mu_in, wts, groups, ngroups, s2):
    """``factorize``, then every inference product of the held factorisation -- the mean's VJP after a fit step at the same
    inputs, since it needs K^^-1 as well -- as CPU float64 tensors by name."""
    from discontinuum_amd import _lib
    from discontinuum_amd.backend import MODE_LOG

    out = {}
    assert bool((p.factorize(theta, r, noise)[..., _lib.OUT_INFO] == 0).all())
    out["predict.mean"], out["predict.var"] = p.predict(theta, Xs)
    pm, pc = p.posterior_cov(theta, Xs)
    m = Xs.shape[-2]
    out["posterior_cov.mean"], out["posterior_cov.cov"] = pm, torch.tril(pc[..., :m, :m])
    out["terms.mean"], out["terms.cov"] = p.predict_terms(theta, Xs)
    if cols:
        out["slopes.mean"], out["slopes.cov"] = p.predict_slopes(theta, Xs, cols)
    out["fisher"] = p.fisher(theta, dg)
    out["period_moments.mean"], out["period_moments.cov"] = p.posterior_period_moments(theta, Xs, mu_in, s2, wts, groups, ngroups, MODE_LOG)
    p.fit_step(theta, r, noise)
    out["mean_vjp.dtheta"], out["mean_vjp.dr"], out["mean_vjp.dnoise"] = p.mean_vjp(theta, Xs, w)
    return {k: v.detach().cpu().double() for k, v in out.items()}


def _batch_of_ten(name, d, sites, dtype, dev, cols, prior_fn, tag):
    """``sites``: ten (X, r, noise, theta, Xs) of the sizes SIZES.  The fit step of the ragged batched plan (NaN padding)
    against the oracle per site; then every product after ``factorize`` against ten single-site plans, twice with the same
    bits; then the state: a prediction at OTHER hyperparameters must leave no trace in the products of the held fit step
    that follow it (the same bits as before it), nor in the next fit step or staged gradient (1e-12 relative, both dtypes)."""
    from discontinuum_amd import _lib
    from discontinuum_amd.backend import GPPlan

    f64 = dtype == torch.float64
    B, n, m = len(sites), max(SIZES), sites[0][4].shape[0]
    assert tuple(s[0].shape[0] for s in sites) == SIZES
    P = sites[0][3].numel()
    X = torch.full((B, n, d), float("nan"), dtype=torch.float64)
    r = torch.full((B, n), float("nan"), dtype=torch.float64)
    noise = torch.full((B, n), float("nan"), dtype=torch.float64)
    dg = torch.full((B, 1, n), float("nan"), dtype=torch.float64)
    for b, (nb, s) in enumerate(zip(SIZES, sites)):
        X[b, :nb], r[b, :nb], noise[b, :nb], dg[b, 0, :nb] = s[0], s[1], s[2], 1.0
    theta = torch.stack([s[3] for s in sites])
    assert len({tuple(t.tolist()) for t in theta}) == B  # every site its own hyperparameters
    Xs = torch.stack([s[4] for s in sites]).to(dev, dtype).contiguous()
    gen = torch.Generator().manual_seed(7)
    w = torch.randn(B, m, dtype=torch.float64, generator=gen).to(dev, dtype).contiguous()
    mu_in = (0.3 * torch.randn(B, m, dtype=torch.float64, generator=gen)).to(dev, dtype).contiguous()
    wts = (0.5 + 1.5 * torch.rand(B, m, dtype=torch.float64, generator=gen)).to(dev)
    groups = (torch.arange(m) // 50).to(torch.int32).repeat(B, 1).to(dev).contiguous()
    ngroups = int(groups.max()) + 1
    s2 = torch.linspace(0.5, 0.9, B, dtype=torch.float64)
    rd, nd, dgd = (t.to(dev, dtype).contiguous() for t in (r, noise, dg))
    pb = GPPlan(name, n, d, dtype=dtype, device=dev, lookahead=1, batch=B)
    pb.set_site_sizes(SIZES)
    pb.set_inputs(X.to(dev, dtype).contiguous())
    out, dr, dn = pb.fit_step(theta, rd, nd)
    worst = [0.0] * 4
    for b, (nb, s) in enumerate(zip(SIZES, sites)):
        e = _fit_errors(out[b], dr[b, :nb], dn[b, :nb], orc.nll_data_and_grads(name, s[0], s[1], s[2], s[3]), P)
        bounds = (1e-10, 1e-8, 1e-8, 1e-8) if f64 else (1e-4, 1e-2, 1e-2, 1e-2)
        assert all(x <= y for x, y in zip(e, bounds)), (tag, b, nb, e)
        assert bool((dr[b, nb:] == 0).all()) and bool((dn[b, nb:] == 0).all())
        worst = [max(a, x) for a, x in zip(worst, e)]
    print(f"sweep batch fit_step {tag}: nll {worst[0]:.2e} dtheta {worst[1]:.2e} dr {worst[2]:.2e} dnoise {worst[3]:.2e} against the oracle")
    _nan_all(pb, m, len(cols), P=ngroups)
    got = _products(pb, theta, rd, nd, Xs, cols, w, dgd, mu_in, wts, groups, ngroups, s2)
    again = _products(pb, theta, rd, nd, Xs, cols, w, dgd, mu_in, wts, groups, ngroups, s2)
    for k in got:
        assert bool(torch.isfinite(got[k]).all()), (tag, k)
        assert torch.equal(got[k], again[k]), (tag, k)  # the same bits run to run
    worst = {}
    for b, (nb, s) in enumerate(zip(SIZES, sites)):
        ps = _plan(name, nb, d, s[0], dtype, dev, lookahead=1)
        one = _products(ps, s[3], s[1].to(dev, dtype), s[2].to(dev, dtype), Xs[b].contiguous(), cols, w[b].contiguous(), dgd[b, :, :nb].contiguous(), mu_in[b].contiguous(),
                        wts[b].contiguous(), groups[b].contiguous(), ngroups, float(s2[b]))
        prior = prior_fn(s[3], s[4])
        scale = float(prior[0, 0].max())  # the largest total prior variance at the site's test points
        sel = [0] + [1 + c for c in cols]
        scales = torch.sqrt(torch.stack([prior[a, a].max() for a in sel]))
        err = {}
        err["predict"] = max((got["predict.mean"][b] - one["predict.mean"]).abs().max().item() / max(1.0, one["predict.mean"].abs().max().item()),
                             (got["predict.var"][b] - one["predict.var"]).abs().max().item() / scale)
        err["posterior_cov"] = max((got["posterior_cov.mean"][b] - one["posterior_cov.mean"]).abs().max().item() / max(1.0, one["posterior_cov.mean"].abs().max().item()),
                                   (got["posterior_cov.cov"][b] - one["posterior_cov.cov"]).abs().max().item() / scale)
        err["terms"] = max((got["terms.mean"][b] - one["terms.mean"]).abs().max().item() / max(1.0, one["terms.mean"].abs().max().item()),
                           (got["terms.cov"][b] - one["terms.cov"]).abs().max().item() / scale)
        if cols:
            err["slopes"] = max(H.plane_errors(got["slopes.mean"][b], got["slopes.cov"][b], one["slopes.mean"], unpack_cov(one["slopes.cov"]), scales))
        err["fisher"] = scaled_error(got["fisher"][b], one["fisher"])
        err["period_moments"] = max(_rel(got["period_moments.mean"][b], one["period_moments.mean"]),
                                    _rel(got["period_moments.cov"][b], one["period_moments.cov"]))
        err["mean_vjp"] = max(_rel(got["mean_vjp.dtheta"][b], one["mean_vjp.dtheta"]), _rel(got["mean_vjp.dr"][b, :nb], one["mean_vjp.dr"]),
                              _rel(got["mean_vjp.dnoise"][b, :nb], one["mean_vjp.dnoise"]))
        assert bool((got["mean_vjp.dr"][b, nb:] == 0).all()) and bool((got["mean_vjp.dnoise"][b, nb:] == 0).all())
        assert torch.equal(got["fisher"][b], got["fisher"][b].T)
        for k, v in err.items():
            bound = 1e-11 if f64 else (1e-2 if k in ("fisher", "mean_vjp") else 1e-3)
            assert v <= bound, (tag, k, b, nb, v)
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"sweep batch products {tag} against single-site plans: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    # state: fit step at theta, then a prediction at OTHER hyperparameters (every site gets another site's: it overwrites the
    # scratch copy of the hyperparameters).  The products of the HELD fit step give the bits they gave before it ...
    def held():
        return [t.clone() for t in (*pb.predict(theta, Xs), *pb.mean_vjp(theta, Xs, w))]

    first = [t.clone() for t in pb.fit_step(theta, rd, nd)]
    before = held()
    other = [t.clone() for t in pb.predict(theta.flip(0), Xs)]
    assert not torch.equal(other[0], before[0])
    after = held()
    assert all(torch.equal(a, b) for a, b in zip(after, before)), tag
    # ... and the fit step run again gives what it gave
    second = pb.fit_step(theta, rd, nd)
    e_s = max(_rel(a, b) for a, b in zip(second, first))
    print(f"sweep batch state {tag}: after a prediction at other hyperparameters: predict and mean_vjp the same bits, fit step {e_s:.2e}")
    assert e_s <= 1e-12, (tag, e_s)
    # ... and on the largest single site through the staged gradient (dgp_stage_grad serves single-site plans only)
    b = SIZES.index(max(SIZES))
    s = sites[b]
    ps = _plan(name, SIZES[b], d, s[0], dtype, dev)
    o = ps.fit_step(s[3], s[1].to(dev, dtype), s[2].to(dev, dtype))[0]
    ps.predict(sites[b - 1][3], Xs[b].contiguous())
    g = ps.stage_grad(s[3])
    e_g = _rel(g, o[_lib.OUT_DTHETA:_lib.OUT_DTHETA + P])
    print(f"sweep state {tag}: stage_grad after a prediction at other hyperparameters {e_g:.2e}")
    assert e_g <= 1e-12, (tag, e_g)


def _composite_sites(i):
    case = H.CASES[i]
    sites = []
    for b, nb in enumerate(SIZES):
        X, r, noise = H.data(i, nb, False, seed=b + 1)
        theta = H.theta_for(np.random.default_rng(77 * i + b), case.spec)
        sites.append((X, r, noise, theta, H.query_points(i, 130, seed=b + 1)))
    return sites


BATCH = [(H.BIGGEST, torch.float64), (2, torch.float64), (8, torch.float64), (26, torch.float64), (H.BIGGEST, torch.float32), (8, torch.float32)]


@pytest.mark.parametrize("i,dtype", BATCH, ids=[f"{H.CASES[i].name} {str(dt)[6:]}" for i, dt in BATCH])
def test_batch_of_ten_ragged(i, dtype, gpu_device):
    case = H.CASES[i]
    name = H.define(case.spec)
    prior = composite_prior(list(case.spec))
    _batch_of_ten(name, case.d, _composite_sites(i), dtype, gpu_device, H.differentiable_columns(case.spec), prior,
                  f"{case.name} {str(dtype)[6:]}")


@pytest.mark.parametrize("model,d", [("loadest", 3), ("rating", 2)])
def test_batch_of_ten_on_a_fused_model(model, d, gpu_device):
    sites = []
    for b, nb in enumerate(SIZES):
        X, r, noise, theta = make_case(model, d, nb, seed=140 + b, perturb=0.2)
        sites.append((X, torch.nan_to_num(r, nan=0.3), noise, theta, make_case(model, d, 130, seed=190 + b)[0]))
    _batch_of_ten(model, d, sites, torch.float64, gpu_device, list(range(d)), PRIORS[model], f"{model} d={d} float64")


def test_two_structures_in_alternation(gpu_device):
    """Two plans with different trees called A, B, A, B: every result equals the bits of that plan's first call (the
    descriptor the dispatch selects is per call, never the last plan's).  Both plans exist before the first call, so the
    first calls are held against the oracle as well: the same wrong descriptor twice would give the same bits twice."""
    dev, m = gpu_device, 130
    plans, refs = [], []
    for i, n in ((H.BIGGEST, 300), (26, 257)):
        case = H.CASES[i]
        X, r, noise = H.data(i, n)
        p = _plan(H.define(case.spec), n, case.d, X, torch.float64, dev, lookahead=1)
        plans.append((p, case.theta, r.to(dev), noise.to(dev), H.query_points(i, m).to(dev).contiguous()))
        refs.append((orc.nll_data_and_grads(p.model, X, r, noise, case.theta), orc.posterior(p.model, X, r, noise, case.theta, H.query_points(i, m))))
    first = {}
    for rnd in range(2):
        for k, (p, theta, r, noise, Xs) in enumerate(plans):
            res = [t.clone() for t in p.fit_step(theta, r, noise)] + [t.clone() for t in p.predict(theta, Xs)]
            if rnd == 0:
                first[k] = res
            else:
                assert all(torch.equal(a, b) for a, b in zip(res, first[k])), k
    for k, ((p, theta, _r, _noise, _Xs), (fit_ref, (mu_ref, var_ref))) in enumerate(zip(plans, refs)):
        out, dr, dnoise, mu, var = first[k]
        e = _fit_errors(out, dr, dnoise, fit_ref, theta.numel())
        e_m = (mu.cpu() - mu_ref).abs().max().item()
        e_v = ((var.cpu() - var_ref).abs() / (var_ref.abs() + 1e-4)).max().item()
        print(f"sweep alternation fp64 plan {k}: nll {e[0]:.2e} dtheta {e[1]:.2e} dr {e[2]:.2e} dnoise {e[3]:.2e} mean {e_m:.2e} var {e_v:.2e}")
        assert e[0] <= 1e-10 and max(e[1:]) <= 1e-8 and e_m < 1e-9 and e_v < 1e-8, (k, e, e_m, e_v)


def test_distributed_slab_path_three_thread_ranks(gpu_device):
    """A random three-term tree at n = 900 over three thread ranks (two panels per group: four groups, one rank with two)
    against the single plan: NLL 1e-11, gradient 1e-9, as in tests/test_gpu_composite.py for one rank."""
    from discontinuum_amd import _lib
    from discontinuum_amd.dist_chol import DistributedFit, run_thread_ranks

    dev, n = gpu_device, 900
    NLL = _lib.OUT_NLL
    i = next(k for k in H.RANDOM if len(H.CASES[k].terms) == 3)
    case = H.CASES[i]
    name, d, theta, P = H.define(case.spec), case.d, case.theta, case.ntheta
    X, r, noise = H.data(i, n)
    Xd, rd, nd = (t.to(dev).contiguous() for t in (X, r, noise))
    G = slice(_lib.OUT_DTHETA, _lib.OUT_DTHETA + P)

    def rank_body(comm):
        ctx = DistributedFit(name, n, d, device=dev, group_panels=2, comm=comm)
        ctx.set_inputs(Xd)
        return ctx.fit_step(theta, rd, nd).cpu().double()

    res = run_thread_ranks(3, rank_body, device=dev)
    torch.cuda.synchronize()
    p = _plan(name, n, d, X, torch.float64, dev)
    ref = p.fit_step(theta, rd, nd)[0].cpu()
    e_n = max(abs(o[NLL] - ref[NLL]).item() / abs(ref[NLL]).item() for o in res)
    e_g = max(_rel(o[G], ref[G]) for o in res)
    print(f"sweep distributed fp64 {case.name} n={n} over 3 thread ranks: nll {e_n:.2e} dtheta {e_g:.2e} against the single plan")
    assert all(o[_lib.OUT_INFO] == 0 for o in res) and e_n <= 1e-11 and e_g <= 1e-9, (e_n, e_g)
    assert all(torch.equal(o, res[0]) for o in res)
    val, g_theta, _g_r, _g_noise = orc.nll_data_and_grads(name, X, r, noise, theta)
    assert abs(res[0][NLL] - val) <= 1e-10 * abs(val) and _rel(res[0][G], g_theta) <= 1e-8
