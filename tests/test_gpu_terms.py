"""GPU parity of ``dgp_predict_terms`` (the exact posterior of the covariance's additive parts, with the cross-covariances
between them) against the dense CPU construction of tests/terms_helpers.py -- the oracle's own Gram with the other parts'
outputscales zeroed, Cholesky, ``solve_triangular`` -- and against ``dgp_predict`` on the same plan.

Bounds.  fp64 means 1e-9 of max |mean| (floor 1); fp64 variances and covariances 1e-8 of the largest TOTAL prior variance
max_j k(x*_j, x*_j) -- DESIGN section 5's bounds for the posterior mean and variance; absolute, never relative per entry
(per-part variances of the gated rating terms go down to 1e-10 of the prior variance).  The reference's own parts sum to
``orc.posterior`` to <= 1.3e-13 / 6e-15 on these scales (tests/test_terms_cpu.py).  Identities against ``GPPlan.predict`` on
the same plan: sum of the means 1e-12, sum of the C x C covariance 1e-11 of the same scales.  fp32 plans: mean abs 1e-3,
covariances 1e-3 of the prior-variance scale (tests/test_gpu_fp32.py's posterior row).  Every printed figure is a
measurement, the assertions are the bounds.
"""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as orc
from tests.terms_helpers import NAMES, model_reference, outputscale_indices, pack_cov, term_grams, terms_reference, unpack_cov
from tests.test_gpu_stages import make_case, plan_for

pytestmark = pytest.mark.gpu

# every n in {1, 17, 128, 129, 300, 1000, 1300}, every m in {1, 130, 300, 1000} (m > n included), loadest d in {2, 3, 4}, rating
CASES = [
    ("loadest", 2, 1, 130), ("loadest", 2, 129, 1), ("loadest", 2, 1000, 300),
    ("loadest", 3, 17, 300), ("loadest", 3, 300, 1000), ("loadest", 3, 1000, 130), ("loadest", 3, 1300, 300),
    ("loadest", 4, 128, 130), ("loadest", 4, 300, 1),
    ("rating", 2, 1, 1), ("rating", 2, 17, 130), ("rating", 2, 129, 300), ("rating", 2, 128, 1000), ("rating", 2, 300, 1000),
    ("rating", 2, 1000, 300), ("rating", 2, 1300, 1000),
]


def _test_points(model, d, m, seed=8):
    return make_case(model, d, m, seed=seed)[0]


def _case(model, d, n, seed, perturb):
    """``make_case``; its synthetic target is standardised, which a single observation cannot be: that one gets a residual
    of 0.3."""
    X, r, noise, theta = make_case(model, d, n, seed=seed, perturb=perturb)
    if n == 1:
        r = torch.full_like(r, 0.3)
    return X, r, noise, theta


def _errors(mean, cov, ref_mean, ref_cov, scale):
    """(mean error / max(1, max |mean|), packed-covariance error / scale)"""
    e_m = ((mean.cpu().double() - ref_mean).abs().max() / ref_mean.abs().max().clamp(min=1.0)).item()
    e_c = ((cov.cpu().double() - pack_cov(ref_cov)).abs().max() / scale).item()
    return e_m, e_c


def _nan_work_area(p, m):
    """Hand the plan a prediction work area whose every byte is 0xFF (NaN in both dtypes)."""
    need = int(p.lib.dgp_predict_terms_workspace_bytes(p._h, m))
    p._terms_ws = torch.full((need + 256,), 255, dtype=torch.uint8, device=p.device)


@pytest.mark.parametrize("model,d,n,m", CASES)
def test_parity_and_identities_fp64(model, d, n, m, gpu_device):
    dev = gpu_device
    X, r, noise, theta = _case(model, d, n, seed=1, perturb=0.3)
    Xs = _test_points(model, d, m)
    ref_mean, ref_cov, scale = terms_reference(orc.GRAMS[model], outputscale_indices(model, d), X, r, noise, theta, Xs)
    C = len(NAMES[model])
    p = plan_for(model, d, n, X, torch.float64, dev)
    assert p.nterms == C
    Xd = Xs.to(dev).contiguous()
    results = []
    for state in ("factorize", "fit_step"):
        if state == "factorize":
            p.factorize(theta, r.to(dev), noise.to(dev))
        else:
            p.fit_step(theta, r.to(dev), noise.to(dev))
        _nan_work_area(p, m)  # pad columns, ragged rows, m % 128 != 0: nothing of the work area may reach an output
        mean, cov = p.predict_terms(theta, Xd)
        assert mean.shape == (C, m) and cov.shape == (C * (C + 1) // 2, m)
        assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(cov).all())
        e_m, e_c = _errors(mean, cov, ref_mean, ref_cov, scale)
        mu, var = p.predict(theta, Xd)
        full = unpack_cov(cov.cpu())
        i_m = ((mean.sum(0) - mu).abs().max().item()) / max(1.0, ref_mean.abs().max().item())
        i_c = (full.sum((0, 1)) - var.cpu()).abs().max().item() / scale
        print(f"terms fp64 {model} d={d} n={n} m={m} after {state}: mean {e_m:.2e} cov {e_c:.2e} | sum mean {i_m:.2e} sum cov {i_c:.2e}")
        assert e_m < 1e-9 and e_c < 1e-8, (state, e_m, e_c)
        assert i_m < 1e-12 and i_c < 1e-11, (state, i_m, i_c)
        again = p.predict_terms(theta, Xd)
        assert torch.equal(again[0], mean) and torch.equal(again[1], cov)  # bitwise run to run
        only_mean, none = p.predict_terms(theta, Xd, return_cov=False)
        assert none is None and torch.equal(only_mean, mean)
        results.append((mean, cov))
    # the factorisation the fit step leaves is the one factorize leaves
    e_m, e_c = _errors(results[1][0], results[1][1], results[0][0].cpu().double(), unpack_cov(results[0][1].cpu().double()), scale)
    assert e_m < 1e-12 and e_c < 1e-11, (e_m, e_c)
    if m > 128:  # chunks of 128 points give the same numbers as one launch sequence
        mean_c, cov_c = p.predict_terms(theta, Xd, chunk=128)
        e_m, e_c = _errors(mean_c, cov_c, results[1][0].cpu().double(), unpack_cov(results[1][1].cpu().double()), scale)
        assert e_m < 1e-12 and e_c < 1e-11, (e_m, e_c)


@pytest.mark.parametrize("model,d,n,m", [("loadest", 3, 300, 130), ("loadest", 4, 129, 300), ("rating", 2, 300, 130), ("rating", 2, 17, 300)])
def test_in_order_sum_of_terms_against_the_cross_gram(model, d, n, m, gpu_device):
    """The parts, added in index order, against ``dgp_cross_gram`` (``pair<false>``) on the same inputs.  Not bitwise: hipcc
    contracts ``pair``'s products into its adds (-ffp-contract=fast) and ``pair`` gates the SUM of the two rating shifts,
    while a part is a rounded product of its own.  All parts are >= 0, so the sum's error is a few ulp of the total: the
    bound is 4 ulp of ``pair``'s value."""
    dev = gpu_device
    X, r, noise, theta = make_case(model, d, n, seed=1, perturb=0.3)
    Xs = _test_points(model, d, m).to(dev).contiguous()
    p = plan_for(model, d, n, X, torch.float64, dev)
    p.factorize(theta, r.to(dev), noise.to(dev))
    p.predict_terms(theta, Xs)
    C, N, Mp = p.nterms, p.N, int(p.lib.dgp_padded_n(m))
    # the work area begins with the test points' SoA copy (d Mp elements, rounded up to 256 bytes), then the N x (C Mp) cross Grams
    base = (-p._terms_ws.data_ptr()) % 256
    off = base + (8 * Mp * d + 255) // 256 * 256
    planes = p._terms_ws[off:off + 8 * N * C * Mp].view(torch.float64).view(N, C, Mp)
    assert bool((planes[n:] == 0).all()) and bool((planes[:, :, m:] == 0).all())  # pad rows and columns are zeros
    total = torch.zeros(n, m, dtype=torch.float64, device=dev)
    for c in range(C):
        total = total + planes[:n, c, :m]
    pair = p.cross_gram(theta, Xs)
    ulp = torch.from_numpy(np.spacing(pair.cpu().numpy()))
    worst = ((total.cpu() - pair.cpu()).abs() / ulp).max().item()
    print(f"in-order sum of terms vs pair {model} d={d} n={n} m={m}: {worst:.1f} ulp, bitwise equal: {bool(torch.equal(total, pair))}")
    assert worst <= 4.0, worst
    ref = [g(X, Xs.cpu(), theta) for g in term_grams(orc.GRAMS[model], outputscale_indices(model, d))]
    for c in range(C):
        assert (planes[:n, c, :m].cpu() - ref[c]).abs().max().item() < 1e-13, c


@pytest.mark.parametrize("model,d,sizes", [("loadest", 3, (200, 129, 17)), ("rating", 2, (60, 130, 1, 128, 97, 33, 129, 5, 150, 64, 111))])
def test_ragged_batch_against_single_site_plans(model, d, sizes, gpu_device):
    """Every site of a ragged batched plan against a single-site plan of its own size; 11 sites take the hyperparameters
    through the device scratch (more than 8 do not fit the kernel arguments)."""
    from discontinuum_amd.backend import GPPlan

    dev, B, n, m = gpu_device, len(sizes), max(sizes), 150
    cases = [_case(model, d, nb, seed=40 + b, perturb=0.2) for b, nb in enumerate(sizes)]
    Xs = torch.stack([_test_points(model, d, m, seed=90 + b) for b in range(B)]).to(dev).contiguous()
    X = torch.full((B, n, d), float("nan"), dtype=torch.float64)
    r = torch.full((B, n), float("nan"), dtype=torch.float64)
    noise = torch.full((B, n), float("nan"), dtype=torch.float64)
    for b, (nb, c) in enumerate(zip(sizes, cases)):
        X[b, :nb], r[b, :nb], noise[b, :nb] = c[0], c[1], c[2]
    theta = torch.stack([c[3] for c in cases])
    pb = GPPlan(model, n, d, device=dev, lookahead=1, batch=B)
    pb.set_site_sizes(sizes)
    pb.set_inputs(X.to(dev).contiguous())
    pb.factorize(theta, r.to(dev).contiguous(), noise.to(dev).contiguous())
    _nan_work_area(pb, m)
    mean, cov = pb.predict_terms(theta, Xs)
    C = pb.nterms
    assert mean.shape == (B, C, m) and cov.shape == (B, C * (C + 1) // 2, m)
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(cov).all())
    again = pb.predict_terms(theta, Xs)
    assert torch.equal(again[0], mean) and torch.equal(again[1], cov)
    mean_c, cov_c = pb.predict_terms(theta, Xs, chunk=128)  # staged column ranges of a batched result
    worst = (0.0, 0.0)
    for b, (nb, c) in enumerate(zip(sizes, cases)):
        ps = plan_for(model, d, nb, c[0], torch.float64, dev)
        ps.factorize(c[3], c[1].to(dev), c[2].to(dev))
        m1, c1 = ps.predict_terms(c[3], Xs[b].contiguous())
        scale = float(torch.diagonal(orc.GRAMS[model](Xs[b].cpu(), Xs[b].cpu(), c[3])).max())
        e_m, e_c = _errors(mean[b], cov[b], m1.cpu(), unpack_cov(c1.cpu()), scale)
        assert e_m < 1e-11 and e_c < 1e-11, (b, nb, e_m, e_c)
        f_m, f_c = _errors(mean_c[b], cov_c[b], m1.cpu(), unpack_cov(c1.cpu()), scale)
        assert f_m < 1e-11 and f_c < 1e-11, (b, nb, f_m, f_c)
        worst = (max(worst[0], e_m), max(worst[1], e_c))
    print(f"ragged batch {model} B={B}: mean {worst[0]:.2e} cov {worst[1]:.2e} against single-site plans")


def _composite(name):
    from discontinuum_amd.gp import kernels as K
    from discontinuum_amd.gp.lowering import composite_spec, lower

    if name == "three terms d=3":
        d = 3
        cov = (K.ScaleKernel(K.RBFKernel(active_dims=[0]))
               + K.ScaleKernel(K.PeriodicKernel(active_dims=[0]) * K.MaternKernel(nu=2.5, active_dims=[0]))
               + K.ScaleKernel(K.MaternKernel(nu=1.5, active_dims=[0, 1, 2], ard_num_dims=3)))
    else:  # five columns: the widest feature strips
        d = 5
        cov = (K.ScaleKernel(K.RBFKernel(active_dims=[0, 1, 2, 3, 4], ard_num_dims=5))
               + K.ScaleKernel(K.MaternKernel(nu=0.5, active_dims=[0]))
               + K.ScaleKernel(K.PeriodicKernel(active_dims=[0]) * K.RBFKernel(active_dims=[4]))
               + K.ScaleKernel(K.MaternKernel(nu=2.5, active_dims=[1, 3])))
    torch.manual_seed(3)
    for q in cov.parameters():
        with torch.no_grad():
            q.add_(0.4 * torch.randn_like(q))
    model, theta_fn = lower(cov, d)
    assert model.startswith("composite:")
    spec, _ = composite_spec(cov, d)
    return model, d, spec, theta_fn().detach()


@pytest.mark.parametrize("name,nterms", [("three terms d=3", 3), ("four terms d=5", 4)])
def test_composite_model_against_the_oracle(name, nterms, gpu_device):
    from discontinuum_amd.backend import GPPlan

    dev, n, m = gpu_device, 300, 130
    model, d, spec, theta = _composite(name)
    gram = orc.composite_gram(spec)
    rng = np.random.default_rng(0)
    pts = lambda k: torch.tensor(np.concatenate([np.sort(rng.uniform(-4.0, 4.0, k))[:, None], rng.standard_normal((k, d - 1))], axis=1))  # noqa: E731
    X, Xs = pts(n), pts(m)
    r = torch.tensor(rng.standard_normal(n))
    noise = torch.full((n,), 0.05, dtype=torch.float64)
    ref_mean, ref_cov, scale = terms_reference(gram, outputscale_indices(model, d, spec), X, r, noise, theta, Xs)
    p = GPPlan(model, n, d, device=dev)
    assert p.nterms == nterms
    p.set_inputs(X.to(dev).contiguous())
    p.factorize(theta, r.to(dev), noise.to(dev))
    _nan_work_area(p, m)
    mean, cov = p.predict_terms(theta, Xs.to(dev).contiguous())
    e_m, e_c = _errors(mean, cov, ref_mean, ref_cov, scale)
    mu, var = p.predict(theta, Xs.to(dev).contiguous())
    i_m = (mean.sum(0) - mu).abs().max().item() / max(1.0, ref_mean.abs().max().item())
    i_c = (unpack_cov(cov.cpu()).sum((0, 1)) - var.cpu()).abs().max().item() / scale
    print(f"terms fp64 {name}: mean {e_m:.2e} cov {e_c:.2e} | sum mean {i_m:.2e} sum cov {i_c:.2e}")
    assert e_m < 1e-9 and e_c < 1e-8 and i_m < 1e-12 and i_c < 1e-11, (e_m, e_c, i_m, i_c)


@pytest.mark.parametrize("model,d,n", [("loadest", 3, 1000), ("rating", 2, 1300)])
def test_parity_fp32(model, d, n, gpu_device):
    dev, m = gpu_device, 300
    X, r, noise, theta = make_case(model, d, n, seed=7, perturb=0.1)
    Xs = _test_points(model, d, m)
    ref_mean, ref_cov, scale = terms_reference(orc.GRAMS[model], outputscale_indices(model, d), X, r, noise, theta, Xs)
    p = plan_for(model, d, n, X, torch.float32, dev)
    Xd = Xs.to(dev, torch.float32).contiguous()
    for state in ("factorize", "fit_step"):
        if state == "factorize":
            p.factorize(theta, r.to(dev, torch.float32), noise.to(dev, torch.float32))
        else:
            p.fit_step(theta, r.to(dev, torch.float32), noise.to(dev, torch.float32))
        _nan_work_area(p, m)
        mean, cov = p.predict_terms(theta, Xd)
        assert mean.dtype == torch.float32 and cov.dtype == torch.float32
        e_m = (mean.cpu().double() - ref_mean).abs().max().item()
        e_c = (cov.cpu().double() - pack_cov(ref_cov)).abs().max().item() / scale
        mu, var = p.predict(theta, Xd)
        i_m = (mean.sum(0) - mu).abs().max().item()
        i_c = (unpack_cov(cov.cpu()).sum((0, 1)) - var.cpu()).abs().max().item() / scale
        print(f"terms fp32 {model} n={n} after {state}: mean abs {e_m:.2e} cov/scale {e_c:.2e} (scale {scale:.3g}) | sum mean {i_m:.2e} sum cov {i_c:.2e}")
        assert e_m <= 1e-3 and e_c <= 1e-3, (state, e_m, e_c)
        again = p.predict_terms(theta, Xd)
        assert torch.equal(again[0], mean) and torch.equal(again[1], cov)


def test_bad_arguments_on_a_live_plan(gpu_device):
    import ctypes as C

    from discontinuum_amd import _lib
    from discontinuum_amd.backend import GPPlan

    dev, n, d, m = gpu_device, 200, 3, 130
    X, r, noise, theta = make_case("loadest", d, n, seed=1)
    p = GPPlan("loadest", n, d, device=dev)
    lib = p.lib
    need = int(lib.dgp_predict_terms_workspace_bytes(p._h, m))
    work = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    Xs = _test_points("loadest", d, m).to(dev).contiguous()
    mean = torch.full((3, m), 7.0, dtype=torch.float64, device=dev)
    th = (C.c_double * p.ntheta)(*theta.tolist())
    call = lambda mm, wb: lib.dgp_predict_terms(p._h, th, C.c_void_p(Xs.data_ptr()), mm, C.c_void_p(work.data_ptr()), wb,  # noqa: E731
                                                C.c_void_p(mean.data_ptr()), None, None)
    p.set_inputs(X.to(dev).contiguous())
    assert call(m, need) == -4 and b"factorisation" in lib.dgp_last_error()  # DGP_E_STATE: nothing factorised yet
    p.factorize(theta, r.to(dev), noise.to(dev))
    assert call(0, need) == -1 and call(-1, need) == -1
    assert call(m, need - 1) == -3 and b"too small" in lib.dgp_last_error()
    torch.cuda.synchronize(dev)
    assert bool((mean == 7.0).all())  # no launch wrote anything
    with pytest.raises(_lib.DGPError):
        _lib.check(call(m, 0), "dgp_predict_terms")
    with pytest.raises(ValueError):
        p.predict_terms(theta, Xs.cpu())


def _fitted(kind):
    from discontinuum_amd.loadest_gp import LoadestGP
    from discontinuum_amd.rating_gp import RatingGP
    from tests.helpers import loadest_dataset, rating_dataset

    torch.manual_seed(0)
    if kind == "loadest":
        covariates, target = loadest_dataset(n=150, seed=1)
        model = LoadestGP()
        model.fit(covariates, target, iterations=6)
    else:
        covariates, target, unc = rating_dataset(n=120, seed=2)
        model = RatingGP()
        model.fit(covariates, target, target_unc=unc, iterations=6)
    return model, covariates


@pytest.mark.parametrize("kind", ["loadest", "rating"])
def test_engine_decompose_against_the_reference(kind, gpu_device):
    from discontinuum_amd.loads import target_transform

    model, covariates = _fitted(kind)
    names = NAMES[kind]
    C = len(names)
    ds = model.decompose(covariates, return_cov=True)
    assert list(ds.coords["component"].values) == list(names) + ["mean"]
    _mode, s, t = target_transform(model.dm)
    Xnew = torch.tensor(model.dm.Xnew(covariates), dtype=torch.float64)
    ref_mean, ref_cov, scale = model_reference(model, Xnew)
    mean, se, cov = (np.asarray(ds[k].values) for k in ("mean", "se", "cov"))
    e_m = np.abs(mean[:C] / s - ref_mean.numpy()).max() / max(1.0, float(ref_mean.abs().max()))
    e_c = np.abs(cov[:C, :C] / (s * s) - ref_cov.numpy()).max() / scale
    print(f"decompose {kind}: mean {e_m:.2e} cov {e_c:.2e}")
    assert e_m < 1e-8 and e_c < 1e-8, (e_m, e_c)
    assert np.all(se >= 0) and np.all(se[C] == 0)
    target, _se = model.predict(covariates)
    assert np.abs(mean.sum(0) - np.log(np.asarray(target.values).reshape(-1))).max() < 1e-9
    if kind == "rating":
        merged = model.decompose(covariates, groups={"shift": ("shift_1", "shift_2")}, return_cov=True)
        assert list(merged.coords["component"].values) == ["shift", "bend", "base", "periodic", "mean"]
        var = (ref_cov[0, 0] + ref_cov[1, 1] + 2 * ref_cov[0, 1]).numpy()
        e_v = np.abs(merged["se"].values[0] ** 2 / (s * s) - var.clip(0)).max() / scale
        e_s = np.abs(merged["mean"].values[0] / s - (ref_mean[0] + ref_mean[1]).numpy()).max() / max(1.0, float(ref_mean.abs().max()))
        print(f"decompose rating, merged shift: mean {e_s:.2e} var {e_v:.2e}")
        assert e_v < 1e-8 and e_s < 1e-8, (e_s, e_v)
