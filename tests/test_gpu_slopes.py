"""GPU parity of ``dgp_predict_slopes`` (the exact posterior of the fit's input derivatives, with the covariances between the
slopes and with the value) against the dense CPU construction of tests/slopes_helpers.py -- autograd derivative planes of the
oracle's own Gram, closed-form prior block, Cholesky, ``solve_triangular`` -- and against ``dgp_predict`` on the same plan.

Bounds (those of ``dgp_predict_terms``, per plane): fp64 means 1e-9 of max |mean_plane| (floor 1); fp64 covariances 1e-8 of
the plane-pair scale sqrt(max_j prior_aa max_j prior_bb); plane 0 against ``GPPlan.predict`` 1e-12 / 1e-11 of the same scales;
fp32 plans 1e-3 of the same scales; a ragged batch against single-site plans 1e-11.  Every printed figure is a measurement,
the assertions are the bounds.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import gp_oracle as orc
from tests.slopes_helpers import PRIORS, composite_prior, cross_planes, errors, model_reference, shifted, slopes_reference
from tests.terms_helpers import unpack_cov
from tests.test_gpu_stages import make_case, plan_for

pytestmark = pytest.mark.gpu

# n and m off the multiples of 128, m > n, a single observation / point
CASES = [
    ("loadest", 2, 129, 300), ("loadest", 2, 1000, 130), ("loadest", 2, 1, 130),
    ("loadest", 3, 300, 1000), ("loadest", 3, 1000, 130), ("loadest", 3, 1300, 300), ("loadest", 3, 17, 1),
    ("rating", 2, 129, 300), ("rating", 2, 300, 1000), ("rating", 2, 1000, 130), ("rating", 2, 1300, 300), ("rating", 2, 1, 1),
]

# generic composites as dgp_composite_define takes them ([d, nterms, per term: scaled, nfac, per factor: type, 2 nu, ard,
# ndims, columns...]) with their hyperparameters and the columns asked for
COMPOSITES = {
    # scaled rbf(0) + scaled periodic(0) x matern52(0) + scaled matern32 ARD(0, 1, 2)
    "periodic d=3": ([3, 3, 1, 1, 0, 0, 0, 1, 0, 1, 2, 2, 0, 0, 1, 0, 1, 5, 0, 1, 0, 1, 1, 1, 3, 1, 3, 0, 1, 2],
                     [0.7, 2.1, 0.9, 0.8, 1.0, 1.4, 0.6, 1.2, 0.9, 1.6], [0, 1, 2]),
    # scaled periodic(0) x matern52(0) + UNSCALED matern32 ARD(0, 1) x rbf(1)
    "unscaled d=2": ([2, 2, 1, 2, 2, 0, 0, 1, 0, 1, 5, 0, 1, 0, 0, 2, 1, 3, 1, 2, 0, 1, 0, 0, 0, 1, 1],
                     [0.8, 1.3, 0.9, 0.7, 1.1, 0.6, 1.7], [1, 0]),
    # rbf ARD(0 .. 4) + matern12(0) + periodic(0) x rbf(4) + matern52(1, 3): column 0 is not differentiable, the rest is
    "matern12 d=5": ([5, 4, 1, 1, 0, 0, 1, 5, 0, 1, 2, 3, 4, 1, 1, 1, 1, 0, 1, 0, 1, 2, 2, 0, 0, 1, 0, 0, 0, 0, 1, 4,
                      1, 1, 1, 5, 0, 2, 1, 3],
                     [0.6, 1.5, 1.1, 0.9, 1.3, 0.8, 0.3, 1.2, 0.5, 1.4, 1.0, 0.7, 0.9, 1.1], [3, 1, 4, 2]),
}


def _test_points(model, d, m, seed=8):
    return make_case(model, d, m, seed=seed)[0]


def _case(model, d, n, seed, perturb):
    X, r, noise, theta = make_case(model, d, n, seed=seed, perturb=perturb)
    if n == 1:  # a single observation cannot be standardised
        r = torch.full_like(r, 0.3)
    return X, r, noise, theta


def _nan_work_area(p, m, ncols):
    """Hand the plan a work area whose every byte is 0xFF (NaN in both dtypes)."""
    need = int(p.lib.dgp_predict_slopes_workspace_bytes(p._h, m, ncols))
    p._slopes_ws = torch.full((need + 256,), 255, dtype=torch.uint8, device=p.device)


def _planes(p, d, m, ncols):
    """The N x (P Mp) cross planes the last ``predict_slopes`` left in the work area (after the test points' SoA copy)."""
    N, Mp, P = p.N, int(p.lib.dgp_padded_n(m)), 1 + ncols
    base = (-p._slopes_ws.data_ptr()) % 256
    off = base + (8 * Mp * d + 255) // 256 * 256
    return p._slopes_ws[off:off + 8 * N * P * Mp].view(torch.float64).view(N, P, Mp)


def _check_fp64(p, tag, theta, r, noise, Xd, ref, cols, dev):
    """Parity after factorize and after fit_step, plane 0 against dgp_predict, repeatability, read-only state, chunks."""
    ref_mean, ref_cov, scales = ref
    P, m = 1 + len(cols), Xd.shape[0]
    results = []
    for state in ("factorize", "fit_step"):
        if state == "factorize":
            p.factorize(theta, r.to(dev), noise.to(dev))
        else:
            p.fit_step(theta, r.to(dev), noise.to(dev))
        mu0, var0 = p.predict(theta, Xd)
        _nan_work_area(p, m, len(cols))  # pad columns, ragged rows, m % 128 != 0: nothing of the work area may reach an output
        mean, cov = p.predict_slopes(theta, Xd, cols)
        assert mean.shape == (P, m) and cov.shape == (P * (P + 1) // 2, m)
        assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(cov).all())
        e_m, e_c = errors(mean, cov, ref_mean, ref_cov, scales)
        mu, var = p.predict(theta, Xd)
        assert torch.equal(mu, mu0) and torch.equal(var, var0)  # the plan is only read
        i_m = (mean[0] - mu).abs().max().item() / max(1.0, ref_mean[0].abs().max().item())
        i_c = (cov[0] - var).abs().max().item() / float(scales[0] ** 2)
        print(f"slopes fp64 {tag} after {state}: mean {e_m:.2e} cov {e_c:.2e} | plane 0 vs predict: mean {i_m:.2e} var {i_c:.2e}")
        assert e_m < 1e-9 and e_c < 1e-8, (state, e_m, e_c)
        assert i_m < 1e-12 and i_c < 1e-11, (state, i_m, i_c)
        again = p.predict_slopes(theta, Xd, cols)
        assert torch.equal(again[0], mean) and torch.equal(again[1], cov)  # bitwise run to run
        only_mean, none = p.predict_slopes(theta, Xd, cols, return_cov=False)
        assert none is None and torch.equal(only_mean, mean)
        results.append((mean, cov))
    full = unpack_cov(results[1][1].cpu().double())
    e_m, e_c = errors(results[0][0], results[0][1], results[1][0].cpu().double(), full, scales)
    assert e_m < 1e-12 and e_c < 1e-11, (e_m, e_c)  # the factorisation the fit step leaves is the one factorize leaves
    # nearby ncols: one column at a time gives the shared planes of the all-columns call
    for q, c in enumerate(cols):
        m1, c1 = p.predict_slopes(theta, Xd, [c])
        sel = [0, q + 1]
        e_m, e_c = errors(m1, c1, results[1][0].cpu().double()[sel], full[sel][:, sel], scales[sel])
        assert e_m < 1e-9 and e_c < 1e-8, (c, e_m, e_c)
    if m > 128:  # chunks of 128 points give the same numbers as one launch sequence
        mean_c, cov_c = p.predict_slopes(theta, Xd, cols, chunk=128)
        e_m, e_c = errors(mean_c, cov_c, results[1][0].cpu().double(), full, scales)
        assert e_m < 1e-12 and e_c < 1e-11, (e_m, e_c)


@pytest.mark.parametrize("model,d,n,m", CASES)
def test_parity_and_identities_fp64(model, d, n, m, gpu_device):
    dev = gpu_device
    X, r, noise, theta = _case(model, d, n, seed=1, perturb=0.3)
    Xs = _test_points(model, d, m)
    cols = list(range(d))
    ref = slopes_reference(orc.GRAMS[model], PRIORS[model], X, r, noise, theta, Xs, cols)
    p = plan_for(model, d, n, X, torch.float64, dev)
    _check_fp64(p, f"{model} d={d} n={n} m={m}", theta, r, noise, Xs.to(dev).contiguous(), ref, cols, dev)


@pytest.mark.parametrize("name", list(COMPOSITES))
def test_composite_models_against_the_oracle(name, gpu_device):
    from discontinuum_amd import _lib
    from discontinuum_amd.backend import GPPlan

    dev, n, m = gpu_device, 300, 130
    spec, theta, cols = COMPOSITES[name]
    d = spec[0]
    lib = _lib.load()
    arr, mid = (C.c_int * len(spec))(*spec), C.c_int()
    assert lib.dgp_composite_define(arr, len(spec), C.byref(mid)) == 0
    theta = torch.tensor(theta, dtype=torch.float64)
    rng = np.random.default_rng(0)
    pts = lambda k: torch.tensor(np.concatenate([np.sort(rng.uniform(-4.0, 4.0, k))[:, None], rng.standard_normal((k, d - 1))], axis=1))  # noqa: E731
    X, Xs = pts(n), pts(m)
    r = torch.tensor(rng.standard_normal(n))
    noise = torch.full((n,), 0.05, dtype=torch.float64)
    ref = slopes_reference(orc.composite_gram(spec), composite_prior(spec), X, r, noise, theta, Xs, cols)
    p = GPPlan(f"composite:{mid.value}", n, d, device=dev)
    assert p.ntheta == len(theta)
    p.set_inputs(X.to(dev).contiguous())
    _check_fp64(p, name, theta, r, noise, Xs.to(dev).contiguous(), ref, cols, dev)
    if name == "matern12 d=5":
        with pytest.raises(ValueError, match="not differentiable"):
            p.predict_slopes(theta, Xs.to(dev).contiguous(), [0])


@pytest.mark.parametrize("model,d,n", [("loadest", 3, 1000), ("rating", 2, 1300)])
def test_parity_fp32(model, d, n, gpu_device):
    dev, m = gpu_device, 300
    X, r, noise, theta = make_case(model, d, n, seed=7, perturb=0.1)
    Xs = _test_points(model, d, m)
    cols = list(range(d))
    ref_mean, ref_cov, scales = slopes_reference(orc.GRAMS[model], PRIORS[model], X, r, noise, theta, Xs, cols)
    p = plan_for(model, d, n, X, torch.float32, dev)
    Xd = Xs.to(dev, torch.float32).contiguous()
    for state in ("factorize", "fit_step"):
        if state == "factorize":
            p.factorize(theta, r.to(dev, torch.float32), noise.to(dev, torch.float32))
        else:
            p.fit_step(theta, r.to(dev, torch.float32), noise.to(dev, torch.float32))
        _nan_work_area(p, m, d)
        mean, cov = p.predict_slopes(theta, Xd, cols)
        assert mean.dtype == torch.float32 and cov.dtype == torch.float32
        e_m, e_c = errors(mean, cov, ref_mean, ref_cov, scales)
        print(f"slopes fp32 {model} n={n} after {state}: mean {e_m:.2e} cov {e_c:.2e} (plane scales {[f'{float(v):.3g}' for v in scales]})")
        assert e_m <= 1e-3 and e_c <= 1e-3, (state, e_m, e_c)
        again = p.predict_slopes(theta, Xd, cols)
        assert torch.equal(again[0], mean) and torch.equal(again[1], cov)


@pytest.mark.parametrize("model,d", [("loadest", 3), ("rating", 2), ("composite", 3)])
def test_coincident_points(model, d, gpu_device):
    """Test points equal to training points and a repeated test point: finite results within the parity bounds, and the
    derivative planes' entries at the coincident pairs EXACTLY 0 for the stationary models (for rating: the time plane; its
    stage plane carries the gate's derivative) -- the evaluators never divide by the distance."""
    from discontinuum_amd import _lib
    from discontinuum_amd.backend import GPPlan

    dev, n, m, k = gpu_device, 300, 130, 40
    if model == "composite":
        spec, theta, _cols = COMPOSITES["periodic d=3"]
        arr, mid = (C.c_int * len(spec))(*spec), C.c_int()
        assert _lib.load().dgp_composite_define(arr, len(spec), C.byref(mid)) == 0
        theta = torch.tensor(theta, dtype=torch.float64)
        rng = np.random.default_rng(5)
        X = torch.tensor(np.concatenate([np.sort(rng.uniform(-4.0, 4.0, n))[:, None], rng.standard_normal((n, 2))], axis=1))
        Xs = torch.tensor(np.concatenate([rng.uniform(-4.0, 4.0, m)[:, None], rng.standard_normal((m, 2))], axis=1))
        r, noise = torch.tensor(rng.standard_normal(n)), torch.full((n,), 0.05, dtype=torch.float64)
        gram, prior_fn, name = orc.composite_gram(spec), composite_prior(spec), f"composite:{mid.value}"
    else:
        X, r, noise, theta = make_case(model, d, n, seed=1, perturb=0.3)
        Xs = _test_points(model, d, m)
        gram, prior_fn, name = orc.GRAMS[model], PRIORS[model], model
    Xs[:k] = X[100:100 + k]
    Xs[k + 1] = Xs[k]
    Xs[k + 2] = Xs[k]
    cols = list(range(d))
    ref_mean, ref_cov, scales = slopes_reference(gram, prior_fn, X, r, noise, theta, Xs, cols)
    p = GPPlan(name, n, d, device=dev)
    p.set_inputs(X.to(dev).contiguous())
    p.factorize(theta, r.to(dev), noise.to(dev))
    _nan_work_area(p, m, d)
    mean, cov = p.predict_slopes(theta, Xs.to(dev).contiguous(), cols)
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(cov).all())
    e_m, e_c = errors(mean, cov, ref_mean, ref_cov, scales)
    print(f"coincident points {model}: mean {e_m:.2e} cov {e_c:.2e}")
    assert e_m < 1e-9 and e_c < 1e-8, (e_m, e_c)
    assert torch.equal(mean[:, k], mean[:, k + 1]) and torch.equal(cov[:, k], cov[:, k + 2])
    planes = _planes(p, d, m, d)
    assert bool((planes[n:] == 0).all()) and bool((planes[:, :, m:] == 0).all())  # pad rows and columns are zeros
    assert bool(torch.isfinite(planes).all())
    at_pairs = planes[100:100 + k, :, :k].diagonal(dim1=0, dim2=2)  # (P, k)
    assert bool((at_pairs[0] > 0).all())
    for q in range(d):
        if model != "rating" or q == 0:
            assert bool((at_pairs[1 + q] == 0).all()), (q, at_pairs[1 + q].abs().max().item())
    ref_planes = torch.stack(cross_planes(gram, X, Xs, theta, cols), dim=1)
    worst = (planes[:n, :, :m].cpu() - ref_planes).abs().amax(dim=(0, 2)) / ref_planes.abs().amax(dim=(0, 2))
    print(f"coincident points {model}: planes against autograd {[f'{float(v):.1e}' for v in worst]}")
    assert bool((worst < 1e-12).all()), worst


@pytest.mark.parametrize("model,d,sizes", [("loadest", 3, (200, 129, 17)), ("rating", 2, (60, 130, 1, 128, 97, 33, 129, 5, 150, 64, 111))])
def test_ragged_batch_against_single_site_plans(model, d, sizes, gpu_device):
    """Every site of a ragged batched plan against a single-site plan of its own size; 11 sites take the hyperparameters
    through the device scratch (more than 8 do not fit the kernel arguments)."""
    from discontinuum_amd.backend import GPPlan

    dev, B, n, m = gpu_device, len(sizes), max(sizes), 150
    cols = list(range(d))[::-1]
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
    _nan_work_area(pb, m, d)
    mean, cov = pb.predict_slopes(theta, Xs, cols)
    P = 1 + d
    assert mean.shape == (B, P, m) and cov.shape == (B, P * (P + 1) // 2, m)
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(cov).all())
    again = pb.predict_slopes(theta, Xs, cols)
    assert torch.equal(again[0], mean) and torch.equal(again[1], cov)
    mean_c, cov_c = pb.predict_slopes(theta, Xs, cols, chunk=128)  # staged column ranges of a batched result
    worst = (0.0, 0.0)
    for b, (nb, c) in enumerate(zip(sizes, cases)):
        ps = plan_for(model, d, nb, c[0], torch.float64, dev)
        ps.factorize(c[3], c[1].to(dev), c[2].to(dev))
        m1, c1 = ps.predict_slopes(c[3], Xs[b].contiguous(), cols)
        sel = [0] + [1 + q for q in cols]
        prior = PRIORS[model](c[3], Xs[b].cpu())[sel][:, sel]
        scales = torch.sqrt(torch.stack([prior[a, a].max() for a in range(P)]))
        e_m, e_c = errors(mean[b], cov[b], m1.cpu().double(), unpack_cov(c1.cpu().double()), scales)
        assert e_m < 1e-11 and e_c < 1e-11, (b, nb, e_m, e_c)
        f_m, f_c = errors(mean_c[b], cov_c[b], m1.cpu().double(), unpack_cov(c1.cpu().double()), scales)
        assert f_m < 1e-11 and f_c < 1e-11, (b, nb, f_m, f_c)
        worst = (max(worst[0], e_m), max(worst[1], e_c))
    print(f"ragged batch {model} B={B}: mean {worst[0]:.2e} cov {worst[1]:.2e} against single-site plans")


def test_bad_arguments_on_a_live_plan(gpu_device):
    from discontinuum_amd import _lib
    from discontinuum_amd.backend import GPPlan

    dev, n, d, m = gpu_device, 200, 3, 130
    X, r, noise, theta = make_case("loadest", d, n, seed=1)
    p = GPPlan("loadest", n, d, device=dev)
    lib = p.lib
    need = int(lib.dgp_predict_slopes_workspace_bytes(p._h, m, d))
    work = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    Xs = _test_points("loadest", d, m).to(dev).contiguous()
    mean = torch.full((1 + d, m), 7.0, dtype=torch.float64, device=dev)
    cov = torch.full(((1 + d) * (2 + d) // 2, m), 7.0, dtype=torch.float64, device=dev)
    th = (C.c_double * p.ntheta)(*theta.tolist())
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ints = lambda *v: (C.c_int * len(v))(*v)  # noqa: E731

    def call(mm=m, cols=(0, 1, 2), wb=need, theta_=th, xs=vp(Xs), wk=vp(work), mn=vp(mean), ncols=None, carr=True):
        arr = ints(*cols) if carr else None
        return lib.dgp_predict_slopes(p._h, theta_, xs, mm, arr, len(cols) if ncols is None else ncols, wk, wb, mn, vp(cov), None)

    p.set_inputs(X.to(dev).contiguous())
    assert call() == -4 and b"factorisation" in lib.dgp_last_error()  # DGP_E_STATE: nothing factorised yet
    p.factorize(theta, r.to(dev), noise.to(dev))
    assert call(mm=0) == -1 and call(mm=-1) == -1
    assert call(theta_=None) == -1 and call(xs=None) == -1 and call(wk=None) == -1 and call(mn=None) == -1 and call(carr=False) == -1
    assert lib.dgp_predict_slopes(None, th, vp(Xs), m, ints(0), 1, vp(work), need, vp(mean), None, None) == -1
    assert call(cols=(), ncols=0, carr=False) == -1 and call(cols=(0,), ncols=0) == -1 and b"ncols" in lib.dgp_last_error()
    assert call(cols=(0, 1, 2, 0), ncols=d + 1) == -1
    assert call(cols=(1, 1)) == -1 and b"repeated" in lib.dgp_last_error()
    assert call(cols=(0, 3)) == -1 and call(cols=(-1,)) == -1
    assert call(wb=need - 1) == -3 and b"too small" in lib.dgp_last_error()
    spec = COMPOSITES["matern12 d=5"][0]
    arr, mid = (C.c_int * len(spec))(*spec), C.c_int()
    assert lib.dgp_composite_define(arr, len(spec), C.byref(mid)) == 0
    pc = GPPlan(f"composite:{mid.value}", n, 5, device=dev)
    rng = np.random.default_rng(0)
    pc.set_inputs(torch.tensor(rng.standard_normal((n, 5))).to(dev).contiguous())
    pc.factorize(torch.tensor(COMPOSITES["matern12 d=5"][1]), r.to(dev), noise.to(dev))
    thc = (C.c_double * pc.ntheta)(*COMPOSITES["matern12 d=5"][1])
    xs5 = torch.tensor(rng.standard_normal((m, 5))).to(dev).contiguous()
    big = torch.empty(int(lib.dgp_predict_slopes_workspace_bytes(pc._h, m, 2)) + 256, dtype=torch.uint8, device=dev)
    rc = lib.dgp_predict_slopes(pc._h, thc, vp(xs5), m, ints(1, 0), 2, vp(big), big.numel() - 256, vp(mean), vp(cov), None)
    assert rc == -2 and b"differentiable" in lib.dgp_last_error()  # DGP_E_MODEL: the Matern-1/2 column
    torch.cuda.synchronize(dev)
    assert bool((mean == 7.0).all()) and bool((cov == 7.0).all())  # no launch wrote anything
    with pytest.raises(_lib.DGPError):
        _lib.check(call(wb=0), "dgp_predict_slopes")
    with pytest.raises(ValueError):
        p.predict_slopes(theta, Xs.cpu(), [0])
    for bad in ([], [0, 0], [3], [0, 1, 2, 1]):
        with pytest.raises(ValueError):
            p.predict_slopes(theta, Xs, bad)


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


FD_STEP = 1e-4  # in the slope's unit u: ln flow, years, stage


@pytest.mark.parametrize("kind", ["loadest", "rating"])
def test_engine_slopes_against_the_reference_and_differences_of_predict(kind, gpu_device):
    """``slope`` (and ``rating_exponent``) after a short fit against the dense reference in model space, 1e-8 of the plane
    scales; and against central differences of ``model.predict`` in covariate space at step FD_STEP.  The differences carry a
    truncation error of their own, measured on the CPU reference alone (its analytic slope against the same differences of
    its own posterior mean); the bound is twice that plus the 1e-8 parity bound.  Measured finite-difference error of the CPU
    reference alone at FD_STEP = 1e-4, relative to max(1, max |slope|), at the hyperparameters the same six iterations reach
    on the same data: loadest time 1.24e-6, ln flow 4.15e-7; rating time 2.38e-7, stage 1.58e-8 (the test points are the
    training points, where the Matern-3/2 parts have a kink in their second derivative: the differences are first order in
    the step there).  The test measures it again on every run and prints it next to the figure it bounds."""
    from discontinuum_amd.loads import target_transform
    from discontinuum_amd.slopes import covariate_chain, prior_mean_slopes

    model, covariates = _fitted(kind)
    names = list(model.dm.covariate_pipelines)
    cols = list(range(len(names)))
    ds = model.slope(covariates, return_cov=True)
    _mode, s, _t = target_transform(model.dm)
    a = np.asarray([covariate_chain(nm, model.dm.covariate_pipelines[nm])[0] for nm in names])
    Xnew = torch.tensor(model.dm.Xnew(covariates), dtype=torch.float64)
    ref_mean, ref_cov, scales = model_reference(model, Xnew, cols)
    dprior = prior_mean_slopes(model, Xnew.to(model.device), cols)
    mean, cov, cov_value = (np.asarray(ds[k].values) for k in ("mean", "cov", "cov_value"))
    latent = mean / (s * a[:, None]) - dprior
    e_m = max(np.abs(latent[q] - ref_mean[1 + q].numpy()).max() / max(1.0, float(ref_mean[1 + q].abs().max())) for q in cols)
    sc = scales.numpy()
    e_c = max(np.abs(cov[q, e] / (s * s * a[q] * a[e]) - ref_cov[1 + q, 1 + e].numpy()).max() / (sc[1 + q] * sc[1 + e])
              for q in cols for e in cols)
    e_v = max(np.abs(cov_value[q] / (s * s * a[q]) - ref_cov[1 + q, 0].numpy()).max() / (sc[1 + q] * sc[0]) for q in cols)
    print(f"engine slope {kind}: mean {e_m:.2e} cov {e_c:.2e} cov with the value {e_v:.2e}")
    assert e_m < 1e-8 and e_c < 1e-8 and e_v < 1e-8, (e_m, e_c, e_v)
    se = np.asarray(ds["se"].values)
    assert np.all(se > 0) and np.allclose(se ** 2, np.einsum("aam->am", cov), rtol=1e-10)

    def reference_value(cv):
        """s (posterior mean + prior mean) at the covariates ``cv`` from the CPU reference"""
        x = torch.tensor(model.dm.Xnew(cv), dtype=torch.float64)
        mu = model_reference(model, x, [0])[0][0]
        with torch.no_grad():
            pm = model.model.prior_mean(x.to(model.device)).detach().cpu().double().reshape(-1)
        return s * (mu + pm).numpy()

    for q, name in enumerate(names):
        (hi, du_hi), (lo, du_lo) = shifted(covariates, name, FD_STEP), shifted(covariates, name, -FD_STEP)
        du = du_hi - du_lo
        analytic_ref = s * a[q] * (ref_mean[1 + q].numpy() + dprior[q])
        norm_ = max(1.0, np.abs(analytic_ref).max())
        fd_ref = (reference_value(hi) - reference_value(lo)) / du
        fd_err = np.abs(fd_ref - analytic_ref).max() / norm_
        f_hi = np.log(np.asarray(model.predict(hi)[0].values, dtype=np.float64).reshape(-1))
        f_lo = np.log(np.asarray(model.predict(lo)[0].values, dtype=np.float64).reshape(-1))
        err = np.abs(mean[q] - (f_hi - f_lo) / du).max() / norm_
        print(f"engine slope {kind} wrt {name}: finite-difference error of the CPU reference alone {fd_err:.2e}; "
              f"slope against differences of predict {err:.2e} (bound {2 * fd_err + 1e-8:.2e})")
        assert err <= 2 * fd_err + 1e-8, (name, err, fd_err)
    if kind == "rating":
        ex = model.rating_exponent(covariates)
        h = np.asarray(covariates["stage"].values)
        want = h * s * a[1] * (ref_mean[2].numpy() + dprior[1])
        e_x = np.abs(ex["mean"].values - want).max() / max(1.0, np.abs(want).max())
        want_se = h * s * a[1] * np.sqrt(ref_cov[2, 2].numpy().clip(0))
        e_s = np.abs(ex["se"].values - want_se).max() / (h.max() * s * a[1] * sc[2])
        print(f"rating exponent: mean {e_x:.2e} se {e_s:.2e}; median {np.median(ex['mean'].values):.3f}, "
              f"smallest P(increasing) {ex['prob_positive'].values.min():.4f}")
        assert e_x < 1e-8 and e_s < 1e-8, (e_x, e_s)
        assert np.all((ex["prob_positive"].values >= 0) & (ex["prob_positive"].values <= 1))
