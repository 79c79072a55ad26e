"""The gradient contraction streamed along tile rows (csrc/dgp_gram.hip::gram_grad_kernel): a workgroup walks a run of up to
eight consecutive 64 x 64 tiles of one tile row, with a path of its own for tiles strictly below the diagonal whose rows are
all real.

n = 63, 65, 129, 200: one tile, the first sizes with two and three tile rows, a ragged last tile; n = 577 and 700: tile rows
longer than one run (10 and 12 tiles; at n = 700 the last tile row is all padding) with ragged last tiles, so that a run of eight is followed by a short one that holds the
diagonal.  loadest d = 2 and 3 and rating; MODE 0 (the marginal likelihood's gradient) through `fit_step`, MODE 1 (the mean's
vector-Jacobian product) through `mean_vjp`; against the oracle's gradients at 1e-8 of their largest entry (the bound of
tests/test_gpu_stages.py); a repeated call is bitwise the first; a ragged batch, every site against its single-site plan at
bench.PARITY_TOL["f64"]."""
import functools

import pytest
import torch

from oracle import gp_oracle as orc
from tests.test_gpu_stages import make_case, plan_for

pytestmark = pytest.mark.gpu

SIZES = [63, 65, 129, 200, 577, 700]
MODELS = [("loadest", 2), ("loadest", 3), ("rating", 2)]
M_TEST = 70
RAGGED = (577, 200, 65, 513)
PARITY_F64 = {"nll_rel": 1e-11, "grad_rel": 1e-9, "alpha_rel": 1e-9, "dnoise_rel": 1e-9}  # bench.PARITY_TOL["f64"]


def test_parity_bounds_are_the_benchmarks():
    import bench

    assert bench.PARITY_TOL["f64"] == PARITY_F64


@functools.lru_cache(maxsize=None)
def _reference(model, d, n):
    """-> inputs and the oracle's gradients of the NLL and of w^T mean(X*); shared, never modified."""
    X, r, noise, theta = make_case(model, d, n, seed=31, perturb=0.2)
    Xs = make_case(model, d, M_TEST, seed=32)[0]
    w = torch.randn(M_TEST, dtype=torch.float64, generator=torch.Generator().manual_seed(n))
    val, g_theta, _g_r, _g_noise = orc.nll_data_and_grads(model, X, r, noise, theta)
    th = theta.clone().requires_grad_(True)
    mu, _ = orc.posterior(model, X, r, noise, th, Xs)
    (v_theta,) = torch.autograd.grad((mu * w).sum(), (th,))
    return X, r, noise, theta, Xs, w, float(val), g_theta, v_theta


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("model,d", MODELS)
def test_gradients_against_the_oracle(model, d, n, gpu_device):
    from discontinuum_amd import _lib

    dev = gpu_device
    X, r, noise, theta, Xs, w, val, g_theta, v_theta = _reference(model, d, n)
    p = plan_for(model, d, n, X, torch.float64, dev)
    P = theta.numel()
    out = p.fit_step(theta, r.to(dev), noise.to(dev))[0].cpu()
    g = out[_lib.OUT_DTHETA:_lib.OUT_DTHETA + P]
    e_nll = abs(float(out[_lib.OUT_NLL]) - val) / abs(val)
    e_grad = float((g - g_theta).abs().max() / g_theta.abs().max())
    dtheta = p.mean_vjp(theta, Xs.to(dev).contiguous(), w.to(dev))[0].cpu()
    e_vjp = float((dtheta - v_theta).abs().max() / v_theta.abs().max())
    print(f"streamed gradient {model} d={d} n={n}: NLL {e_nll:.2e}, dtheta {e_grad:.2e}, mean_vjp dtheta {e_vjp:.2e}")
    assert int(out[_lib.OUT_INFO]) == 0 and e_nll < 1e-10
    assert e_grad < 1e-8 and e_vjp < 1e-8, (e_grad, e_vjp)
    # a second call on the same inputs: the same bits (every summation order is fixed by the shapes)
    out2 = p.fit_step(theta, r.to(dev), noise.to(dev))[0].cpu()
    dtheta2 = p.mean_vjp(theta, Xs.to(dev).contiguous(), w.to(dev))[0].cpu()
    assert torch.equal(out, out2) and torch.equal(dtheta, dtheta2)
    assert torch.equal(p.stage_grad(theta).cpu(), g)


@functools.lru_cache(maxsize=None)
def _ragged_batch(dev, model, d):
    from discontinuum_amd.backend import GPPlan

    B, n = len(RAGGED), max(RAGGED)
    refs = [_reference(model, d, nb) for nb in RAGGED]
    X = torch.full((B, n, d), float("nan"), dtype=torch.float64)
    r = torch.full((B, n), float("nan"), dtype=torch.float64)
    noise = torch.ones((B, n), dtype=torch.float64)
    for b, (nb, ref) in enumerate(zip(RAGGED, refs)):
        X[b, :nb], r[b, :nb], noise[b, :nb] = ref[0], ref[1], ref[2]
    theta = torch.stack([ref[3] for ref in refs])
    Xs = torch.stack([ref[4] for ref in refs]).to(dev).contiguous()
    w = torch.stack([ref[5] for ref in refs]).to(dev).contiguous()
    p = GPPlan(model, n, d, dtype=torch.float64, device=dev, lookahead=1, batch=B)
    p.set_site_sizes(list(RAGGED))
    p.set_inputs(X.to(dev).contiguous())
    args = (theta, r.to(dev).contiguous(), noise.to(dev).contiguous())
    out, dr, dnoise = (t.cpu().clone() for t in p.fit_step(*args))
    dtheta = p.mean_vjp(theta, Xs, w)[0].cpu().clone()
    out2 = p.fit_step(*args)[0].cpu()
    dtheta2 = p.mean_vjp(theta, Xs, w)[0].cpu()
    assert torch.equal(out, out2) and torch.equal(dtheta, dtheta2)
    return refs, out, dr, dnoise, dtheta


@pytest.mark.parametrize("b", range(len(RAGGED)))
@pytest.mark.parametrize("model,d", [("loadest", 3), ("rating", 2)])
def test_ragged_batch_site_against_the_oracle_and_the_single_site_plan(model, d, b, gpu_device):
    from discontinuum_amd import _lib

    dev = gpu_device
    refs, out, dr, dnoise, dtheta = _ragged_batch(dev, model, d)
    nb = RAGGED[b]
    X, r, noise, theta, Xs, w, val, g_theta, v_theta = refs[b]
    P = theta.numel()
    g = slice(_lib.OUT_DTHETA, _lib.OUT_DTHETA + P)
    e_grad = float((out[b, g] - g_theta).abs().max() / g_theta.abs().max())
    e_vjp = float((dtheta[b, :P] - v_theta).abs().max() / v_theta.abs().max())
    p1 = plan_for(model, d, nb, X, torch.float64, dev)
    o1, a1, n1 = (t.cpu() for t in p1.fit_step(theta, r.to(dev), noise.to(dev)))
    d1 = p1.mean_vjp(theta, Xs.to(dev).contiguous(), w.to(dev))[0].cpu()
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max())  # noqa: E731
    res = {"nll_rel": abs(float(out[b, _lib.OUT_NLL] - o1[_lib.OUT_NLL])) / abs(float(o1[_lib.OUT_NLL])), "grad_rel": rel(out[b, g], o1[g]),
           "alpha_rel": rel(dr[b, :nb], a1), "dnoise_rel": rel(dnoise[b, :nb], n1)}
    e_vjp1 = rel(dtheta[b, :P], d1)
    print(f"streamed gradient, ragged site {b} ({model} n={nb}): oracle dtheta {e_grad:.2e}, mean_vjp {e_vjp:.2e}; single-site plan {res}, "
          f"mean_vjp {e_vjp1:.2e}")
    assert int(out[b, _lib.OUT_INFO]) == 0 and e_grad < 1e-8 and e_vjp < 1e-8, (e_grad, e_vjp)
    assert all(res[k] <= PARITY_F64[k] for k in PARITY_F64) and e_vjp1 <= PARITY_F64["grad_rel"], (res, e_vjp1)
