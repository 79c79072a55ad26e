"""The fit step's two triangular solves from ONE read of T = L^-1 (csrc/dgp_chol.hip: trsv_rows_kernel, trsv_reduce_kernel):
z = T r, alpha = T^T z and quad = z^T z through every entry point that launches them.

* `GPPlan.factorize` (solve) at N = 128, 256, 384, 1152 and 2176 -- one block column, the first sizes with two and three, more
  rows than the 128 row groups hold pairs of, 17 block columns -- with n = N, N - 1, N - 63 and N - 127
  (padding: r counts as zero beyond n), and a ragged batch of five sites: alpha and quad against the oracle at the bounds
  tests/test_gpu_stages.py states for alpha (1e-8 of its largest entry) and the NLL (1e-10 relative); a second call is
  bitwise the first; a site of the batch against a single-site plan at bench.PARITY_TOL["f64"].
* fp32, n = 640, single and a batch of three (refine_solve: the same kernels a second time on the fp64 residual), at the
  bounds of tests/test_gpu_fp32.py.
* one censored fit step (solve_work: r, z, the result and the partial sums in the Laplace step's own work area) at the bounds
  of tests/test_gpu_censored.py.
* the row kernel's path for rows longer than its registers hold -- plans reach it above n = 8192 only -- at small N through
  `dgp_debug_solve`, against the in-register path and against a dense product."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import gp_oracle as orc
from tests.test_gpu_stages import make_case

pytestmark = pytest.mark.gpu

D = 3
SIZES = [128, 256, 384, 1152, 2176]
PADS = [0, 1, 63, 127]
RAGGED = (300, 257, 129, 64, 383)
PARITY_F64 = {"nll_rel": 1e-11, "grad_rel": 1e-9, "alpha_rel": 1e-9, "dnoise_rel": 1e-9}  # bench.PARITY_TOL["f64"]


def test_parity_bounds_are_the_benchmarks():
    import bench

    assert bench.PARITY_TOL["f64"] == PARITY_F64


@functools.lru_cache(maxsize=None)
def _reference(n, seed):
    """-> (X, r, noise, theta, alpha, quad, nll) of a loadest d = 3 case from the oracle; shared, never modified."""
    X, r, noise, theta = make_case("loadest", D, max(n, 8), seed=seed, perturb=0.2)  # (the generator standardises y: n >= 2)
    X, r, noise = X[:n].contiguous(), r[:n].contiguous(), noise[:n].contiguous()
    Khat = orc.GRAMS["loadest"](X, X, theta) + torch.diag(noise)
    L = torch.linalg.cholesky(Khat)
    alpha = torch.cholesky_solve(r[:, None], L)[:, 0]
    z = torch.linalg.solve_triangular(L, r[:, None], upper=False)[:, 0]
    return X, r, noise, theta, alpha, float((z * z).sum()), float(orc.nll_data(Khat, r))


def _plan(n, dev, dtype=torch.float64, batch=1, sizes=None):
    from discontinuum_amd.backend import GPPlan

    p = GPPlan("loadest", n, D, dtype=dtype, device=dev, lookahead=1 if batch > 1 else True, batch=batch)
    if sizes is not None:
        p.set_site_sizes(list(sizes))
    return p


def _check_site(label, out, alpha, n, ref):
    from discontinuum_amd import _lib

    _X, _r, _noise, _theta, alpha_ref, quad_ref, nll_ref = ref
    e_alpha = float((alpha[:n] - alpha_ref).abs().max() / alpha_ref.abs().max())
    e_quad = abs(float(out[_lib.OUT_QUAD]) - quad_ref) / abs(quad_ref)
    e_nll = abs(float(out[_lib.OUT_NLL]) - nll_ref) / abs(nll_ref)
    print(f"one-pass solve {label}: alpha {e_alpha:.2e}, quad {e_quad:.2e}, NLL {e_nll:.2e}")
    assert int(out[_lib.OUT_INFO]) == 0
    assert e_alpha < 1e-8 and e_quad < 1e-10 and e_nll < 1e-10, (e_alpha, e_quad, e_nll)
    if alpha.numel() > n:
        assert alpha[n:].abs().max().item() == 0  # the padding rows are the identity's and r is zero there


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("N", SIZES)
def test_solve_against_the_oracle(N, pad, gpu_device):
    from discontinuum_amd import _lib

    dev, n = gpu_device, N - pad
    ref = _reference(n, 11)
    X, r, noise, theta = ref[:4]
    p = _plan(n, dev)
    assert p.N == N
    p.set_inputs(X.to(dev).contiguous())
    out = p.factorize(theta, r.to(dev), noise.to(dev)).cpu()
    alpha, z = p.buffer(_lib.BUF_ALPHA).cpu(), p.buffer(_lib.BUF_Z).cpu()
    _check_site(f"N={N} n={n}", out, alpha, n, ref)
    out2 = p.factorize(theta, r.to(dev), noise.to(dev)).cpu()
    assert torch.equal(out, out2) and torch.equal(alpha, p.buffer(_lib.BUF_ALPHA).cpu()) and torch.equal(z, p.buffer(_lib.BUF_Z).cpu())
    # the full step leaves the same alpha behind (same kernel, same inputs) and returns it as dNLL/dr
    _o, dr, _dn = p.fit_step(theta, r.to(dev), noise.to(dev))
    assert torch.equal(dr.cpu(), alpha[:n])


@functools.lru_cache(maxsize=None)
def _ragged_batch(dev):
    from discontinuum_amd import _lib

    B, n = len(RAGGED), max(RAGGED)
    refs = [_reference(nb, 20 + b) for b, nb in enumerate(RAGGED)]
    X = torch.full((B, n, D), float("nan"), dtype=torch.float64)
    r = torch.full((B, n), float("nan"), dtype=torch.float64)
    noise = torch.ones((B, n), dtype=torch.float64)
    for b, (nb, ref) in enumerate(zip(RAGGED, refs)):
        X[b, :nb], r[b, :nb], noise[b, :nb] = ref[0], ref[1], ref[2]
    theta = torch.stack([ref[3] for ref in refs])
    p = _plan(n, dev, batch=B, sizes=RAGGED)
    p.set_inputs(X.to(dev).contiguous())
    args = (theta, r.to(dev).contiguous(), noise.to(dev).contiguous())
    out, dr, dnoise = (t.cpu().clone() for t in p.fit_step(*args))
    alpha = torch.stack([p.buffer(_lib.BUF_ALPHA, b).cpu() for b in range(B)])
    return p, args, refs, out, dr, dnoise, alpha


def test_ragged_batch_against_the_oracle_and_repeatable(gpu_device):
    p, args, refs, out, dr, dnoise, alpha = _ragged_batch(gpu_device)
    for b, nb in enumerate(RAGGED):
        _check_site(f"ragged site {b} n={nb}", out[b], alpha[b], nb, refs[b])
        assert torch.equal(dr[b, :nb], alpha[b, :nb])
    out2, dr2, dnoise2 = (t.cpu() for t in p.fit_step(*args))
    assert torch.equal(out, out2) and torch.equal(dr[:, :64], dr2[:, :64]) and torch.equal(dnoise[:, :64], dnoise2[:, :64])
    for b, nb in enumerate(RAGGED):
        assert torch.equal(dr[b, :nb], dr2[b, :nb])


@pytest.mark.parametrize("b", range(len(RAGGED)))
def test_batched_site_against_the_single_site_plan(b, gpu_device):
    from discontinuum_amd import _lib

    dev = gpu_device
    _p, _args, refs, out, dr, dnoise, _alpha = _ragged_batch(dev)
    nb = RAGGED[b]
    X, r, noise, theta = refs[b][:4]
    p1 = _plan(nb, dev)
    p1.set_inputs(X.to(dev).contiguous())
    o1, a1, n1 = (t.cpu() for t in p1.fit_step(theta, r.to(dev), noise.to(dev)))
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max())  # noqa: E731
    g = slice(_lib.OUT_DTHETA, _lib.OUT_DTHETA + theta.numel())
    res = {"nll_rel": abs(float(out[b, _lib.OUT_NLL] - o1[_lib.OUT_NLL])) / abs(float(o1[_lib.OUT_NLL])), "grad_rel": rel(out[b, g], o1[g]),
           "alpha_rel": rel(dr[b, :nb], a1), "dnoise_rel": rel(dnoise[b, :nb], n1)}
    print(f"one-pass solve, batched site {b} (n={nb}) against a single-site plan: {res}")
    assert all(res[k] <= PARITY_F64[k] for k in PARITY_F64), res


def test_fp32_single_and_batch_of_three(gpu_device):
    """n = 640: the refinement runs the solve kernels a second time on the fp64 residual (refine_solve).  Bounds: those of
    tests/test_gpu_fp32.py against the fp64 oracle (alpha 1e-4 of its norm, NLL 1e-4 relative, gradients 5e-4) and between the
    batched and the single-site plan (NLL 2e-5, alpha 5e-5)."""
    from discontinuum_amd import _lib

    dev, n, B = gpu_device, 640, 3
    cases = [make_case("loadest", D, n, seed=40 + b, perturb=0.1) for b in range(B)]
    X = torch.stack([c[0] for c in cases]).float().to(dev).contiguous()
    r = torch.stack([c[1] for c in cases]).float().to(dev).contiguous()
    noise = torch.stack([c[2] for c in cases]).float().to(dev).contiguous()
    theta = torch.stack([c[3] for c in cases])
    pb = _plan(n, dev, dtype=torch.float32, batch=B)
    pb.set_inputs(X)
    out, dr, _ = (t.cpu().clone() for t in pb.fit_step(theta, r, noise))
    out2, dr2, _ = (t.cpu() for t in pb.fit_step(theta, r, noise))
    assert torch.equal(out, out2) and torch.equal(dr, dr2)
    p1 = _plan(n, dev, dtype=torch.float32)
    for b in range(B):
        val, g_theta, g_r, _g_noise = orc.nll_data_and_grads("loadest", *[cases[b][k] for k in (0, 1, 2, 3)])
        p1.set_inputs(X[b].contiguous())
        o1, a1, _ = (t.cpu() for t in p1.fit_step(theta[b], r[b].contiguous(), noise[b].contiguous()))
        for label, o, a in (("batched", out[b], dr[b]), ("single", o1, a1)):
            o = o.double()
            e_nll = abs(float(o[_lib.OUT_NLL]) - float(val)) / abs(float(val))
            e_alpha = float(torch.linalg.norm(a.double() - g_r) / torch.linalg.norm(g_r))
            e_grad = float((o[_lib.OUT_DTHETA:_lib.OUT_DTHETA + theta.shape[1]] - g_theta).abs().max() / g_theta.abs().max())
            print(f"one-pass solve fp32 n={n} site {b} {label}: NLL {e_nll:.2e}, alpha {e_alpha:.2e}, grad {e_grad:.2e}")
            assert int(o[_lib.OUT_INFO]) == 0 and e_nll <= 1e-4 and e_alpha <= 1e-4 and e_grad <= 5e-4, (label, e_nll, e_alpha, e_grad)
        e_nll = abs(float(out[b, 0] - o1[0])) / abs(float(o1[0]))
        e_alpha = float(torch.linalg.norm((dr[b] - a1).double()) / torch.linalg.norm(a1.double()))
        assert e_nll <= 2e-5 and e_alpha <= 5e-5, (e_nll, e_alpha)


@pytest.mark.parametrize("n,d,frac,seed", [(64, 2, 1.0, 7), (129, 3, 0.2, 11)])
def test_censored_fit_step(n, d, frac, seed, gpu_device):
    """solve_work beside the fit step's own solve; set-up and bounds of tests/test_gpu_censored.py (its smallest full cases)."""
    from tests import test_gpu_censored as cen

    case, ref = cen._case("loadest", n, d, frac, seed), cen._reference("loadest", n, d, frac, seed)
    plan = cen._plan(case[0], n, d, gpu_device)
    out, dr, f_hat, stat = cen._fit_step(plan, gpu_device, case)
    cen._check_against(out, dr, f_hat, stat, ref, plan.ntheta, f"one-pass solve, censored n={n} d={d}")
    again = cen._fit_step(plan, gpu_device, case)
    assert torch.equal(out, again[0]) and torch.equal(dr, again[1]) and torch.equal(f_hat, again[2]) and stat == again[3]


def _debug_solve(lib, code, capacity, T, r, n):
    N = T.shape[0]
    z, alpha = torch.full_like(r, float("nan")), torch.full_like(r, float("nan"))
    partials = torch.empty(lib.dgp_debug_solve_partials(N), dtype=T.dtype, device=T.device)
    quad = torch.zeros(8, dtype=T.dtype, device=T.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.dgp_debug_solve(code, capacity, p(T), N, p(r), n, p(z), p(alpha), p(partials), p(quad),
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    return z.cpu(), alpha.cpu(), quad.cpu()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("N,n", [(128, 128), (1152, 1100), (2176, 2176), (4224, 4097)])
def test_rows_longer_than_the_registers_hold(N, n, dtype, gpu_device):
    """Capacity 1 keeps 1024 (fp64) / 2048 (fp32) columns of a row in registers and streams the rest, with their column sums in
    the partials rows -- the path of plans above n = 8192.  Both paths must match the dense product in float64 to the
    precision's rounding of an N-term sum, and each other likewise; above the diagonal blocks T holds NaN: never read."""
    from discontinuum_amd import _lib

    lib, dev = _lib.load(), gpu_device
    g = torch.Generator().manual_seed(N)
    T64 = torch.tril(torch.randn(N, N, generator=g, dtype=torch.float64)) / np.sqrt(N)
    r64 = torch.randn(N, generator=g, dtype=torch.float64)
    blk = torch.arange(N) // 128
    T = T64.to(dtype).clone()
    T[blk[:, None] < blk[None, :]] = float("nan")
    T, r = T.to(dev).contiguous(), r64.to(dtype).to(dev).contiguous()
    Tq, rq = T64.to(dtype).double(), r64.to(dtype).double()
    rq[n:] = 0
    z_ref = Tq @ rq
    a_ref = Tq.T @ z_ref
    code = _lib.F64 if dtype == torch.float64 else _lib.F32
    eps = 2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24
    res = {}
    for capacity in (0, 1):
        z, alpha, quad = _debug_solve(lib, code, capacity, T, r, n)
        ez = float((z.double() - z_ref).abs().max() / (Tq.abs() @ rq.abs()).max())
        ea = float((alpha.double() - a_ref).abs().max() / (Tq.abs().T @ z_ref.abs()).max())
        eq = abs(float(quad[0 if dtype == torch.float64 else 1]) - float(z.double() @ z.double())) / float(z.double() @ z.double())
        print(f"debug solve N={N} n={n} {dtype} capacity {capacity}: z {ez:.2e}, alpha {ea:.2e}, quad {eq:.2e} (eps {eps:.1e})")
        # a sum of N products in floating point: N eps of the sum of magnitudes bounds ANY order; quad is summed in double
        assert ez <= N * eps and ea <= 2 * N * eps and eq <= (4 * eps if dtype == torch.float64 else 2.0 ** -23), (ez, ea, eq)
        if dtype == torch.float32:
            q64 = quad[4:6].contiguous().view(torch.float64)
            assert abs(float(q64[0]) - float(z.double() @ z.double())) <= 1e-12 * float(z.double() @ z.double())
        res[capacity] = (z, alpha)
    assert (res[0][1].double() - res[1][1].double()).abs().max() <= 2 * N * eps * (Tq.abs().T @ z_ref.abs()).max()
