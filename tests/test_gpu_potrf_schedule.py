"""`DGP_OPT_POTRF_SCHEDULE` (batched plans of >= 4 sites): the factorisation left-looking at group level -- each group of four
block columns is updated ONCE, just before it is factored, with everything to its left (one `syrk_strip_kernel` launch of
K = 128 k0, every tile stored once) -- instead of right-looking K = 512 passes over the whole trailing matrix per group
(csrc/dgp_chol.hip::potrf_scheduled, csrc/dgp_schedule.h).

Every tile still receives its k-blocks in ascending gap-free order, and in fp64 a trailing tile starts its accumulators at
-C and continues one k-ordered fma chain per element, so with the panel-by-panel chain (`DGP_OPT_POTRF_SOLVE` = 0) L, L^-1
and everything computed from them are BITWISE what option 0 gives: `torch.equal`, no tolerance.  That is the test that
catches a wrong schedule.  With the group solve (`DGP_OPT_POTRF_SOLVE` = 1: another association of the same sums, as
`DGP_OPT_GROUP_GEMM`) and with the library's default cut the results are held against the dense oracle at the usual
tolerances (fp64 NLL 1e-10, gradients / alpha / dnoise 1e-8; fp32 NLL 1e-4 max(1, n / 1024), rest 1e-2) and against option 0
at 1e-11 (NLL) / 1e-9 (gradients, alpha): the error model of tests/test_gpu_bigtile.py::test_group_panel_gemm_option -- the
panel entries differ by ~cond(L_D) eps <= 1e3 x 1.1e-16 relative, the NLL by less.
What it restates: the Cholesky inside the reference's `mll(output, y)`, engines/gpytorch.py:350-353."""
import pytest
import torch

from oracle import gp_oracle as orc
from tests.test_gpu_bigtile import forced_plan
from tests.test_gpu_stages import make_case

pytestmark = pytest.mark.gpu

# N = 1408 = 11 block columns: three groups, the last one short (three panels); ragged sites
BATCHES = [("loadest", 3, [1300, 1000, 1171, 1300, 900]), ("rating", 2, [1408, 1300, 1408, 1100])]


def ragged_batch(model, d, sizes, seed0):
    B, n = len(sizes), max(sizes)
    cases = [make_case(model, d, nb, seed=seed0 + b, perturb=0.2) for b, nb in enumerate(sizes)]
    X = torch.full((B, n, d), float("nan"), dtype=torch.float64)
    r = torch.full((B, n), float("nan"), dtype=torch.float64)
    noise = torch.full((B, n), float("nan"), dtype=torch.float64)
    for b, (nb, c) in enumerate(zip(sizes, cases)):
        X[b, :nb], r[b, :nb], noise[b, :nb] = c[0], c[1], c[2]
    return cases, X, r, noise, torch.stack([c[3] for c in cases])


def set_schedule(p, schedule, sweep=None, solve=None, overlap=None, tail=None, tail_sweep=None):
    from discontinuum_amd import _lib

    p.set_option(_lib.OPT_POTRF_SCHEDULE, schedule)
    assert p.get_option(_lib.OPT_POTRF_SCHEDULE) == schedule
    for key, v in ((_lib.OPT_POTRF_SWEEP, sweep), (_lib.OPT_POTRF_SOLVE, solve), (_lib.OPT_POTRF_OVERLAP, overlap), (_lib.OPT_POTRF_TAIL, tail),
                   (_lib.OPT_POTRF_TAIL_SWEEP, tail_sweep)):
        if v is not None:
            p.set_option(key, v)
            assert p.get_option(key) == v


def run_and_collect(p, B, theta, r, noise):
    from discontinuum_amd import _lib

    out, dr, dnoise = p.fit_step(theta, r, noise)
    L = [torch.tril(p.buffer(_lib.BUF_A, site=b)).cpu() for b in range(B)]
    T = [torch.tril(p.buffer(_lib.BUF_T, site=b)).cpu() for b in range(B)]
    return out.cpu(), dr.cpu(), dnoise.cpu(), L, T


@pytest.mark.parametrize("model,d,sizes", BATCHES)
@pytest.mark.parametrize("sweep,tail", [(0, 0), (4, 0), (8, 0), (0, 4), (0, 7)])
def test_left_looking_schedule_is_bitwise_the_group_ahead_one_fp64(model, d, sizes, sweep, tail, gpu_device):
    """Step 1 alone (SOLVE off), forced big tiles (4 slots per site: whole rounds of 128 x 128 tiles AND a cut remainder in every
    UPDATE launch): pure left-looking (sweep 0), super-groups of one group (4: today's data flow on one stream) and of two, and
    the last three / seven block columns as a super-group of their own (tail)."""
    from discontinuum_amd import _lib

    dev, B, n = gpu_device, len(sizes), max(sizes)
    cases, X, r, noise, theta = ragged_batch(model, d, sizes, 120)
    pb = forced_plan(model, d, n, None, torch.float64, dev, lookahead=1, batch=B)
    pb.set_option(_lib.OPT_SYRK_SLOTS, 4 * B)  # (a batch shares the bulk update's slots: 4 per site)
    pb.set_option(_lib.OPT_POTRF_SLOTS, 4 * B)  # (the strip updates cut over the whole batch)
    pb.set_site_sizes(sizes)
    pb.set_inputs(X.to(dev).contiguous())
    rd, nd = r.to(dev).contiguous(), noise.to(dev).contiguous()
    set_schedule(pb, 0)
    ref = run_and_collect(pb, B, theta, rd, nd)
    assert bool((ref[0][:, _lib.OUT_INFO] == 0).all())
    set_schedule(pb, 1, sweep=sweep, solve=0, overlap=0, tail=tail, tail_sweep=4)
    new = run_and_collect(pb, B, theta, rd, nd)
    for k in range(3):
        assert torch.equal(new[k], ref[k]), ("out", "alpha", "dnoise")[k]
    for b in range(B):
        assert torch.equal(new[3][b], ref[3][b]), ("L", b)
        assert torch.equal(new[4][b], ref[4][b]), ("T", b)
    # and site 0 against the dense oracle (the bitwise comparison alone would not notice both being wrong)
    val = orc.nll_data_and_grads(model, *cases[0][:3], cases[0][3])[0]
    assert abs(new[0][0, _lib.OUT_NLL].double() - val) / abs(val) < 1e-10


def test_left_looking_schedule_bitwise_with_default_selectors_12x4096(gpu_device):
    """The default tile selectors at 12 sites of n = 4096 (32 block columns, eight groups; the UPDATE launches cut their
    remainder by the default slot count): option 1 with the panel chain against option 0, bitwise."""
    import numpy as np

    from discontinuum_amd import _lib
    from discontinuum_amd.backend import GPPlan

    dev, d, B, n = gpu_device, 3, 12, 4096
    P = 2 * d + 5
    Xs, ys = zip(*[orc.synth_loadest(n, d, seed=40 + b) for b in range(B)])
    X = torch.tensor(np.stack(Xs), device=dev).contiguous()
    y = torch.tensor(np.stack(ys), device=dev).contiguous()
    noise = torch.full((B, n), 0.01, dtype=torch.float64, device=dev)
    g = torch.Generator().manual_seed(11)
    theta = orc.positive(0.3 * torch.randn(B, P, dtype=torch.float64, generator=g))
    pb = GPPlan("loadest", n, d, device=dev, lookahead=1, batch=B)
    pb.set_inputs(X)
    rows = {}
    for opt in (0, 1):
        set_schedule(pb, opt, sweep=0, solve=0, overlap=0, tail=16, tail_sweep=8)
        out, alpha, dnoise = pb.fit_step(theta, y, noise)
        rows[opt] = (out.cpu(), alpha.cpu(), dnoise.cpu(), [torch.tril(pb.buffer(_lib.BUF_A, site=b)).cpu() for b in (0, 5, 11)],
                     [torch.tril(pb.buffer(_lib.BUF_T, site=b)).cpu() for b in (0, 5, 11)])
    assert bool((rows[0][0][:, _lib.OUT_INFO] == 0).all())
    for k in range(3):
        assert torch.equal(rows[1][k], rows[0][k]), k
    for k in (3, 4):
        assert all(torch.equal(a, b) for a, b in zip(rows[1][k], rows[0][k])), k


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model,d,sizes", BATCHES)
@pytest.mark.parametrize("cut", ["default", "solve", "solve+overlap", "solve+overlap+sweep8"])
def test_left_looking_schedule_against_the_oracle(model, d, sizes, dtype, cut, gpu_device):
    """Option 1 with the library's default cut points and with the group solve (alone, overlapped, in super-groups): against
    the dense oracle at the usual tolerances, and in fp64 against option 0 at 1e-11 / 1e-9."""
    from discontinuum_amd import _lib

    dev, B, n = gpu_device, len(sizes), max(sizes)
    cases, X, r, noise, theta = ragged_batch(model, d, sizes, 140)
    pb = forced_plan(model, d, n, None, dtype, dev, lookahead=1, batch=B)
    pb.set_option(_lib.OPT_POTRF_SLOTS, 4 * B + 3)  # (whole rounds of 128 x 128 tiles AND a cut remainder in the strip updates)
    pb.set_site_sizes(sizes)
    pb.set_inputs(X.to(dev, dtype).contiguous())
    rd, nd = r.to(dev, dtype).contiguous(), noise.to(dev, dtype).contiguous()
    set_schedule(pb, 0)
    o0, a0, _ = [t.cpu().double() for t in pb.fit_step(theta, rd, nd)]
    if cut == "default":
        set_schedule(pb, 1)
    else:
        set_schedule(pb, 1, sweep=8 if "sweep8" in cut else 0, solve=1, overlap=1 if "overlap" in cut else 0)
    out, dr, dnoise = [t.cpu().double() for t in pb.fit_step(theta, rd, nd)]
    P = theta.shape[1]
    g = slice(_lib.OUT_DTHETA, _lib.OUT_DTHETA + P)
    for b, (nb, c) in enumerate(zip(sizes, cases)):
        val, g_theta, g_r, g_noise = orc.nll_data_and_grads(model, c[0], c[1], c[2], c[3])
        assert out[b, _lib.OUT_INFO] == 0
        e_nll = (abs(out[b, _lib.OUT_NLL] - val) / abs(val)).item()
        e_g = ((out[b, g] - g_theta).abs().max() / g_theta.abs().max()).item()
        e_a = ((dr[b, :nb] - g_r).abs().max() / g_r.abs().max()).item()
        e_n = ((dnoise[b, :nb] - g_noise).abs().max() / g_noise.abs().max()).item()
        if dtype == torch.float64:
            assert e_nll < 1e-10 and e_g < 1e-8 and e_a < 1e-8 and e_n < 1e-8, (b, e_nll, e_g, e_a, e_n)
            assert abs(out[b, 0] - o0[b, 0]) <= 1e-11 * abs(o0[b, 0])
            assert (out[b, g] - o0[b, g]).abs().max() <= 1e-9 * o0[b, g].abs().max()
            assert (dr[b] - a0[b]).abs().max() <= 1e-9 * a0[b].abs().max()
        else:
            assert e_nll < 1e-4 * max(1.0, nb / 1024) and e_g < 1e-2 and e_a < 1e-2 and e_n < 2e-2, (b, e_nll, e_g, e_a, e_n)


@pytest.mark.parametrize("cut", ["chain", "solve+overlap"])
def test_left_looking_schedule_fp32_batch_of_32_against_single_plans(cut, gpu_device):
    """fp32 sums each pass from zero and subtracts once, so fewer, longer passes round differently: a 32-site batch (the
    headline's batch, at n = 4096: eight groups) under option 1 against single-site plans, within the batched-vs-single bounds of
    tests/test_gpu_fp32.py (NLL 2e-5, alpha 5e-5: two roundings of the same fp64 truth, both refined)."""
    from discontinuum_amd import _lib
    from discontinuum_amd.backend import GPPlan

    dev, model, d, n, B = gpu_device, "loadest", 3, 4096, 32
    cases = [make_case(model, d, n, seed=90 + b, perturb=0.1) for b in range(B)]
    X = torch.stack([c[0] for c in cases]).float().to(dev).contiguous()
    r = torch.stack([c[1] for c in cases]).float().to(dev).contiguous()
    noise = torch.stack([c[2] for c in cases]).float().to(dev).contiguous()
    theta = torch.stack([c[3] for c in cases])
    pb = GPPlan(model, n, d, dtype=torch.float32, device=dev, lookahead=1, batch=B)
    set_schedule(pb, 1, sweep=0, solve=0 if cut == "chain" else 1, overlap=0 if cut == "chain" else 1)
    pb.set_inputs(X)
    out, dr, _ = pb.fit_step(theta, r, noise)
    p1 = GPPlan(model, n, d, dtype=torch.float32, device=dev)
    for b in (0, 13, B - 1):
        p1.set_inputs(X[b].contiguous())
        o1, a1, _ = p1.fit_step(theta[b], r[b].contiguous(), noise[b].contiguous())
        assert int(out[b, _lib.OUT_INFO]) == 0 and int(o1[_lib.OUT_INFO]) == 0
        e_nll = (abs(out[b, 0] - o1[0]) / abs(o1[0])).item()
        e_alpha = (torch.linalg.norm((dr[b] - a1).double()) / torch.linalg.norm(a1.double())).item()
        assert e_nll <= 2e-5, e_nll
        assert e_alpha <= 5e-5, e_alpha
