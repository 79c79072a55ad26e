"""Censored observations in batched plans: ``dgp_laplace_batched_fit_step`` / ``dgp_laplace_batched_factorize`` on ragged batches
against the dense restatement of tests/censored_helpers.py and against single-site plans, the freeze rule (a site's answer does
not depend on its batch-mates' iteration counts), the B = 1 and the nothing-censored identities, the batched bilinear sweep, the
plan state, the error paths and the engine surface (``fit_many(censored=...)``, ``predict_many``, ``annual_flux_many``).

The fixture is a ragged batch of ten loadest sites (d = 2) whose reference Newton counts are 0 / 7 / 8 / 9 and one further site with
a capped row (2 iterations): more than 8 sites (the hyperparameters travel through the plan's scratch), n = 257 at most (two
256-row blocks in the elementwise reductions, N = 384).

Bounds.  Against the dense restatement: the suite's bounds of a batched fit step against the oracle, NLL 1e-10 relative, gradients
and dr 1e-8 of their largest entry, f 1e-9 absolute.  A site in a batch against its single-site plan: the bounds of
tests/test_gpu_headline_shape.py, NLL 1e-11, gradients / dr 1e-9, the sums 1e-9 of max(|sum|, max |dr|); f 1e-9 absolute (f = y~ -
n~ o a with a held to 1e-9 of its largest entry).  The measured figures are in EXPERIMENTS.md ("Censored observations in batched
plans")."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from oracle import gp_oracle as orc
from tests import censored_helpers as ch
from tests import composite_helpers as comp

pytestmark = pytest.mark.gpu

LN2 = 0.6931471805599453
TOL = 1e-10
D = 2
# (n, frac or None = side all 0, seed): reference Newton iterations 8, 9, 9, 9, 9, 0, 7, 9, 9, 9
SITES = ((257, 0.2, 21), (129, 0.5, 22), (64, 1.0, 23), (1, 0.2, 24), (2, 0.2, 25), (128, None, 26), (127, 0.05, 27), (200, 0.8, 28),
         (130, 0.2, 29), (256, 0.35, 30))
REF_ITERATIONS = (8, 9, 9, 9, 9, 0, 7, 9, 9, 9)
CAPPED = (129, "capped", 31)
COMPOSITE = "one column three kinds d=2"
SENTINEL = 12345.0


def _theta():
    theta = torch.full((orc.loadest_ntheta(D),), LN2, dtype=torch.float64)
    return theta * torch.linspace(0.8, 1.3, theta.numel(), dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _case(n, frac, seed):
    """-> (X, y, side, v, m, theta) of a loadest site, shared between tests and never modified."""
    X = torch.tensor(orc.synth_loadest(n, D, seed=seed)[0])
    y, side, v, m = ch.synth(X.numpy(), 0.2 if frac in (None, "capped") else frac, seed)
    if frac is None:
        side = np.zeros_like(side)
    elif frac == "capped":  # one limit 10 sigma above the data: it says nothing
        side = np.zeros_like(side)
        side[5] = -1
        y = y.copy()
        y[5] += 1.0
    for a in (y, side, v, m):
        a.setflags(write=False)
    return X, y, side, v, m, _theta()


@functools.lru_cache(maxsize=None)
def _reference(n, frac, seed):
    X, y, side, v, m, theta = _case(n, frac, seed)
    return ch.laplace("loadest", X, y, side, v, m, theta, tol=TOL)


def _check_inputs(sites):
    """The condition on the INPUTS every test starts with: the reference converges in <= 30 iterations, capped count as expected."""
    for s in sites:
        ref = _reference(*s)
        assert ref["converged"] and ref["iterations"] <= 30, s
        assert ref["capped"] == (1 if s[1] == "capped" else 0), s
        if s in SITES:
            assert ref["iterations"] == REF_ITERATIONS[SITES.index(s)] and ref["halvings"] == 0, (s, ref["iterations"])


def _plan(n, dev, batch=1, sizes=None, model="loadest", dtype=torch.float64):
    from discontinuum_amd.backend import GPPlan

    plan = GPPlan(model, n, D, dtype=dtype, device=dev, lookahead=1 if batch > 1 else True, batch=batch)
    if sizes is not None:
        plan.set_site_sizes(sizes)
    return plan


def _pack(dev, sites, side_tail=0, f_tail=None):
    """Batch-major device arrays of the sites, the unused tails NaN (side: ``side_tail``): X, theta, y, m, v, side, f or None."""
    cases = [_case(*s) for s in sites]
    B, n = len(sites), max(s[0] for s in sites)
    X = torch.full((B, n, D), float("nan"), dtype=torch.float64)
    y, m, v = (torch.full((B, n), float("nan"), dtype=torch.float64) for _ in range(3))
    side = torch.full((B, n), side_tail, dtype=torch.int32)
    for b, (c, s) in enumerate(zip(cases, sites)):
        nb = s[0]
        X[b, :nb], y[b, :nb], m[b, :nb], v[b, :nb] = c[0], torch.tensor(c[1]), torch.tensor(c[4]), torch.tensor(c[3])
        side[b, :nb] = torch.tensor(c[2])
    f = None
    if f_tail is not None:
        f = torch.full((B, n), float(f_tail), dtype=torch.float64)
        for b, s in enumerate(sites):
            f[b, :s[0]] = m[b, :s[0]]
        f = f.to(dev).contiguous()
    theta = torch.stack([c[5] for c in cases])
    return tuple(t.to(dev).contiguous() for t in (X, y, m, v, side)) + (theta, f)


def _batched_plan(dev, sites):
    X, y, m, v, side, theta, _f = _pack(dev, sites)
    plan = _plan(max(s[0] for s in sites), dev, batch=len(sites), sizes=[s[0] for s in sites])
    plan.set_inputs(X)
    return plan, (theta, y, m, v, side)


@functools.lru_cache(maxsize=None)
def _batch_result(dev, sites):
    """One batched ``laplace_fit_step`` of ``sites`` from a cold start, on the host: (out, dr, f_hat, stat); shared, never modified."""
    plan, args = _batched_plan(dev, sites)
    out, dr, f_hat, stat = plan.laplace_fit_step(*args, tol=TOL)
    return out.cpu(), dr.cpu(), f_hat.cpu(), stat


@functools.lru_cache(maxsize=None)
def _single_result(dev, site):
    X, y, side, v, m, theta = _case(*site)
    plan = _plan(site[0], dev)
    plan.set_inputs(X.to(dev).contiguous())
    t = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt).to(dev).contiguous()  # noqa: E731
    args = (theta, t(y), t(m), t(v), t(side, torch.int32))
    out, dr, f_hat, stat = plan.laplace_fit_step(*args, tol=TOL)
    return out.cpu(), dr.cpu(), f_hat.cpu(), stat, plan, args


def _against_reference(b, site, out, dr, f_hat, stat, label):
    nb, ref, nt = site[0], _reference(*site), orc.loadest_ntheta(D)
    ef = float(np.abs(f_hat[b, :nb].numpy() - ref["f"]).max())
    enll = abs(float(out[b, _lib.OUT_NLL]) - ref["nll"]) / abs(ref["nll"])
    edth = float(np.abs(out[b, _lib.OUT_DTHETA:_lib.OUT_DTHETA + nt].numpy() - ref["dtheta"]).max() / np.abs(ref["dtheta"]).max())
    edr = float(np.abs(dr[b, :nb].numpy() - ref["dr"]).max() / np.abs(ref["dr"]).max())
    esum = abs(float(out[b, _lib.OUT_SUM_DR]) - ref["dr"].sum())
    print(f"{label} site {b} n={nb}: |f - ref| {ef:.2e}, NLL rel {enll:.2e}, dtheta {edth:.2e}, dr {edr:.2e}, sum dr {esum:.2e}, "
          f"iterations {stat[b][0]:.0f} (ref {ref['iterations']}), halvings {stat[b][2]:.0f}, capped {stat[b][3]:.0f}")
    assert int(out[b, _lib.OUT_INFO]) == 0
    assert ef <= 1e-9 and enll <= 1e-10 and edth <= 1e-8 and edr <= 1e-8, (b, ef, enll, edth, edr)
    assert esum <= 1e-8 * np.abs(ref["dr"]).max() * nb
    assert abs(stat[b][0] - ref["iterations"]) <= 1 and stat[b][1] <= TOL and stat[b][3] == ref["capped"], (b, stat[b])
    return ef, enll, edth, edr


def _same_search(dev, site, stat, stat1):
    """Iteration count, halvings and capped rows of a site in a batch against its single-site run: equal, except +-1 iteration
    where the single-site max |df| of the deciding iteration lies within a factor 10 of tol."""
    assert stat[3] == stat1[3], (site, stat, stat1)
    if stat[0] == stat1[0]:
        assert stat[2] == stat1[2], (site, stat, stat1)
        return
    assert abs(stat[0] - stat1[0]) == 1, (site, stat, stat1)
    k = int(min(stat[0], stat1[0]))
    dmax = stat1[1]
    if stat1[0] != k:  # the single-site search went on: its max |df| at iteration k
        _o, _d, _f, _s, plan, args = _single_result(dev, site)
        with pytest.raises(_lib.DGPError):
            plan.laplace_fit_step(*args, maxit=k, tol=TOL)
        dmax = plan.laplace_stat[1]
    assert TOL / 10 <= dmax <= 10 * TOL, (site, stat, stat1, dmax)


def _against_other(site, got, b, other, c, label, dev):
    """Site ``b`` of one result against site ``c`` of another (None: a single-site result) at the batched-versus-single bounds."""
    nb, nt = site[0], orc.loadest_ntheta(D)
    out, dr, f_hat, stat = got
    o1, d1, f1, s1 = other[:4]
    if c is not None:
        o1, d1, f1, s1 = o1[c], d1[c], f1[c], s1[c]
    a1 = float(d1[:nb].abs().max())
    assert abs(float(out[b, 0] - o1[0])) <= 1e-11 * abs(float(o1[0])), (label, b)
    gs = slice(_lib.OUT_DTHETA, _lib.OUT_DTHETA + nt)
    edth = float((out[b, gs] - o1[gs]).abs().max() / o1[gs].abs().max())
    edr = float((dr[b, :nb] - d1[:nb]).abs().max()) / a1
    ef = float((f_hat[b, :nb] - f1[:nb]).abs().max())
    assert edth <= 1e-9 and edr <= 1e-9 and ef <= 1e-9, (label, b, edth, edr, ef)
    k = _lib.OUT_SUM_DR
    assert abs(float(out[b, k] - o1[k])) <= 1e-9 * max(abs(float(o1[k])), a1)
    _same_search(dev, site, stat[b], s1)
    return edth, edr, ef


def test_ragged_batch_of_ten_against_the_dense_restatement(gpu_device):
    _check_inputs(SITES)
    got = _batch_result(gpu_device, SITES)
    out, dr, f_hat, stat = got
    assert out.shape == (10, _lib.OUT_LEN) and dr.shape == (10, 257) and f_hat.shape == (10, 257) and len(stat) == 10
    worst = np.max([_against_reference(b, s, *got, "batch of 10") for b, s in enumerate(SITES)], axis=0)
    print(f"ragged batch of 10 against the dense restatement, worst: |f - ref| {worst[0]:.2e}, NLL {worst[1]:.2e}, dtheta {worst[2]:.2e}, "
          f"dr {worst[3]:.2e}")
    assert stat[5] == (0.0, 0.0, 0.0, 0.0)  # the uncensored batch-mate took no iteration
    # a second call on a fresh plan: bitwise the same
    plan, args = _batched_plan(gpu_device, SITES)
    out2, dr2, f2, stat2 = plan.laplace_fit_step(*args, tol=TOL)
    out3, dr3, f3, stat3 = plan.laplace_fit_step(*args, tol=TOL)
    for b, s in enumerate(SITES):
        nb = s[0]
        for x, y_, z in ((out, out2, out3), (dr[:, :nb], dr2[:, :nb], dr3[:, :nb]), (f_hat[:, :nb], f2[:, :nb], f3[:, :nb])):
            assert torch.equal(x[b], y_[b].cpu()) and torch.equal(x[b], z[b].cpu()), b
    assert stat == stat2 == stat3


def test_every_site_against_its_single_site_plan_and_another_batch(gpu_device):
    _check_inputs(SITES)
    dev = gpu_device
    got = _batch_result(dev, SITES)
    worst = np.zeros(3)
    for b, s in enumerate(SITES):
        worst = np.maximum(worst, _against_other(s, got, b, _single_result(dev, s), None, "batch of 10 vs single", dev))
    print(f"batch of 10 against single-site plans, worst: dtheta {worst[0]:.2e}, dr {worst[1]:.2e}, |f - f1| {worst[2]:.2e}; "
          f"iterations {[int(t[0]) for t in got[3]]}")
    # the first three alone: a site's answer does not depend on its batch-mates' iteration counts
    three = _batch_result(dev, SITES[:3])
    worst = np.zeros(3)
    for b, s in enumerate(SITES[:3]):
        worst = np.maximum(worst, _against_other(s, three, b, got, b, "batch of 3 vs batch of 10", dev))
        _against_reference(b, s, *three, "batch of 3")
    print(f"batch of 3 against the batch of 10, worst: dtheta {worst[0]:.2e}, dr {worst[1]:.2e}, |f - f1| {worst[2]:.2e}")


def _raw(plan, dev, arrays, theta, name="dgp_laplace_batched_fit_step", maxit=50, work_bytes=None, f="cold"):
    """A batched entry through ctypes, as it is: -> (return code, out, dr, f, stat, error text)."""
    y, m, v, side = arrays
    lib, B = plan.lib, plan.batch
    fd = m.clone() if f == "cold" else f
    th = (C.c_double * theta.numel())(*theta.reshape(-1).tolist())
    need = max(int(lib.dgp_laplace_batched_workspace_bytes(plan._h)), 1 << 16)
    work = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    base = work.data_ptr() + (-work.data_ptr()) % 256
    out = torch.zeros((B, _lib.OUT_LEN), dtype=torch.float64, device=dev)
    dr = torch.zeros((B, plan.n), dtype=torch.float64, device=dev)
    stat = (C.c_double * (4 * B))()
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    with torch.cuda.device(dev):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        args = (plan._h, th, ptr(y), ptr(m), ptr(v), ptr(side), ptr(fd), maxit, TOL, C.c_void_p(base), need if work_bytes is None else work_bytes,
                ptr(out))
        if name.endswith("fit_step"):
            rc = getattr(lib, name)(*args, ptr(dr), stat, s)
        else:
            rc = getattr(lib, name)(*args, stat, s)
        torch.cuda.synchronize(dev)
    return rc, out.cpu(), dr.cpu(), None if fd is None else fd.cpu(), tuple(stat), lib.dgp_last_error().decode()


def test_one_site_plan_is_bitwise_the_single_site_entries(gpu_device):
    dev, site = gpu_device, SITES[0]
    _check_inputs((site,))
    out1, dr1, f1, stat1, plan, args = _single_result(dev, site)
    theta, y, m, v, side = args
    rc, out, dr, f, stat, msg = _raw(plan, dev, (y, m, v, side), theta)
    assert rc == 0, msg
    assert torch.equal(out[0], out1) and torch.equal(dr[0], dr1) and torch.equal(f, f1) and stat == stat1
    o2, f2, s2 = plan.laplace_factorize(*args, tol=TOL)
    rc, out, _dr, f, stat, msg = _raw(plan, dev, (y, m, v, side), theta, name="dgp_laplace_batched_factorize")
    assert rc == 0, msg
    assert torch.equal(out[0], o2.cpu()) and torch.equal(f, f2.cpu()) and stat == s2


def test_batch_without_a_censored_row_is_the_plain_batched_step_bitwise(gpu_device):
    dev = gpu_device
    sites = ((128, None, 26), (200, None, 28), (65, None, 29))
    plan, (theta, y, m, v, side) = _batched_plan(dev, sites)
    r = (y - m).contiguous()
    out0, dr0, _dn = plan.fit_step(theta, r, v)
    alpha0 = [plan.buffer(_lib.BUF_ALPHA, b).clone() for b in range(3)]
    out0, dr0 = out0.clone(), dr0.clone()
    out1, dr1, f_hat, stat = plan.laplace_fit_step(theta, y, m, v, side, tol=TOL)
    assert torch.equal(out0, out1)
    for b, s in enumerate(sites):
        nb = s[0]
        assert torch.equal(dr0[b, :nb], dr1[b, :nb]) and torch.equal(alpha0[b], plan.buffer(_lib.BUF_ALPHA, b))
        # f = m + K alpha = y - v alpha: the posterior mean at the samples
        assert torch.allclose(f_hat[b, :nb], y[b, :nb] - v[b, :nb] * dr1[b, :nb], rtol=0, atol=1e-14)
    assert stat == ((0.0, 0.0, 0.0, 0.0),) * 3
    outf = plan.factorize(theta, r, v).clone()
    outl, _f, stat = plan.laplace_factorize(theta, y, m, v, side, tol=TOL)
    assert torch.equal(outf, outl) and stat == ((0.0, 0.0, 0.0, 0.0),) * 3


def test_capped_site_in_a_ragged_batch_and_the_ignored_tails(gpu_device):
    dev = gpu_device
    sites = (CAPPED, (200, 0.8, 28), (127, 0.05, 27))
    _check_inputs(sites)
    assert _reference(*CAPPED)["iterations"] == 2
    X, y, m, v, side, theta, f0 = _pack(dev, sites, side_tail=7, f_tail=SENTINEL)
    plan = _plan(200, dev, batch=3, sizes=[s[0] for s in sites])
    plan.set_inputs(X)
    out, dr, f_hat, stat = plan.laplace_fit_step(theta, y, m, v, side, f=f0, tol=TOL)
    got = (out.cpu(), dr.cpu(), f_hat.cpu(), stat)
    for b, s in enumerate(sites):
        _against_reference(b, s, *got, "capped batch")
        assert bool((got[2][b, s[0]:] == SENTINEL).all()), b
    assert stat[0][3] == 1.0 and stat[1][3] == 0.0 and stat[2][3] == 0.0


def test_error_paths(gpu_device):
    dev = gpu_device
    sites = ((129, 0.5, 22), (128, None, 26), (130, 0.2, 29))
    _check_inputs(sites)
    plan, (theta, y, m, v, side) = _batched_plan(dev, sites)
    bad = side.clone()
    bad[2, 5] = 2
    rc, _o, _d, _f, _s, msg = _raw(plan, dev, (y, m, v, bad), theta)
    assert rc == _lib.E_ARG and "side" in msg and "site 2" in msg, msg
    with pytest.raises(_lib.DGPError, match="site 2") as err:
        plan.laplace_fit_step(theta, y, m, v, bad, tol=TOL)
    assert err.value.code == _lib.E_ARG
    rc, _o, _d, _f, _s, msg = _raw(plan, dev, (y, m, v, side), theta, f=None)
    assert rc == _lib.E_ARG and "f_dev" in msg
    rc, _o, _d, _f, _s, msg = _raw(plan, dev, (y, m, v, side), theta, work_bytes=1024)
    assert rc == _lib.E_WORKSPACE
    # too few iterations is a return code: the results are filled, stat says which sites, the plan stays usable
    rc, out, dr, f, stat, msg = _raw(plan, dev, (y, m, v, side), theta, maxit=1)
    assert rc == _lib.E_NOCONV and "converge" in msg and "site 0" in msg, msg
    assert bool(torch.isfinite(out[:, _lib.OUT_NLL]).all()) and bool(torch.isfinite(dr[0, :129]).all()) and bool(torch.isfinite(f[0, :129]).all())
    assert stat[0] == 1.0 and stat[1] > TOL and stat[8] == 1.0 and stat[9] > TOL and stat[4:8] == (0.0, 0.0, 0.0, 0.0)
    with pytest.raises(_lib.DGPError) as err:
        plan.laplace_fit_step(theta, y, m, v, side, maxit=1, tol=TOL)
    assert err.value.code == _lib.E_NOCONV and plan.laplace_stat[0][0] == 1.0 and plan.laplace_stat[1] == (0.0, 0.0, 0.0, 0.0)
    out, dr, f_hat, stat = plan.laplace_fit_step(theta, y, m, v, side, tol=TOL)
    for b, s in enumerate(sites):
        _against_reference(b, s, out.cpu(), dr.cpu(), f_hat.cpu(), stat, "after E_NOCONV")
    # an fp32 plan is refused, by the library and by the plan object
    p32 = _plan(130, dev, batch=3, sizes=[s[0] for s in sites], dtype=torch.float32)
    rc, _o, _d, _f, _s, msg = _raw(p32, dev, (y, m, v, side), theta)
    assert rc == _lib.E_ARG and "float64" in msg
    assert int(p32.lib.dgp_laplace_batched_workspace_bytes(p32._h)) == 0
    with pytest.raises(ValueError, match="float64"):
        p32.laplace_fit_step(theta, y.float(), m.float(), v.float(), side)


def test_batched_bilinear_sweep_alone(gpu_device):
    dev = gpu_device
    sizes = (257, 129, 64, 1, 2, 128, 127, 200, 130)
    B, n = len(sizes), max(sizes)
    rng = np.random.default_rng(7)
    X = torch.full((B, n, D), float("nan"), dtype=torch.float64)
    u, a = (torch.full((B, n), float("nan"), dtype=torch.float64) for _ in range(2))
    theta = torch.stack([_theta() * (1.0 + 0.02 * b) for b in range(B)])
    for b, nb in enumerate(sizes):
        X[b, :nb] = torch.tensor(orc.synth_loadest(nb, D, seed=50 + b)[0])
        u[b, :nb], a[b, :nb] = torch.tensor(rng.standard_normal(nb)), torch.tensor(rng.standard_normal(nb))
    plan = _plan(n, dev, batch=B, sizes=sizes)
    plan.set_inputs(X.to(dev).contiguous())
    got = plan.bilinear(theta, u.to(dev).contiguous(), a.to(dev).contiguous()).cpu()
    again = plan.bilinear(theta, u.to(dev).contiguous(), a.to(dev).contiguous()).cpu()
    assert got.shape == (B, plan.ntheta) and torch.equal(got, again)
    worst = 0.0
    for b, nb in enumerate(sizes):
        ref = ch.bilinear("loadest", X[b, :nb], theta[b], u[b, :nb].numpy(), a[b, :nb].numpy())
        err = float(np.abs(got[b].numpy() - ref).max() / np.abs(ref).max())
        assert err <= 1e-10, (b, nb, err)
        worst = max(worst, err)
    print(f"batched bilinear sweep, 9 ragged loadest sites: {worst:.2e} of the largest entry")
    # a composite model, n = 129 and a shorter batch-mate
    index = comp.by_name(COMPOSITE)
    model = comp.define(comp.CASES[index].spec)
    csizes = (129, 100)
    Xc = torch.full((2, 129, D), float("nan"), dtype=torch.float64)
    uc, ac = (torch.full((2, 129), float("nan"), dtype=torch.float64) for _ in range(2))
    th = torch.stack([comp.CASES[index].theta, comp.CASES[index].theta * 1.05])
    for b, nb in enumerate(csizes):
        Xc[b, :nb] = comp.data(index, nb)[0]
        uc[b, :nb], ac[b, :nb] = torch.tensor(rng.standard_normal(nb)), torch.tensor(rng.standard_normal(nb))
    pc = _plan(129, dev, batch=2, sizes=csizes, model=model)
    pc.set_inputs(Xc.to(dev).contiguous())
    gc = pc.bilinear(th, uc.to(dev).contiguous(), ac.to(dev).contiguous()).cpu()
    for b, nb in enumerate(csizes):
        ref = ch.bilinear(model, Xc[b, :nb], th[b], uc[b, :nb].numpy(), ac[b, :nb].numpy())
        err = float(np.abs(gc[b].numpy() - ref).max() / np.abs(ref).max())
        print(f"batched bilinear sweep composite site {b} n={nb}: {err:.2e} of the largest entry")
        assert err <= 1e-10, (b, nb, err)


def test_plan_state_is_every_sites_laplace_posterior(gpu_device):
    dev = gpu_device
    sites = (SITES[0], SITES[5], SITES[6], CAPPED)
    _check_inputs(sites)
    plan, (theta, y, m, v, side) = _batched_plan(dev, sites)
    _out, f_hat, stat = plan.laplace_factorize(theta, y, m, v, side, tol=TOL)
    Xs = torch.stack([torch.tensor(orc.synth_loadest(50, D, seed=90 + b)[0]) for b in range(len(sites))])
    mu, var = (t.cpu() for t in plan.predict(theta, Xs.to(dev).contiguous()))
    for b, s in enumerate(sites):
        ref = _reference(*s)
        ref_mu, ref_var = ch.posterior("loadest", _case(*s)[0], ref, Xs[b])
        errs = (float((mu[b] - ref_mu).abs().max()), float((var[b] - ref_var).abs().max()))
        print(f"batched censored plan state site {b}: mean {errs[0]:.2e}, variance {errs[1]:.2e}")
        assert max(errs) <= 1e-9 and stat[b][0] == (0.0 if s[1] is None else stat[b][0])
        assert float(np.abs(f_hat[b, :s[0]].cpu().numpy() - ref["f"]).max()) <= 1e-9


def test_engine_fit_many_with_non_detects(gpu_device):
    """``fit_many(censored=masks)`` on three ragged loadest sites, two with about 15 % non-detects (made as
    ``test_gpu_censored.py::test_engine_fit_with_non_detects`` makes them) and one uncensored, against three solo
    ``fit(censored=mask)`` runs (parameters 1e-6: the ``fit_many``-versus-solo bound of test_gpu_engine.py); ``predict_many`` and
    ``annual_flux_many`` against each model's own ``predict`` / ``annual_flux`` (rtol 1e-9), and both away from the fit that takes
    the limits for samples."""
    from discontinuum_amd.loadest_gp import LoadestGP
    from discontinuum_amd.loads import annual_flux_many
    from discontinuum_amd.multisite_fit import fit_many, predict_many
    from tests.flux_helpers import daily_loadest

    data, masks, dailies = [], [], []
    for i, (n, k) in enumerate(((60, 9), (90, 0), (120, 18))):
        cov_obs, target, daily = daily_loadest(n_obs=n, end="2014-01-01", seed=5 + i)
        vals = np.asarray(target.values, dtype=np.float64)
        order = np.argsort(vals)
        mask = np.zeros(n, dtype=bool)
        mask[order[:k]] = True
        reported = vals.copy()
        reported[mask] = vals[order[k]]  # one detection limit: the k lowest samples are reported as "< limit"
        data.append((cov_obs, type(target)(reported, dims=target.dims, coords=target.coords, name=target.name, attrs=target.attrs)))
        masks.append(mask if k else None)
        dailies.append(daily)
    models = [LoadestGP() for _ in data]
    fit_many(models, data, iterations=10, censored=masks)
    for b, (m, (cov, reported), mask) in enumerate(zip(models, data, masks)):
        solo = LoadestGP()
        solo.fit(cov, reported, iterations=10, censored=mask)
        pa = torch.cat([p.detach().reshape(-1) for p in m.model.parameters()])
        pb = torch.cat([p.detach().reshape(-1) for p in solo.model.parameters()])
        print(f"fit_many(censored=) site {b}: parameters against the solo fit {float((pa - pb).abs().max()):.2e}, status {m.laplace_status_}")
        assert float((pa - pb).abs().max()) <= 1e-6, (b, float((pa - pb).abs().max()))
        if mask is None:
            assert m._censor is None and m.laplace_status_ is None
        else:
            it, dmax, _halvings, capped = m.laplace_status_
            assert m._censor is not None and int((m._censor.side != 0).sum()) == int(mask.sum())
            assert it <= 30 and dmax <= m.laplace_tol and capped == 0
    many = predict_many(models, dailies)
    flux = annual_flux_many(models, dailies)
    own = [(m.predict(d), m.annual_flux(d)) for m, d in zip(models, dailies)]
    plain = [LoadestGP() for _ in data]
    fit_many(plain, data, iterations=10)
    sub, sub_flux = predict_many(plain, dailies), annual_flux_many(plain, dailies)
    for b, mask in enumerate(masks):
        (t_s, se_s), f_s = own[b]
        assert np.allclose(many[b][0].values, t_s.values, rtol=1e-9) and np.allclose(many[b][1].values, se_s.values, rtol=1e-9), b
        assert np.allclose(flux[b]["mean"].values, f_s["mean"].values, rtol=1e-9), b
        moved = float(np.max(np.abs(many[b][0].values - sub[b][0].values) / np.abs(sub[b][0].values)))
        moved_flux = float(np.max(np.abs(flux[b]["mean"].values - sub_flux[b]["mean"].values) / np.abs(sub_flux[b]["mean"].values)))
        print(f"site {b}: predict_many / annual_flux_many against substituting the limits {moved:.2e} / {moved_flux:.2e}")
        if mask is not None:
            assert moved > 1e-4 and moved_flux > 1e-4, (b, moved, moved_flux)
