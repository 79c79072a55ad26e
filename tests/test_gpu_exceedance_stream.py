"""GPU parity of ``dgp_posterior_exceedance_moments`` -- the exceedance moments with the posterior covariance produced a panel
of rows at a time from the held factorisation -- and of ``streamed=True`` in the API above it.

1. Against the dense device path on the same plan (``posterior_cov`` + ``exceedance_moments``), float64, with that path's own
   bounds (tests/test_gpu_exceedance.py): a mean entry 1e-13 sum_{i in g} w_i, a covariance entry 1e-11 W_g W_h.  The panels hold
   ``posterior_cov``'s entries; the sums over j are grouped by panel, and sigma_i^2 is the predicted variance instead of the
   buffer's diagonal (another summation order of the same products).
2. Against the dense reference on the ORACLE's posterior covariance: no fixed number; the streamed path may err 4 x what the
   dense device path errs on the same cases (both inherit ``posterior_cov``'s error through rho).
3. float32 plans against the float64 dense device path: the streamed error at most 2 x the dense float32 path's.
4. Ragged batches of 3 and 12 sites (more than 8: the hyperparameters travel through the plan's scratch) against single-site
   plans, 1e-11 like the other products.
5. Work areas and the held fit: NaN / 1e30 in the work area, repeated calls, a work area one byte short, a misaligned one,
   A / T / K^^-1 / alpha and ``predict`` afterwards.
6. ``duration_curve`` / ``exceedance`` with ``streamed=True`` against the default path, 1e-10, and under a byte budget the
   dense path refuses.

A point whose variance is zero to rounding is DECIDED (|z| > 38) on both paths only when its threshold is away from its mean: a
tie there depends on the sign of a rounding error that the two variance computations do not share, so the thresholds of that
point sit one unit from the mean.  A variance that is negative on both paths comes from a negative ``extra_var``.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from discontinuum_amd.backend import GPPlan, _ptr, _stream
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.rating_gp import RatingGP
from oracle import gp_oracle as orc
from tests.exceedance_helpers import dense_exceedance_moments
from tests.exceedance_stream_helpers import stream_bytes
from tests.flux_helpers import daily_loadest, daily_rating
from tests.test_gpu_composite import _case as composite_case
from tests.test_gpu_exceedance import _check, _groups
from tests.test_gpu_influence import _ragged
from tests.test_gpu_stages import make_case

pytestmark = pytest.mark.gpu

TREND = "loadest+trend d=3"
MODELS = ["loadest", "rating", TREND]


def _held(name, n, dev, dtype=torch.float64, seed=0, quiet_point=None):
    """A factorised plan -> (plan, oracle model name, d, X, r, noise, theta); ``quiet_point``: a training row whose noise is 1e-12."""
    if name == TREND:
        model, d, X, r, noise, theta = composite_case(name, n, seed=seed)
    else:
        model, d = name, 3 if name == "loadest" else 2
        # (a synthetic record of one point has no spread to standardise by: NaN -> a number, as the ragged batches do)
        X, r, noise, theta = (torch.nan_to_num(t, nan=0.3) for t in make_case(model, d, n, seed=seed, perturb=0.2))
    noise = noise.clone()
    if quiet_point is not None:
        noise[quiet_point] = 1e-12
    plan = GPPlan(model, n, d, dtype=dtype, device=dev)
    plan.set_inputs(X.to(dev, dtype).contiguous())
    out = plan.factorize(theta, r.to(dev, dtype).contiguous(), noise.to(dev, dtype).contiguous())
    assert int(out[_lib.OUT_INFO]) == 0
    return plan, model, d, X, r, noise, theta


def _points(name, d, m, seed):
    """Test points with neighbours in the first coordinate (high correlations), float64 on the host."""
    if name == "rating":
        return torch.tensor(orc.synth_rating(m, seed)[0])
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(-2.0, 2.0, m))
    return torch.tensor(np.concatenate([t[:, None], rng.standard_normal((m, d - 1))], axis=1))


def _grouping(m, P, kind):
    """``plain``: tests/test_gpu_exceedance.py's ids (excluded points at the head, in the middle, at the tail; an empty group);
    ``gap`` (m = 700): the points 200 .. 519 excluded INSIDE one group's column range -- the whole record for P = 1, group 1 =
    100 .. 599 otherwise -- so that the reduce pass reads Y there: the blocks 256 .. 383 and 384 .. 511 are whole 128-row panels
    of excluded rows, 256 .. 511 a whole 256-row one; the first two points and the last are excluded too;
    ``aligned``: group boundaries at multiples of 256 -- on the cuts of 256-row panels and on every other cut of 128-row ones."""
    if kind == "aligned":
        return np.minimum(np.arange(m) // 256, P - 1).astype(np.int32)
    if kind == "gap":
        i = np.arange(m)
        g = (np.zeros(m) if P == 1 else np.where(i < 100, 0, np.where(i < 600, 1, 2))).astype(np.int32)
        g[:2], g[-1], g[200:520] = -1, -1, -1
        return g
    return _groups(m, P)


def _dense(plan, theta, xs, m, mu, u, w, g, P, ev):
    kmean, cov = plan.posterior_cov(theta, xs)
    return plan.exceedance_moments(cov, m, mu, u, w, g, P, extra_var=ev)


def _scaled(mean, pc, rmean, rcov, w, g, P):
    """(max |mean - ref| / W_g, max |cov - ref| / (W_g W_h)) over the non-empty groups."""
    W = np.bincount(g[g >= 0], weights=w[g >= 0], minlength=P)
    W = np.where(W > 0, W, np.inf)
    return (float(np.max(np.abs(mean - rmean) / W[None, :])), float(np.max(np.abs(pc - rcov) / (W[:, None] * W[None, :])[None])))


# ------------------------------------------------------------------------------------------------ 1. the dense device path
@pytest.mark.parametrize("n", [1, 129, 300])
@pytest.mark.parametrize("name", MODELS)
def test_streamed_moments_match_the_dense_device_path(name, n, gpu_device):
    """Measured on MI355X, worst mean error / W and covariance error / (W_g W_h): loadest 3.7e-16 / 1.6e-16, rating 1.5e-14 /
    5.3e-15, composite 9.2e-16 / 4.3e-16 (bounds 1e-13 and 1e-11)."""
    dev = gpu_device
    quiet = 5 if n >= 129 else None
    plan, model, d, X, _r, _noise, theta = _held(name, n, dev, quiet_point=quiet)
    rng = np.random.default_rng(11)
    worst = [0.0, 0.0]
    for m in (1, 2, 127, 129, 300, 700):
        Xs = _points(name, d, m, seed=3 + m)
        if quiet is not None and m >= 127:
            Xs[40] = X[quiet]  # a test point ON the nearly noise-free training point: variance zero to rounding
        xs = Xs.to(dev).contiguous()
        kmean, var = plan.predict(theta, xs)
        mu = kmean.clone()
        sd = var.clamp_min(1e-300).sqrt().cpu().numpy()
        muh = mu.cpu().numpy()
        w = rng.uniform(0.5, 2.0, m)
        evh = rng.uniform(0.0, 0.05, m)
        if m >= 127:
            evh[41] = -10.0  # sigma^2 < 0 on both paths: decided
        ev_t = torch.tensor(evh, device=dev)
        combos = [(1, 1, "plain"), (3, 5, "plain"), (40, 1, "plain")]
        if m >= 300:
            combos += [(3, 21, "plain"), (40, 5, "plain"), (3, 5, "aligned")]
        if m == 700:
            combos += [(3, 8, "gap"), (1, 2, "gap")]
        for k, (P, L, kind) in enumerate(combos):
            g = _grouping(m, P, kind)
            u = muh[None, :] + sd[None, :] * rng.normal(0.0, 1.2, (L, m))
            if m >= 127:
                u[0, 7], u[0, 90], u[L - 1, 100] = np.inf, -np.inf, np.inf
                u[:, 40] = muh[40] + np.where(np.arange(L) % 2 == 0, 1.0, -1.0)
                u[:, 41] = muh[41] + np.where(np.arange(L) % 2 == 0, -0.5, 0.5)
                if L >= 15:  # (levels of the later chunks)
                    u[9, 60], u[13, 61] = -np.inf, np.inf
            ev = ev_t if k % 2 else None
            ut, wt, gt = torch.tensor(u), torch.tensor(w), torch.tensor(g)
            dmean, dcov = _dense(plan, theta, xs, m, mu, ut, wt, gt, P, ev)
            assert torch.isfinite(dmean).all() and torch.isfinite(dcov).all()
            for R in (128, 256, 768):
                smean, scov = plan.posterior_exceedance_moments(theta, xs, mu, ut, wt, gt, P, extra_var=ev, panel_rows=R)
                assert smean.shape == (L, P) and scov.shape == (L, P, P)
                e = _scaled(smean.cpu().numpy(), scov.cpu().numpy(), dmean.cpu().numpy(), dcov.cpu().numpy(), w, g, P)
                worst = [max(a, b) for a, b in zip(worst, e)]
                print(f"{name} n={n} m={m} P={P} L={L} {kind} ev={ev is not None} R={R}: mean {e[0]:.3e} cov {e[1]:.3e}")
                _check(smean, scov, dmean.cpu().numpy(), dcov.cpu().numpy(), w, g, P, (name, n, m, P, L, kind, ev is not None, R))
    print(f"{name} n={n}: worst streamed - dense: mean / W = {worst[0]:.3e}, cov / (W_g W_h) = {worst[1]:.3e}")


def test_nan_in_gives_nan_out_like_the_dense_path(gpu_device):
    dev, m, P, L = gpu_device, 300, 3, 2
    plan, _model, d, _X, _r, _noise, theta = _held("loadest", 129, dev)
    xs = _points("loadest", d, m, seed=1).to(dev).contiguous()
    kmean, var = plan.predict(theta, xs)
    mu = kmean.clone()
    mu[10] = float("nan")
    g = _grouping(m, P, "plain")
    u = (kmean[None, :] + var.sqrt()[None, :] * torch.randn(L, m, dtype=torch.float64, device=dev)).contiguous()
    w = torch.ones(m, dtype=torch.float64)
    dmean, dcov = _dense(plan, theta, xs, m, mu, u, w, torch.tensor(g), P, None)
    smean, scov = plan.posterior_exceedance_moments(theta, xs, mu, u, w, torch.tensor(g), P, panel_rows=128)
    assert torch.isnan(dmean[:, g[10]]).all() and torch.equal(torch.isnan(smean), torch.isnan(dmean))
    assert torch.equal(torch.isnan(scov), torch.isnan(dcov)) and torch.isnan(scov).any() and not torch.isnan(scov).all()


# ------------------------------------------------------------------------------------------------ 2. the oracle's posterior
@pytest.mark.parametrize("name", MODELS)
def test_streamed_error_against_the_oracle_is_the_dense_paths(name, gpu_device):
    """Both device paths against ``dense_exceedance_moments`` on the oracle's posterior covariance and variances (mean of the
    device): the streamed path's worst scaled error is allowed 4 x the dense path's.  Measured on MI355X, dense / streamed:
    means 2.3e-16 / 2.3e-16 (loadest), 1.1e-15 / 9.3e-16 (rating), 3.4e-16 / 3.4e-16 (composite); covariances 5.7e-18 / 5.6e-18,
    8.5e-17 / 8.4e-17, 1.8e-17 / 2.1e-17."""
    dev, n = gpu_device, 300
    plan, model, d, X, r, noise, theta = _held(name, n, dev)
    rng = np.random.default_rng(21)
    ed, es = [0.0, 0.0], [0.0, 0.0]
    for m, P, L, R in ((129, 3, 5, 128), (300, 3, 8, 128), (300, 1, 1, 256)):
        Xs = _points(name, d, m, seed=7 + m)
        xs = Xs.to(dev).contiguous()
        _omu, ocov = orc.posterior(model, X, r, noise, theta, Xs, full_cov=True)
        C = ocov.numpy()
        C = 0.5 * (C + C.T)
        kmean, _var = plan.predict(theta, xs)
        muh = kmean.cpu().numpy()
        w, g = rng.uniform(0.5, 2.0, m), _grouping(m, P, "plain")
        ev = rng.uniform(0.0, 0.05, m)
        u = muh[None, :] + np.sqrt(np.diagonal(C) + ev)[None, :] * rng.normal(0.0, 1.2, (L, m))
        rmean, rcov = dense_exceedance_moments(C, muh, u, w, g, P, ev)
        args = (kmean, torch.tensor(u), torch.tensor(w), torch.tensor(g), P)
        dmean, dcov = _dense(plan, theta, xs, m, *args, torch.tensor(ev, device=dev))
        smean, scov = plan.posterior_exceedance_moments(theta, xs, *args, extra_var=torch.tensor(ev, device=dev), panel_rows=R)
        ed = [max(a, b) for a, b in zip(ed, _scaled(dmean.cpu().numpy(), dcov.cpu().numpy(), rmean, rcov, w, g, P))]
        es = [max(a, b) for a, b in zip(es, _scaled(smean.cpu().numpy(), scov.cpu().numpy(), rmean, rcov, w, g, P))]
    print(f"{name} vs oracle posterior: dense mean {ed[0]:.3e} cov {ed[1]:.3e}; streamed mean {es[0]:.3e} cov {es[1]:.3e}")
    assert es[0] <= 4 * ed[0] and es[1] <= 4 * ed[1], (ed, es)


# ------------------------------------------------------------------------------------------------ 3. float32 plans
@pytest.mark.parametrize("name", ["loadest", "rating"])
def test_float32_streamed_error_is_the_dense_float32_paths(name, gpu_device):
    """float32 plans, n = 300, m = 300 and 700, against the float64 dense device path on the same inputs: the streamed float32
    error at most 2 x the dense float32 error.  Measured on MI355X, dense / streamed: means 4.9e-8 / 2.0e-8 (loadest), 1.8e-6 /
    5.5e-7 (rating); covariances 2.2e-8 / 1.7e-8, 3.4e-7 / 2.8e-7."""
    dev, n = gpu_device, 300
    p64, _model, d, _X, _r, _noise, theta = _held(name, n, dev)
    p32 = _held(name, n, dev, dtype=torch.float32)[0]
    rng = np.random.default_rng(31)
    ed, es = [0.0, 0.0], [0.0, 0.0]
    for m, P, L, R in ((300, 3, 5, 128), (700, 3, 2, 256), (700, 40, 1, 128)):
        Xs = _points(name, d, m, seed=9 + m)
        x64, x32 = Xs.to(dev).contiguous(), Xs.to(dev, torch.float32).contiguous()
        kmean, var = p64.predict(theta, x64)
        mu32 = kmean.float()
        mu64 = mu32.double()  # the same mean on every path
        w, g = rng.uniform(0.5, 2.0, m), _grouping(m, P, "plain")
        ev = rng.uniform(0.01, 0.05, m)
        u = torch.tensor(mu64.cpu().numpy()[None, :] + np.sqrt(var.cpu().numpy() + ev)[None, :] * rng.normal(0.0, 1.2, (L, m)))
        wt, gt = torch.tensor(w), torch.tensor(g)
        rmean, rcov = (t.cpu().numpy() for t in _dense(p64, theta, x64, m, mu64, u, wt, gt, P, torch.tensor(ev, device=dev)))
        ev32 = torch.tensor(ev, device=dev, dtype=torch.float32)
        dmean, dcov = _dense(p32, theta, x32, m, mu32, u, wt, gt, P, ev32)
        smean, scov = p32.posterior_exceedance_moments(theta, x32, mu32, u, wt, gt, P, extra_var=ev32, panel_rows=R)
        ed = [max(a, b) for a, b in zip(ed, _scaled(dmean.cpu().numpy(), dcov.cpu().numpy(), rmean, rcov, w, g, P))]
        es = [max(a, b) for a, b in zip(es, _scaled(smean.cpu().numpy(), scov.cpu().numpy(), rmean, rcov, w, g, P))]
    print(f"{name} float32 vs float64 dense: dense mean {ed[0]:.3e} cov {ed[1]:.3e}; streamed mean {es[0]:.3e} cov {es[1]:.3e}")
    assert es[0] <= 2 * ed[0] and es[1] <= 2 * ed[1], (ed, es)


# ------------------------------------------------------------------------------------------------ 4. ragged batches
@pytest.mark.parametrize("model,d,sizes", [("loadest", 3, [300, 129, 257]),
                                           ("rating", 2, [129, 64, 200, 1, 2, 127, 128, 130, 77, 150, 199, 33])])
def test_ragged_batches_match_single_site_plans(model, d, sizes, gpu_device):
    dev, m, P, L, B = gpu_device, 300, 3, 5, len(sizes)
    pb, cases, theta, Xs = _ragged(model, d, sizes, m, dev, seed0=80)
    assert not torch.equal(theta[0], theta[1])
    xs = Xs.to(dev).contiguous()
    rng = np.random.default_rng(41)
    kmean, var = pb.predict(theta, xs)
    u = kmean[:, None, :] + var.sqrt()[:, None, :] * torch.tensor(rng.normal(0.0, 1.2, (B, L, m)), device=dev)
    w = torch.tensor(rng.uniform(0.5, 2.0, (B, m)))
    g = torch.tensor(np.stack([_grouping(m, P, "plain")] * B))
    ev = torch.tensor(rng.uniform(0.0, 0.05, (B, m)), device=dev)
    first = pb.posterior_exceedance_moments(theta, xs, kmean, u, w, g, P, extra_var=ev, panel_rows=128)
    again = pb.posterior_exceedance_moments(theta, xs, kmean, u, w, g, P, extra_var=ev, panel_rows=128)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert first[0].shape == (B, L, P) and first[1].shape == (B, L, P, P)
    worst = [0.0, 0.0]
    for b, (nb, c) in enumerate(zip(sizes, cases)):
        p1 = GPPlan(model, nb, d, device=dev)
        p1.set_inputs(c[0].to(dev).contiguous())
        p1.factorize(c[3], c[1].to(dev).contiguous(), c[2].to(dev).contiguous())
        one = p1.posterior_exceedance_moments(c[3], xs[b], kmean[b], u[b], w[b], g[b], P, extra_var=ev[b], panel_rows=128)
        e = _scaled(first[0][b].cpu().numpy(), first[1][b].cpu().numpy(), one[0].cpu().numpy(), one[1].cpu().numpy(),
                    w[b].numpy(), g[b].numpy(), P)
        worst = [max(a, b_) for a, b_ in zip(worst, e)]
    print(f"{model} ragged batch of {B}: worst scaled difference to the single-site plans mean {worst[0]:.2e} cov {worst[1]:.2e}")
    assert max(worst) <= 1e-11, worst


# ------------------------------------------------------------------------------------------------ 5. work areas, the held fit
def test_work_area_contents_do_not_matter_and_the_held_fit_survives(gpu_device):
    dev, name, n, m, P, L = gpu_device, "rating", 300, 700, 3, 5
    X, r, noise, theta = make_case(name, 2, n, seed=4, perturb=0.2)
    p = GPPlan(name, n, 2, device=dev)
    p.set_inputs(X.to(dev).contiguous())
    out, _dr, _dn = p.fit_step(theta, r.to(dev), noise.to(dev))
    assert int(out[_lib.OUT_INFO]) == 0
    xs = _points(name, 2, m, seed=2).to(dev).contiguous()
    bufs = (_lib.BUF_A, _lib.BUF_T, _lib.BUF_S, _lib.BUF_ALPHA, _lib.BUF_XT)
    before = [p.buffer(b).clone() for b in bufs] + list(p.predict(theta, xs))
    kmean, var = before[-2], before[-1]
    rng = np.random.default_rng(51)
    gh = _grouping(m, P, "gap")  # whole 128- and 256-row panels of excluded points inside group 1's column range
    assert np.all(gh[256:512] == -1) and gh[199] == 1 and gh[520] == 1
    g = torch.tensor(gh)
    u = (kmean[None, :] + var.sqrt()[None, :] * torch.tensor(rng.normal(0.0, 1.2, (L, m)), device=dev)).contiguous()
    w = torch.tensor(rng.uniform(0.5, 2.0, m))
    args = (theta, xs, kmean, u, w, g, P)
    dmean, dcov = _dense(p, theta, xs, m, kmean, u, w, g, P, None)
    for R in (128, 256):
        first = p.posterior_exceedance_moments(*args, panel_rows=R)
        assert torch.isfinite(first[0]).all() and torch.isfinite(first[1]).all()
        ws = p._pex_ws[: p._pex_ws.numel() // 8 * 8].view(torch.float64)
        half = ws.numel() // 2
        ws[:half] = float("nan")
        ws[half:] = 1e30
        dirty = p.posterior_exceedance_moments(*args, panel_rows=R)
        _check(dirty[0], dirty[1], dmean.cpu().numpy(), dcov.cpu().numpy(), w.numpy(), gh, P, ("NaN work area", R))
        ws[:half] = 1e30
        ws[half:] = float("nan")
        other_half = p.posterior_exceedance_moments(*args, panel_rows=R)
        assert torch.equal(first[0], other_half[0]) and torch.equal(first[1], other_half[1]), R
        ws.zero_()
        clean = p.posterior_exceedance_moments(*args, panel_rows=R)
        for other in (dirty, clean, p.posterior_exceedance_moments(*args, panel_rows=R)):
            assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1]), R
        assert torch.equal(first[1], first[1].transpose(-1, -2))
    after = [p.buffer(b) for b in bufs] + list(p.predict(theta, xs))
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    # the C entry: the documented size, one byte short, a misaligned work area
    lib = p.lib
    need = int(lib.dgp_posterior_exceedance_moments_workspace_bytes(p._h, m, P, L, 128))
    assert need == stream_bytes(n, m, 2, P, L, 8, 128)
    assert int(lib.dgp_posterior_exceedance_moments_workspace_bytes(p._h, m, P, L, 256)) == stream_bytes(n, m, 2, P, L, 8, 256)
    work = torch.empty(need + 512, dtype=torch.uint8, device=dev)
    base = work.data_ptr() + (-work.data_ptr()) % 256
    th = (C.c_double * theta.numel())(*theta.tolist())
    mean_out = torch.empty(L, P, dtype=torch.float64, device=dev)
    cov_out = torch.empty(L, P, P, dtype=torch.float64, device=dev)
    wd, gd = w.to(dev), g.to(dev)

    def call(ptr, nbytes):
        return lib.dgp_posterior_exceedance_moments(p._h, th, _ptr(xs), m, _ptr(kmean), _ptr(u), L, _ptr(wd), _ptr(gd), P,
                                                    None, 128, C.c_void_p(ptr), nbytes, _ptr(mean_out), _ptr(cov_out), _stream())

    assert call(base, need - 1) == -3 and b"workspace" in lib.dgp_last_error()
    assert call(base + 8, need) == -1 and b"aligned" in lib.dgp_last_error()
    assert call(base, need) == 0
    torch.cuda.synchronize(dev)
    first = p.posterior_exceedance_moments(*args, panel_rows=128)
    assert torch.equal(mean_out, first[0]) and torch.equal(cov_out, first[1])
    # no factorisation: DGP_E_STATE
    q = GPPlan(name, n, 2, device=dev)
    q.set_inputs(X.to(dev).contiguous())
    with pytest.raises(_lib.DGPError, match="factorisation"):
        q.posterior_exceedance_moments(*args, panel_rows=128)


# ------------------------------------------------------------------------------------------------ 6. the engines
def _close(a, b, names=("mean", "se", "lower", "upper")):
    worst = 0.0
    for k in names:
        x, y = np.asarray(a[k].values, dtype=np.float64), np.asarray(b[k].values, dtype=np.float64)
        worst = max(worst, float(np.max(np.abs(x - y) / np.maximum(1.0, np.abs(y)))))
    return worst


def test_engines_streamed_against_the_default_path_and_under_a_small_budget(gpu_device):
    cov_obs, target, unc, daily = daily_rating(n_obs=150, seed=12)
    rating = RatingGP()
    rating.fit(cov_obs, target, target_unc=unc, iterations=10)
    m = len(daily.coords["time"].values)
    dense = rating.duration_curve(daily)
    streamed = rating.duration_curve(daily, streamed=True)
    e = _close(streamed, dense)
    print(f"rating duration curve (21 levels, m = {m}): streamed - dense {e:.3e}")
    assert e <= 1e-10 and rating._plan.exceedance_panel_rows(m, 1, 21) == -(-m // 128) * 128  # the default budget: one panel
    budget = 8_000_000
    with pytest.raises(ValueError, match="pass streamed=True"):
        rating.duration_curve(daily, max_bytes=budget)
    small = rating.duration_curve(daily, max_bytes=budget, streamed=True)
    R = rating._plan.exceedance_panel_rows(m, 1, 21, max_bytes=budget)  # what the call above picked
    need = int(rating._plan.lib.dgp_posterior_exceedance_moments_workspace_bytes(rating._plan._h, m, 1, 21, R))
    more = int(rating._plan.lib.dgp_posterior_exceedance_moments_workspace_bytes(rating._plan._h, m, 1, 21, R + 128))
    assert 128 <= R < -(-m // 128) * 128 and need <= budget < more
    e = _close(small, dense)
    print(f"rating duration curve under {budget} bytes: panel rows {R}, work area {need} bytes, streamed - dense {e:.3e}")
    assert e <= 1e-10

    cov_obs, target, daily = daily_loadest(n_obs=200, seed=11)
    model = LoadestGP()
    model.fit(cov_obs, target, iterations=10)
    tau = np.array([0.9, 1.3])
    dense, dcov = model.exceedance(daily, threshold=tau, freq="YE", return_cov=True)
    streamed, scov = model.exceedance(daily, threshold=tau, freq="YE", return_cov=True, streamed=True)
    e = _close(streamed, dense)
    ec = float(np.max(np.abs(scov - dcov)) / max(1.0, float(np.max(np.abs(dcov)))))
    print(f"loadest exceedance (YE): streamed - dense {e:.3e}, covariance {ec:.3e}")
    assert e <= 1e-10 and ec <= 1e-10
    with pytest.raises(ValueError, match="pass streamed=True"):
        model.exceedance(daily, threshold=tau, freq="YE", max_bytes=budget)
    small = model.exceedance(daily, threshold=tau, freq="YE", max_bytes=budget, streamed=True)
    md = len(daily.coords["time"].values)
    assert model._plan.exceedance_panel_rows(md, dense["mean"].values.shape[1], 2, max_bytes=budget) < -(-md // 128) * 128
    assert _close(small, dense) <= 1e-10
    flux = model.exceedance(daily, threshold=[300.0], kind="flux")
    assert _close(model.exceedance(daily, threshold=[300.0], kind="flux", streamed=True), flux) <= 1e-10
    dc = model.duration_curve(daily, levels=tau)
    assert _close(model.duration_curve(daily, levels=tau, streamed=True), dc) <= 1e-10
