"""GPU parity of ``dgp_exceedance_moments`` (exact moments of threshold-exceedance counts), of its pair function and of the
API above it: ``LoadestGP.exceedance``, ``RatingGP.duration_curve``.

References (tests/exceedance_helpers.py, numpy / scipy, vectorised): the pair function by Owen's T -- it agrees with scipy's
bivariate normal and with quadrature of Plackett's integral to 1.2e-14 (tests/test_exceedance_cpu.py asserts 1e-13) --
and the dense moments built on it, evaluated on the SAME ``dgp_posterior_cov`` buffer, symmetrised from its lower triangle.
Bounds: the pair function 1e-12 absolute (two orders over the reference's own error, for the device's erfc / asin), the
rho = +-1 closed forms 1e-15; a mean entry 1e-13 sum_{i in g} w_i; a covariance entry 1e-11 (sum_{i in g} w_i)(sum_{j in h}
w_j) -- the pointwise bound summed over the pairs, times ten for summation order.  float32 buffers are compared with the
same reference on the float32 values cast to double: the arithmetic after the loads is double, so the bounds are the same.
"""
import numpy as np
import pytest
import torch
from scipy.special import ndtr

from discontinuum_amd.backend import GPPlan, bvn_excess, exceedance_moments
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.loads import period_groups, target_transform
from discontinuum_amd.rating_gp import RatingGP
from oracle import gp_oracle as orc
from tests.exceedance_helpers import ExceedOraclePlan, bvn_excess_ref, dense_exceedance_moments, design_set
from tests.flux_helpers import daily_loadest, daily_rating, symmetrise_lower
from tests.test_gpu_stages import make_case

pytestmark = pytest.mark.gpu


def test_pair_function_on_the_design_set(gpu_device):
    dev = gpu_device
    h, k, r = design_set(1000, seed=0)
    assert h.size >= 20_000
    dv = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    got = bvn_excess(dv(h), dv(k), dv(r)).cpu().numpy()
    ref = bvn_excess_ref(h, k, r)
    err = np.abs(got - ref)
    for rr in np.unique(np.abs(r)):
        print(f"|rho| = {rr:.10f}: max |D - ref| = {err[np.abs(r) == rr].max():.3e}")
    assert err.max() <= 1e-12, (err.max(), h[err.argmax()], k[err.argmax()], r[err.argmax()])
    edge = np.abs(r) == 1
    ph, pk = ndtr(h[edge]), ndtr(k[edge])
    closed = np.where(r[edge] > 0, np.minimum(ph, pk), np.maximum(0.0, ph + pk - 1.0)) - ph * pk
    assert np.abs(got[edge] - closed).max() <= 1e-15
    # rho beyond [-1, 1] is clamped; decided and NaN arguments
    sp = bvn_excess(dv([0.3, 0.3, np.inf, 0.2, np.nan, 0.1, -40.0]), dv([-0.2, -0.2, 0.1, -np.inf, 0.1, 0.2, 0.0]),
                    dv([1.5, -1.5, 0.5, 0.99, 0.5, np.nan, 0.95])).cpu().numpy()
    assert abs(sp[0] - (ndtr(-0.2) - ndtr(0.3) * ndtr(-0.2))) <= 1e-15 and abs(sp[1] - (ndtr(0.3) + ndtr(-0.2) - 1 - ndtr(0.3) * ndtr(-0.2))) <= 1e-15
    assert sp[2] == 0 and sp[3] == 0 and np.isnan(sp[4]) and np.isnan(sp[5]) and sp[6] == 0


def _posterior_buffers(model, dev, dtype, ms, n=160, seed=0):
    """{m: ((M, M) dgp_posterior_cov buffer, (m,) mean)} from one factorised plan."""
    d = 2
    X, r, noise, theta = make_case(model, d, n, seed=seed)
    plan = GPPlan(model, n, d, dtype=dtype, device=dev)
    plan.set_inputs(X.to(dev, dtype).contiguous())
    plan.factorize(theta, r.to(dev, dtype).contiguous(), noise.to(dev, dtype).contiguous())
    out = {}
    for m in ms:
        if model == "loadest":
            g = torch.Generator().manual_seed(seed + m)
            Xs = torch.rand(m, d, generator=g, dtype=torch.float64) * 4 - 2
            Xs[:, 0] = torch.sort(Xs[:, 0]).values  # neighbours in time: high correlations
        else:
            Xs = torch.tensor(orc.synth_rating(m, seed + m)[0])
        mean, cov = plan.posterior_cov(theta, Xs.to(dev, dtype).contiguous())
        out[m] = (cov, mean)
    return out


def _groups(m, P):
    g = (np.arange(m) * P // max(m, 1)).astype(np.int32) if m >= P else np.arange(m, dtype=np.int32) * (P // m)
    if m > 4:  # excluded points at the head, in the middle and at the tail
        g[:2] = -1
        g[m // 2] = -1
        g[-1] = -1
    if m >= 100 and P >= 3:  # an empty group in the middle
        g[g == 1] = 2 if P > 2 else 1
    return g


def _check(mean, pc, rmean, rcov, w, g, P, tag):
    W = np.bincount(g[g >= 0], weights=w[g >= 0], minlength=P)
    mean, pc = mean.cpu().numpy(), pc.cpu().numpy()
    em = np.abs(mean - rmean) - 1e-13 * W[None, :]
    ec = np.abs(pc - rcov) - 1e-11 * (W[:, None] * W[None, :])[None]
    assert np.all(em <= 0), (tag, "mean", float(np.max(np.abs(mean - rmean) / np.where(W > 0, W, 1.0)[None, :])))
    assert np.all(ec <= 0), (tag, "cov", float(np.max(np.abs(pc - rcov) / np.where(W > 0, W, 1.0)[None, :, None] / np.where(W > 0, W, 1.0)[None, None, :])))
    assert np.array_equal(pc, np.swapaxes(pc, 1, 2)), tag
    return (float(np.max(np.abs(mean - rmean) / np.where(W > 0, W, np.inf)[None, :])),
            float(np.max(np.abs(pc - rcov) / np.where(W > 0, W, np.inf)[None, :, None] / np.where(W > 0, W, np.inf)[None, None, :])))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model", ["loadest", "rating"])
def test_moments_match_the_dense_reference(model, dtype, gpu_device):
    dev = gpu_device
    ms = (1, 2, 127, 129, 300)
    bufs = _posterior_buffers(model, dev, dtype, ms)
    rng = np.random.default_rng(5)
    worst = [0.0, 0.0]
    for m in ms:
        cov, mean = bufs[m]
        cov = cov.clone()
        if m >= 127:  # a zero-variance point: its row and column of the lower triangle, and the diagonal
            cov[40, :41] = 0
            cov[40:, 40] = 0
        C = symmetrise_lower(cov[:m, :m].double()).cpu().numpy()
        mu = mean.clone()
        sd = np.sqrt(np.clip(np.diagonal(C), 1e-300, None))
        w = rng.uniform(0.5, 2.0, m)
        ev_t = torch.tensor(rng.uniform(0.0, 0.05, m), dtype=dtype, device=dev)
        # L = 15 and 21 at m = 300: every chunk size of the level loop (8 + 4 + 2 + 1, 8 + 8 + 4 + 1), later chunks starting
        # at l0 > 0 with more than one level -- the path duration_curve's 21 default levels take
        for L in (1, 5, 15, 21) if m == 300 else (1, 5):
            u = mu.double().cpu().numpy()[None, :] + sd[None, :] * rng.normal(0.0, 1.2, (L, m))
            if m >= 127:
                u[0, 7], u[0, 90], u[L - 1, 100] = np.inf, -np.inf, np.inf
                if L >= 15:  # (levels of the later chunks)
                    u[9, 60], u[13, 61] = -np.inf, np.inf
                u[0, 40] = float(mu[40])  # the tie on the zero-variance point: not exceeded
            for P in (1, 3, 40) if L <= 5 else (3,):
                g = _groups(m, P)
                for ev in (None, ev_t):
                    got_mean, got_cov = exceedance_moments(cov, m, mu, torch.tensor(u), torch.tensor(w), torch.tensor(g), P, extra_var=ev)
                    rmean, rcov = dense_exceedance_moments(C, mu.double().cpu().numpy(), u, w, g, P,
                                                           None if ev is None else ev.double().cpu().numpy())
                    e = _check(got_mean, got_cov, rmean, rcov, w, g, P, (model, dtype, m, L, P, ev is not None))
                    worst = [max(a, b) for a, b in zip(worst, e)]
    print(f"{model} {dtype}: worst mean error / W = {worst[0]:.3e}, worst cov error / (W_g W_h) = {worst[1]:.3e}")


def test_structure_repeatable_symmetric_batch_independent(gpu_device):
    dev = gpu_device
    sizes, P, L = (1500, 1100, 700), 12, 3
    bufs = [_posterior_buffers("loadest", dev, torch.float64, (1500,), seed=s)[1500] for s in (3, 4, 5)]
    M = bufs[0][0].shape[0]
    assert M == 1536
    rng = np.random.default_rng(7)
    mus = torch.stack([b[1] for b in bufs])
    sds = torch.stack([torch.diagonal(b[0])[:1500].clamp_min(1e-300).sqrt() for b in bufs])
    thr = mus[:, None, :] + sds[:, None, :] * torch.tensor(rng.normal(0.0, 1.0, (3, L, 1500)), device=dev)
    ws = torch.tensor(rng.uniform(0.5, 2.0, (3, 1500)), device=dev)
    gs = np.stack([np.where(np.arange(1500) < mb, np.arange(1500) * P // mb, -1).astype(np.int32) for mb in sizes])
    cov3 = torch.stack([b[0] for b in bufs]).contiguous()
    args = (cov3, 1500, mus, thr, ws, torch.tensor(gs, device=dev), P)
    mean_a, cov_a = exceedance_moments(*args)
    mean_b, cov_b = exceedance_moments(*args)
    assert torch.equal(mean_a, mean_b) and torch.equal(cov_a, cov_b)
    assert torch.equal(cov_a, cov_a.transpose(-1, -2)) and torch.isfinite(cov_a).all() and mean_a.shape == (3, L, P)
    for b, mb in enumerate(sizes):
        Mb = -(-mb // 128) * 128
        single = bufs[b][0][:Mb, :Mb].contiguous()
        mean1, cov1 = exceedance_moments(single, mb, mus[b, :mb], thr[b, :, :mb], ws[b, :mb], torch.tensor(gs[b, :mb], device=dev), P)
        assert torch.equal(mean_a[b], mean1) and torch.equal(cov_a[b], cov1), b
    # a diagonal covariance: independent points
    m = 1500
    var = torch.tensor(rng.uniform(0.5, 2.0, M), device=dev)
    mu, w, g = mus[0], ws[0], torch.tensor(gs[0], device=dev)
    mean_d, cov_d = exceedance_moments(torch.diag(var).contiguous(), m, mu, thr[0], w, g, P)
    p = torch.special.ndtr((mu[None, :] - thr[0]) / var[:m].sqrt()[None, :])
    A = torch.nn.functional.one_hot(g.long(), P).double()
    W = (w[:, None] * A).sum(0)
    want = torch.diag_embed((w[None, :, None] ** 2 * (p * (1 - p))[:, :, None] * A[None]).sum(1))
    off = ~torch.eye(P, dtype=torch.bool, device=dev)
    assert float(cov_d[:, off].abs().max()) == 0.0  # rho = 0: no period covariance at all
    dg, wdg = torch.diagonal(cov_d, dim1=1, dim2=2), torch.diagonal(want, dim1=1, dim2=2)
    assert float(((dg - wdg).abs() / wdg).max()) <= 1e-13
    assert float(((mean_d - (w[None, :] * p) @ A).abs() / W[None, :]).max()) <= 1e-13
    # identical rows: rho = 1 everywhere, equal thresholds -> every count is (sum w) times one coin
    # (variance 1/4: 1 / sigma = 2 and rho = 1 exactly; a rho one ulp below 1 already moves D by sqrt(1 - rho^2) ~ 1e-8)
    ones = torch.full((M, M), 0.25, dtype=torch.float64, device=dev)
    mu1 = torch.full((m,), 0.2, dtype=torch.float64, device=dev)
    levels = torch.tensor([-0.3, 0.2, 0.9], dtype=torch.float64, device=dev)
    mean_1, cov_1 = exceedance_moments(ones, m, mu1, levels[:, None].expand(L, m).contiguous(), w, g, P)
    p1 = torch.special.ndtr((0.2 - levels) / 0.5)
    want1 = (p1 * (1 - p1))[:, None, None] * (W[:, None] * W[None, :])[None]
    assert float(((cov_1 - want1).abs() / (W[:, None] * W[None, :])[None]).max()) <= 1e-13


def _record(model):
    """Make the model's plan keep the arguments of its ``exceedance_moments`` calls."""
    calls, real = [], model._plan.exceedance_moments

    def spy(cov, m, mu, thresh, w, groups, ngroups, extra_var=None):
        calls.append((cov, m, mu, thresh, w, groups, ngroups, extra_var))
        return real(cov, m, mu, thresh, w, groups, ngroups, extra_var=extra_var)

    model._plan.exceedance_moments = spy
    return calls


def _oracle_posterior(model, daily):
    """The oracle's posterior at the daily points, at the model's fitted parameters (model space)."""
    model._ensure_factor()
    x = model._train_x.cpu().double()
    with torch.no_grad():
        r = (model._train_y - model.model.prior_mean(model._train_x)).cpu().double()
        noise = model.likelihood.train_noise(torch.device("cpu"), torch.float64).reshape(-1)
        xs = torch.tensor(model.dm.Xnew(daily), dtype=torch.float64)
        kmean, cov = orc.posterior(model._plan.model, x, r, noise, model._factor_theta.cpu().double(), xs, full_cov=True)
        mu = kmean + model.model.prior_mean(xs.to(model.device)).cpu().double()
    return mu.numpy(), cov.numpy()


def test_exceedance_and_duration_curve_end_to_end(gpu_device):
    """``LoadestGP.exceedance`` and ``RatingGP.duration_curve`` on the device against the oracle-backed double's
    ``exceedance_moments`` (the dense reference) at the same fitted parameters.  On the covariance the device formed, the
    bounds of the moment test hold; with the oracle's own posterior in place of it the two factorisations differ by about
    1e-9 (tests/test_gpu_flux.py), so that second comparison asserts 1e-8 of the period's weight, for both models.
    ``duration_curve`` also runs with its 21 default levels (chunks of 8 + 8 + 4 + 1 levels)."""
    cov_obs, target, daily = daily_loadest(n_obs=200, seed=11)
    model = LoadestGP()
    model.fit(cov_obs, target, iterations=10)
    calls = _record(model)
    _mode, s, t = target_transform(model.dm)
    tau = np.array([0.9, 1.3])
    ds, pcov = model.exceedance(daily, threshold=tau, freq="YE", return_cov=True)
    cov, m, mu, thresh, w, groups, P, extra = calls[-1]
    rmean, rcov = (a.numpy() for a in ExceedOraclePlan.exceedance_moments(None, cov, m, mu, thresh, w, groups, P, extra))
    e = _check(torch.tensor(ds["mean"].values), torch.tensor(pcov), rmean, rcov, np.asarray(w), np.asarray(groups), P, "loadest")
    print(f"loadest exceedance: mean error / W = {e[0]:.3e}, cov error / (W_g W_h) = {e[1]:.3e}")
    assert np.allclose(ds["se"].values, np.sqrt(np.diagonal(pcov, axis1=1, axis2=2)))
    omu, ocov = _oracle_posterior(model, daily)
    _o, og, labels, n_pts, _d = period_groups(daily.coords["time"].values, np.ones(len(omu)), "YE")
    u = np.broadcast_to(((np.log(tau) - t) / s)[:, None], (2, len(omu)))
    omean, oc = dense_exceedance_moments(ocov, omu, u, np.ones(len(omu)), og, len(labels))
    n = n_pts.astype(np.float64)
    print("loadest vs oracle posterior:", float(np.abs(ds["mean"].values - omean).max()), float(np.abs(pcov - oc).max()))
    assert np.all(np.abs(ds["mean"].values - omean) <= 1e-8 * n[None, :])
    assert np.all(np.abs(pcov - oc) <= 1e-8 * (n[:, None] * n[None, :])[None])

    cov_obs, target, unc, daily = daily_rating(n_obs=150, seed=12)
    rating = RatingGP()
    rating.fit(cov_obs, target, target_unc=unc, iterations=10)
    calls = _record(rating)
    levels = np.quantile(target.values, [0.1, 0.3, 0.5, 0.7, 0.9])
    dc = rating.duration_curve(daily, levels=levels)
    cov, m, mu, thresh, w, groups, P, extra = calls[-1]
    assert P == 1 and m == len(daily.coords["time"].values)
    rmean, rcov = (a.numpy() for a in ExceedOraclePlan.exceedance_moments(None, cov, m, mu, thresh, w, groups, P, extra))
    f, se = dc["mean"].values, dc["se"].values
    assert np.all(np.abs(f * m - rmean[:, 0]) <= 1e-13 * m) and np.all(np.abs((se * m) ** 2 - rcov[:, 0, 0]) <= 1e-11 * m * m)
    print("rating duration curve:", float(np.abs(f - rmean[:, 0] / m).max()), float(np.abs(se ** 2 - rcov[:, 0, 0] / m ** 2).max()))
    assert np.all(np.diff(f) <= 0) and np.all((f >= 0) & (f <= 1))
    _mode, s, t = target_transform(rating.dm)
    omu, ocov = _oracle_posterior(rating, daily)
    u = np.broadcast_to(((np.log(levels) - t) / s)[:, None], (len(levels), m))
    omean, oc = dense_exceedance_moments(ocov, omu, u, np.ones(m), np.zeros(m, dtype=np.int32), 1)
    print("rating vs oracle posterior:", float(np.abs(f - omean[:, 0] / m).max()), float(np.abs(se ** 2 - oc[:, 0, 0] / m ** 2).max()))
    assert np.all(np.abs(f * m - omean[:, 0]) <= 1e-8 * m) and np.all(np.abs((se * m) ** 2 - oc[:, 0, 0]) <= 1e-8 * m * m)
    # the default: 21 levels from the posterior mean
    dc = rating.duration_curve(daily)
    cov, m, mu, thresh, w, groups, P, extra = calls[-1]
    assert tuple(thresh.shape) == (21, m) and dc["mean"].values.shape == (21,)
    rmean, rcov = (a.numpy() for a in ExceedOraclePlan.exceedance_moments(None, cov, m, mu, thresh, w, groups, P, extra))
    f, se = dc["mean"].values, dc["se"].values
    print("rating default duration curve:", float(np.abs(f - rmean[:, 0] / m).max()), float(np.abs(se ** 2 - rcov[:, 0, 0] / m ** 2).max()))
    assert np.all(np.abs(f * m - rmean[:, 0]) <= 1e-13 * m) and np.all(np.abs((se * m) ** 2 - rcov[:, 0, 0]) <= 1e-11 * m * m)
    assert np.all(np.diff(f) <= 0) and f[0] > 0.9 and f[-1] < 0.1
