"""GPU parity of ``dgp_posterior_excess_moments`` -- the excess / deficit moments with the posterior covariance produced a panel
of rows at a time from the held factorisation -- and of ``streamed=True`` in the API above it.

1. Against the dense device path on the same plan (``posterior_cov`` + ``excess_moments``), float64, with that path's own bounds
   (tests/test_gpu_excess.py, Q from ``excess_scales``): a mean entry 1e-13 Q_g, a covariance entry 1e-11 Q_g Q_h, ``total``
   1e-13 of its value.  The panels hold ``posterior_cov``'s entries; the sums over j are grouped by panel, and sigma_i^2 is the
   predicted variance instead of the buffer's diagonal (another summation order of the same products).
2. Both device paths against ``dense_excess_moments`` on the ORACLE's posterior covariance: no fixed number; the streamed path
   may err 4 x what the dense device path errs on the same cases (both inherit ``posterior_cov``'s error through rho).
3. float32 plans against the float64 dense device path: the streamed error at most 2 x the dense float32 path's.
4. Ragged batches of 3 and 12 sites against single-site plans, 1e-11 scaled, and bitwise independence of the batch companions.
5. Work areas and the held fit: NaN / 1e30 in the work area, repeated calls, the size formula, a work area one byte short, a bad
   ``panel_rows`` / ``above``, no factorisation, A / T / K^^-1 / alpha and ``predict`` afterwards.
6. NaN in -> NaN out in the dense path's entries.
7. ``RatingGP.excess`` / ``LoadestGP.excess_load`` with ``streamed=True`` against the default path, and under a byte budget the
   dense path refuses.

The margins 4 x and 2 x are those of tests/test_gpu_exceedance_stream.py.  As there, the thresholds of the point whose variance
is zero to rounding sit one unit from its mean (a tie would depend on the sign of a rounding error the two variance computations
do not share), and a variance that is negative on both paths comes from a negative ``extra_var``.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from discontinuum_amd.backend import GPPlan, _ptr, _stream
from discontinuum_amd.excess import excess_intervals
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.loads import flux_weights
from discontinuum_amd.rating_gp import RatingGP
from oracle import gp_oracle as orc
from tests.excess_helpers import dense_excess_moments, excess_scales
from tests.excess_stream_helpers import excess_stream_bytes
from tests.flux_helpers import daily_loadest, daily_rating
from tests.test_gpu_exceedance_stream import MODELS, _grouping, _held, _points
from tests.test_gpu_excess import S, T, _close
from tests.test_gpu_influence import _ragged
from tests.test_gpu_stages import make_case

pytestmark = pytest.mark.gpu


def _dense(plan, theta, xs, m, mapped, s2, a, w, g, P, above, ev):
    kmean, cov = plan.posterior_cov(theta, xs)
    return plan.excess_moments(cov, m, mapped, s2, a, w, g, P, above=above, extra_var=ev)


def _host(ts):
    return tuple(t.cpu().numpy() for t in ts)


def _scales(var, mapped, s2, a, w, g, P, ev=None):
    """``excess_scales`` reads the covariance's diagonal alone: Q (L, P) from the latent variances ``var`` (m,)."""
    return excess_scales(np.diag(np.asarray(var, np.float64)), mapped, s2, a, w, g, P, ev)


def _check(got, ref, Q, tag):
    """The excess product's bounds with ``ref`` as the reference -> (worst mean error / Q_g, worst cov error / (Q_g Q_h))."""
    e0 = _close(got[0], ref[0], 1e-13 * Q, tag + ("mean",))
    e1 = _close(got[1], ref[1], 1e-11 * Q[:, :, None] * Q[:, None, :], tag + ("cov",))
    _close(got[2], ref[2], 1e-13 * np.abs(ref[2]), tag + ("total",))
    return e0 * 1e-13, e1 * 1e-11


def _scaled(got, ref, Q):
    """(max |mean - ref| / Q_g, max |cov - ref| / (Q_g Q_h)) over the groups with Q > 0; everything finite."""
    Qs = np.where(Q > 0, Q, np.inf)
    assert all(np.isfinite(x).all() for x in got[:2]) and all(np.isfinite(x).all() for x in ref[:2])
    return (float(np.max(np.abs(got[0] - ref[0]) / Qs)), float(np.max(np.abs(got[1] - ref[1]) / (Qs[:, :, None] * Qs[:, None, :]))))


# ------------------------------------------------------------------------------------------------ 1. the dense device path
@pytest.mark.parametrize("n", [1, 129, 300])
@pytest.mark.parametrize("name", MODELS)
def test_streamed_moments_match_the_dense_device_path(name, n, gpu_device):
    """m in {1, 2, 127, 129, 300, 700} x panels of 128 / 256 / 768 rows x both signs; P in {1, 3, 40}, L in {1, 2, 3, 9} (9: two
    level groups, 8 + 1; 3: a 2-level and a 1-level launch in one group), ``extra_var`` on and off, the ``gap`` and ``aligned``
    groupings, a = +-inf, a point on a nearly noise-free training row and a negative total variance.  Measured on MI355X, worst
    mean error / Q_g and covariance error / (Q_g Q_h): loadest 3.7e-16 / 6.6e-16, rating 1.3e-15 / 2.9e-16, composite 5.2e-16 /
    1.0e-15 (bounds 1e-13 and 1e-11)."""
    dev = gpu_device
    quiet = 5 if n >= 129 else None
    plan, _model, d, X, _r, _noise, theta = _held(name, n, dev, quiet_point=quiet)
    rng = np.random.default_rng(11)
    worst = [0.0, 0.0]
    for m in (1, 2, 127, 129, 300, 700):
        Xs = _points(name, d, m, seed=3 + m)
        if quiet is not None and m >= 127:
            Xs[40] = X[quiet]  # a test point ON the nearly noise-free training point: variance zero to rounding
        xs = Xs.to(dev).contiguous()
        kmean, var = plan.predict(theta, xs)
        mapped_t = (S * kmean + T).contiguous()
        mapped, varh = mapped_t.cpu().numpy(), var.cpu().numpy()
        sd = S * np.sqrt(np.clip(varh, 1e-300, None))
        w = rng.uniform(0.5, 2.0, m)
        evh = rng.uniform(0.0, 0.05, m)
        if m >= 127:
            evh[41] = -10.0  # sigma^2 < 0 on both paths: decided
        ev_t = torch.tensor(evh, device=dev)
        combos = [(1, 1, "plain"), (3, 2, "plain"), (40, 3, "plain")]
        if m >= 300:
            combos += [(3, 9, "plain"), (40, 2, "plain"), (3, 3, "aligned")]
        if m == 700:
            combos += [(3, 9, "gap"), (1, 2, "gap")]
        for k, (P, L, kind) in enumerate(combos):
            g = _grouping(m, P, kind)
            a = mapped[None, :] + sd[None, :] * rng.normal(0.0, 1.2, (L, m))
            if m >= 127:
                a[0, 7], a[0, 90], a[L - 1, 100] = np.inf, -np.inf, np.inf
                a[:, 40] = mapped[40] + np.where(np.arange(L) % 2 == 0, 1.0, -1.0)
                a[:, 41] = mapped[41] + np.where(np.arange(L) % 2 == 0, -0.5, 0.5)
                if L >= 9:  # (a level of the second group)
                    a[8, 60], a[8, 61] = -np.inf, np.inf
            ev = ev_t if k % 2 else None
            Q = _scales(varh, mapped, S * S, a, w, g, P, evh if k % 2 else None)
            at, wt, gt = torch.tensor(a), torch.tensor(w), torch.tensor(g)
            for above in (True, False):
                ref = _host(_dense(plan, theta, xs, m, mapped_t, S * S, at, wt, gt, P, above, ev))
                for R in (128, 256, 768):
                    got = plan.posterior_excess_moments(theta, xs, mapped_t, S * S, at, wt, gt, P, above=above, extra_var=ev,
                                                        panel_rows=R)
                    assert got[0].shape == (L, P) and got[1].shape == (L, P, P) and got[2].shape == (P,)
                    assert torch.equal(got[1], got[1].transpose(-1, -2)) or torch.isnan(got[1]).any()
                    e = _check(_host(got), ref, Q, (name, n, m, P, L, kind, above, ev is not None, R))
                    worst = [max(x, y) for x, y in zip(worst, e)]
    print(f"{name} n={n}: worst streamed - dense: mean = {worst[0]:.3e} Q_g, cov = {worst[1]:.3e} Q_g Q_h")


# ------------------------------------------------------------------------------------------------ 6. NaN in -> NaN out
def test_nan_in_gives_nan_out_like_the_dense_path(gpu_device):
    dev, m, P, L = gpu_device, 300, 3, 3
    plan, _model, d, _X, _r, _noise, theta = _held("loadest", 129, dev)
    xs = _points("loadest", d, m, seed=1).to(dev).contiguous()
    kmean, var = plan.predict(theta, xs)
    mapped = (S * kmean + T).contiguous()
    mapped[10] = float("nan")
    g = torch.tensor(_grouping(m, P, "plain"))
    a = (S * kmean[None, :] + T + S * var.sqrt()[None, :] * torch.randn(L, m, dtype=torch.float64, device=dev)).contiguous()
    a[1, 200] = float("nan")
    w = torch.ones(m, dtype=torch.float64)
    for above in (True, False):
        dmean, dcov, dtotal = _dense(plan, theta, xs, m, mapped, S * S, a, w, g, P, above, None)
        smean, scov, stotal = plan.posterior_excess_moments(theta, xs, mapped, S * S, a, w, g, P, above=above, panel_rows=128)
        assert torch.isnan(dmean[:, int(g[10])]).all() and torch.equal(torch.isnan(smean), torch.isnan(dmean))
        assert torch.equal(torch.isnan(scov), torch.isnan(dcov)) and torch.isnan(scov).any() and not torch.isnan(scov).all()
        assert torch.equal(torch.isnan(stotal), torch.isnan(dtotal)) and torch.isnan(stotal).sum() == 1


# ------------------------------------------------------------------------------------------------ 2. the oracle's posterior
@pytest.mark.parametrize("name", MODELS)
def test_streamed_error_against_the_oracle_is_the_dense_paths(name, gpu_device):
    """Both device paths against ``dense_excess_moments`` on the oracle's posterior covariance and variances (mapped mean of the
    device): the streamed path's worst scaled error is allowed 4 x the dense path's.  Measured on MI355X, dense / streamed: means
    6.5e-17 / 6.4e-17 (loadest), 9.8e-17 / 9.8e-17 (rating), 6.6e-17 / 9.8e-17 (composite); covariances 5.3e-18 / 5.3e-18,
    5.3e-18 / 7.7e-18, 4.6e-18 / 7.9e-18."""
    dev, n = gpu_device, 300
    plan, model, d, X, r, noise, theta = _held(name, n, dev)
    rng = np.random.default_rng(21)
    ed, es = [0.0, 0.0], [0.0, 0.0]
    for m, P, L, R, above in ((129, 3, 3, 128, True), (300, 3, 9, 128, False), (300, 1, 1, 256, True)):
        Xs = _points(name, d, m, seed=7 + m)
        xs = Xs.to(dev).contiguous()
        _omu, ocov = orc.posterior(model, X, r, noise, theta, Xs, full_cov=True)
        Co = ocov.numpy()
        Co = 0.5 * (Co + Co.T)
        kmean, _var = plan.predict(theta, xs)
        mapped_t = (S * kmean + T).contiguous()
        mapped = mapped_t.cpu().numpy()
        w, g = rng.uniform(0.5, 2.0, m), _grouping(m, P, "plain")
        ev = rng.uniform(0.0, 0.05, m)
        a = mapped[None, :] + S * np.sqrt(np.diagonal(Co) + ev)[None, :] * rng.normal(0.0, 1.2, (L, m))
        ref = dense_excess_moments(Co, mapped, S * S, a, w, g, P, above, ev)
        Q = excess_scales(Co, mapped, S * S, a, w, g, P, ev)
        args = (mapped_t, S * S, torch.tensor(a), torch.tensor(w), torch.tensor(g), P)
        evt = torch.tensor(ev, device=dev)
        dense = _host(_dense(plan, theta, xs, m, *args, above, evt))
        streamed = _host(plan.posterior_excess_moments(theta, xs, *args, above=above, extra_var=evt, panel_rows=R))
        ed = [max(x, y) for x, y in zip(ed, _scaled(dense, ref, Q))]
        es = [max(x, y) for x, y in zip(es, _scaled(streamed, ref, Q))]
    print(f"{name} vs oracle posterior: dense mean {ed[0]:.3e} cov {ed[1]:.3e}; streamed mean {es[0]:.3e} cov {es[1]:.3e}")
    assert es[0] <= 4 * ed[0] and es[1] <= 4 * ed[1], (ed, es)


# ------------------------------------------------------------------------------------------------ 3. float32 plans
@pytest.mark.parametrize("name", ["loadest", "rating"])
def test_float32_streamed_error_is_the_dense_float32_paths(name, gpu_device):
    """float32 plans, n = 300, m = 300 and 700, against the float64 dense device path on the same inputs: the streamed float32
    error at most 2 x the dense float32 error.  Measured on MI355X, dense / streamed: means 5.3e-8 / 3.5e-8 (loadest), 5.5e-7 /
    3.1e-7 (rating); covariances 3.0e-8 / 2.7e-8, 4.7e-8 / 4.2e-8."""
    dev, n = gpu_device, 300
    p64, _model, d, _X, _r, _noise, theta = _held(name, n, dev)
    p32 = _held(name, n, dev, dtype=torch.float32)[0]
    rng = np.random.default_rng(31)
    ed, es = [0.0, 0.0], [0.0, 0.0]
    for m, P, L, R, above in ((300, 3, 3, 128, True), (700, 3, 2, 256, False), (700, 40, 1, 128, True)):
        Xs = _points(name, d, m, seed=9 + m)
        x64, x32 = Xs.to(dev).contiguous(), Xs.to(dev, torch.float32).contiguous()
        kmean, var = p64.predict(theta, x64)
        mu32 = (S * kmean + T).float().contiguous()
        mu64 = mu32.double()  # the same mapped mean on every path
        mapped, varh = mu64.cpu().numpy(), var.cpu().numpy()
        w, g = rng.uniform(0.5, 2.0, m), _grouping(m, P, "plain")
        ev = rng.uniform(0.01, 0.05, m).astype(np.float32).astype(np.float64)  # (exact in both dtypes)
        a = torch.tensor(mapped[None, :] + S * np.sqrt(varh + ev)[None, :] * rng.normal(0.0, 1.2, (L, m)))
        wt, gt = torch.tensor(w), torch.tensor(g)
        Q = _scales(varh, mapped, S * S, a.numpy(), w, g, P, ev)
        ref = _host(_dense(p64, theta, x64, m, mu64, S * S, a, wt, gt, P, above, torch.tensor(ev, device=dev)))
        ev32 = torch.tensor(ev, device=dev, dtype=torch.float32)
        dense = _host(_dense(p32, theta, x32, m, mu32, S * S, a, wt, gt, P, above, ev32))
        streamed = _host(p32.posterior_excess_moments(theta, x32, mu32, S * S, a, wt, gt, P, above=above, extra_var=ev32, panel_rows=R))
        ed = [max(x, y) for x, y in zip(ed, _scaled(dense, ref, Q))]
        es = [max(x, y) for x, y in zip(es, _scaled(streamed, ref, Q))]
    print(f"{name} float32 vs float64 dense: dense mean {ed[0]:.3e} cov {ed[1]:.3e}; streamed mean {es[0]:.3e} cov {es[1]:.3e}")
    assert es[0] <= 2 * ed[0] and es[1] <= 2 * ed[1], (ed, es)


# ------------------------------------------------------------------------------------------------ 4. ragged batches
@pytest.mark.parametrize("model,d,sizes", [("loadest", 3, [300, 129, 257]),
                                           ("rating", 2, [129, 64, 200, 1, 2, 127, 128, 130, 77, 150, 199, 33])])
def test_ragged_batches_match_single_site_plans(model, d, sizes, gpu_device):
    dev, m, P, L, B = gpu_device, 300, 3, 3, len(sizes)
    pb, cases, theta, Xs = _ragged(model, d, sizes, m, dev, seed0=80)
    assert not torch.equal(theta[0], theta[1])
    xs = Xs.to(dev).contiguous()
    rng = np.random.default_rng(41)
    kmean, var = pb.predict(theta, xs)
    mapped = (S * kmean + T).contiguous()
    a = mapped[:, None, :] + S * var.sqrt()[:, None, :] * torch.tensor(rng.normal(0.0, 1.2, (B, L, m)), device=dev)
    w = torch.tensor(rng.uniform(0.5, 2.0, (B, m)))
    gh = _grouping(m, P, "plain")
    g = torch.tensor(np.stack([gh] * B))
    ev = torch.tensor(rng.uniform(0.0, 0.05, (B, m)), device=dev)
    s2 = [S * S * (1.0 + 0.05 * b) for b in range(B)]
    for above in (True, False):
        first = pb.posterior_excess_moments(theta, xs, mapped, s2, a, w, g, P, above=above, extra_var=ev, panel_rows=128)
        again = pb.posterior_excess_moments(theta, xs, mapped, s2, a, w, g, P, above=above, extra_var=ev, panel_rows=128)
        assert all(torch.equal(x, y) for x, y in zip(first, again))
        assert first[0].shape == (B, L, P) and first[1].shape == (B, L, P, P) and first[2].shape == (B, P)
        worst = [0.0, 0.0]
        for b, (nb, c) in enumerate(zip(sizes, cases)):
            p1 = GPPlan(model, nb, d, device=dev)
            p1.set_inputs(c[0].to(dev).contiguous())
            p1.factorize(c[3], c[1].to(dev).contiguous(), c[2].to(dev).contiguous())
            one = p1.posterior_excess_moments(c[3], xs[b], mapped[b], s2[b], a[b], w[b], g[b], P, above=above, extra_var=ev[b],
                                              panel_rows=128)
            Q = _scales(var[b].cpu().numpy(), mapped[b].cpu().numpy(), s2[b], a[b].cpu().numpy(), w[b].numpy(), gh, P, ev[b].cpu().numpy())
            e = _scaled(_host(tuple(t[b] for t in first)), _host(one), Q)
            worst = [max(x, y) for x, y in zip(worst, e)]
            assert float(((first[2][b] - one[2]).abs() / one[2].abs().clamp_min(1e-300)).max()) <= 1e-11
        print(f"{model} ragged batch of {B} above={above}: worst scaled difference to the single-site plans mean {worst[0]:.2e} "
              f"cov {worst[1]:.2e}")
        assert max(worst) <= 1e-11, worst


def test_a_sites_numbers_do_not_depend_on_its_batch_companions(gpu_device):
    """The sites of a ragged batch of three, then the same sites in another order with other thresholds for the companions: the
    site that kept its inputs keeps its bits."""
    dev, model, d, sizes, m, P, L = gpu_device, "loadest", 3, [300, 129, 257], 300, 3, 3
    pb, cases, theta, Xs = _ragged(model, d, sizes, m, dev, seed0=80)
    xs = Xs.to(dev).contiguous()
    rng = np.random.default_rng(43)
    kmean, var = pb.predict(theta, xs)
    mapped = (S * kmean + T).contiguous()
    a = mapped[:, None, :] + S * var.sqrt()[:, None, :] * torch.tensor(rng.normal(0.0, 1.2, (3, L, m)), device=dev)
    w = torch.tensor(rng.uniform(0.5, 2.0, (3, m)))
    g = torch.tensor(np.stack([_grouping(m, P, "plain")] * 3))
    s2 = [S * S, 0.9 * S * S, 1.1 * S * S]
    first = pb.posterior_excess_moments(theta, xs, mapped, s2, a, w, g, P, panel_rows=128)
    a2, w2, mapped2 = a.clone(), w.clone(), mapped.clone()
    a2[1:] += 0.3  # the companions of site 0 change
    w2[1:] *= 2.0
    mapped2[2, 7] = float("nan")
    second = pb.posterior_excess_moments(theta, xs, mapped2, [s2[0], 0.5, 2.0], a2, w2, g, P, panel_rows=128)
    assert all(torch.equal(x[0], y[0]) for x, y in zip(first, second))
    assert not torch.equal(first[0][1], second[0][1]) and torch.isnan(second[0][2]).any()


# ------------------------------------------------------------------------------------------------ 5. work areas, the held fit
def test_work_area_contents_do_not_matter_and_the_held_fit_survives(gpu_device):
    dev, name, n, m, P, L = gpu_device, "rating", 300, 700, 3, 9
    X, r, noise, theta = make_case(name, 2, n, seed=4, perturb=0.2)
    p = GPPlan(name, n, 2, device=dev)
    p.set_inputs(X.to(dev).contiguous())
    out, _dr, _dn = p.fit_step(theta, r.to(dev), noise.to(dev))
    assert int(out[_lib.OUT_INFO]) == 0
    xs = _points(name, 2, m, seed=2).to(dev).contiguous()
    bufs = (_lib.BUF_A, _lib.BUF_T, _lib.BUF_S, _lib.BUF_ALPHA, _lib.BUF_XT)
    before = [p.buffer(b).clone() for b in bufs] + list(p.predict(theta, xs))
    kmean, var = before[-2], before[-1]
    mapped = (S * kmean + T).contiguous()
    rng = np.random.default_rng(51)
    gh = _grouping(m, P, "gap")  # whole 128- and 256-row panels of excluded points inside group 1's column range
    assert np.all(gh[256:512] == -1) and gh[199] == 1 and gh[520] == 1
    g = torch.tensor(gh)
    a = (mapped[None, :] + S * var.sqrt()[None, :] * torch.tensor(rng.normal(0.0, 1.2, (L, m)), device=dev)).contiguous()
    w = torch.tensor(rng.uniform(0.5, 2.0, m))
    args = (theta, xs, mapped, S * S, a, w, g, P)
    Q = _scales(var.cpu().numpy(), mapped.cpu().numpy(), S * S, a.cpu().numpy(), w.numpy(), gh, P)
    ref = _host(_dense(p, theta, xs, m, mapped, S * S, a, w, g, P, True, None))
    same = lambda x, y: all(torch.equal(u, v) for u, v in zip(x, y))  # noqa: E731
    for R in (128, 256):
        first = p.posterior_excess_moments(*args, panel_rows=R)
        assert all(torch.isfinite(t).all() for t in first)
        ws = p._pxs_ws[: p._pxs_ws.numel() // 8 * 8].view(torch.float64)
        half = ws.numel() // 2
        ws[:half] = float("nan")
        ws[half:] = 1e30
        dirty = p.posterior_excess_moments(*args, panel_rows=R)
        _check(_host(dirty), ref, Q, ("NaN work area", R))
        ws[:half] = 1e30
        ws[half:] = float("nan")
        other_half = p.posterior_excess_moments(*args, panel_rows=R)
        assert same(first, other_half), R
        ws.zero_()
        clean = p.posterior_excess_moments(*args, panel_rows=R)
        for other in (dirty, clean, p.posterior_excess_moments(*args, panel_rows=R)):
            assert same(first, other), R
        assert torch.equal(first[1], first[1].transpose(-1, -2))
    after = [p.buffer(b) for b in bufs] + list(p.predict(theta, xs))
    for k, (x, y) in enumerate(zip(before, after)):
        # bit for bit: the blocks of A / T / K^^-1 above the block diagonal are undefined and may hold a stale NaN
        assert torch.equal(x.reshape(-1).view(torch.int64), y.reshape(-1).view(torch.int64)), (k, int((x != y).sum()))
    # the C entry: the documented size, one byte short, a misaligned work area, a bad panel_rows and a bad above
    lib = p.lib
    need = int(lib.dgp_posterior_excess_moments_workspace_bytes(p._h, m, P, L, 128))
    assert need == excess_stream_bytes(n, m, 2, P, L, 8, 128)
    assert int(lib.dgp_posterior_excess_moments_workspace_bytes(p._h, m, P, L, 256)) == excess_stream_bytes(n, m, 2, P, L, 8, 256)
    assert int(lib.dgp_posterior_excess_moments_workspace_bytes(p._h, m, 40, 3, 768)) == excess_stream_bytes(n, m, 2, 40, 3, 8, 768)
    work = torch.empty(need + 512, dtype=torch.uint8, device=dev)
    base = work.data_ptr() + (-work.data_ptr()) % 256
    th = (C.c_double * theta.numel())(*theta.tolist())
    mean_out = torch.empty(L, P, dtype=torch.float64, device=dev)
    cov_out = torch.empty(L, P, P, dtype=torch.float64, device=dev)
    total_out = torch.empty(P, dtype=torch.float64, device=dev)
    wd, gd, s2 = w.to(dev), g.to(dev), torch.tensor([S * S], dtype=torch.float64, device=dev)

    def call(ptr, nbytes, rows=128, above=1):
        return lib.dgp_posterior_excess_moments(p._h, th, _ptr(xs), m, _ptr(mapped), _ptr(s2), _ptr(a), L, _ptr(wd), _ptr(gd), P, None,
                                                above, rows, C.c_void_p(ptr), nbytes, _ptr(mean_out), _ptr(cov_out), _ptr(total_out),
                                                _stream())

    assert call(base, need - 1) == -3 and b"workspace" in lib.dgp_last_error()
    assert call(base + 8, need) == -1 and b"aligned" in lib.dgp_last_error()
    for rows in (0, 64, 200):
        assert call(base, need, rows=rows) == -1 and b"panel_rows" in lib.dgp_last_error()
    for above in (-1, 2):
        assert call(base, need, above=above) == -1 and b"above" in lib.dgp_last_error()
    assert call(base, need) == 0
    torch.cuda.synchronize(dev)
    first = p.posterior_excess_moments(*args, panel_rows=128)
    assert same((mean_out, cov_out, total_out), first)
    with pytest.raises(ValueError, match="multiple of 128"):
        p.posterior_excess_moments(*args, panel_rows=100)
    # no factorisation: DGP_E_STATE
    q = GPPlan(name, n, 2, device=dev)
    q.set_inputs(X.to(dev).contiguous())
    with pytest.raises(_lib.DGPError, match="factorisation"):
        q.posterior_excess_moments(*args, panel_rows=128)


# ------------------------------------------------------------------------------------------------ 7. the engines
def _record(model):
    """Make the model's plan keep the arguments of its ``excess_moments`` calls (the dense path's)."""
    calls, real = [], model._plan.excess_moments

    def spy(cov, m, mu, scale2, thresh, w, groups, ngroups, above=True, extra_var=None):
        calls.append((torch.diagonal(cov)[:m].double().cpu().numpy(), mu.double().cpu().numpy(), float(scale2),
                      torch.as_tensor(thresh).cpu().numpy(), np.asarray(w, np.float64), np.asarray(groups), ngroups))
        return real(cov, m, mu, scale2, thresh, w, groups, ngroups, above=above, extra_var=extra_var)

    model._plan.excess_moments = spy
    return calls


def _dataset_close(got, gcov, ref, rcov, Q, ci, tag):
    """Test 1's bounds on the Dataset: ``mean`` 1e-13 Q_g, the covariance 1e-11 Q_g Q_h, ``total`` 1e-13 of its value, and what
    they imply for the derived fields: share = mean / total moves by at most (1e-13 Q_g + 1e-13 mean) / total <= 2e-13 Q_g / total;
    se = sqrt(var) by dvar / (se + se') <= 1e-11 Q_g^2 / se; ``lower`` / ``upper`` = q(mean, var) by
    |dq/dmean| 1e-13 Q_g + |dq/dvar| 1e-11 Q_g^2 to first order (central differences of ``excess_intervals``), doubled for the
    higher orders, plus 1e-12 q for the quantile function's own accuracy."""
    mean, total = ref["mean"].values, ref["total"].values
    var = np.diagonal(rcov, axis1=1, axis2=2)
    dm, dv = 1e-13 * Q, 1e-11 * Q * Q
    _close(got["mean"].values, mean, dm, tag + ("mean",))
    _close(gcov, rcov, 1e-11 * Q[:, :, None] * Q[:, None, :], tag + ("cov",))
    _close(got["total"].values, total, 1e-13 * total, tag + ("total",))
    _close(got["share"].values, ref["share"].values, 2e-13 * Q / total[None, :], tag + ("share",))
    _close(got["se"].values, ref["se"].values, dv / ref["se"].values, tag + ("se",))
    hm, hv = 1e-6 * mean, 1e-6 * var
    qm = [(a - b) / (2 * hm) for a, b in zip(excess_intervals(mean + hm, var, ci), excess_intervals(mean - hm, var, ci))]
    qv = [(a - b) / (2 * hv) for a, b in zip(excess_intervals(mean, var + hv, ci), excess_intervals(mean, var - hv, ci))]
    for k, name in enumerate(("lower", "upper")):
        bound = 2 * (np.abs(qm[k]) * dm + np.abs(qv[k]) * dv) + 1e-12 * np.abs(ref[name].values)
        _close(got[name].values, ref[name].values, bound, tag + (name,))
    assert np.array_equal(got["n_points"].values, ref["n_points"].values)


def test_engines_streamed_against_the_default_path_and_under_a_small_budget(gpu_device):
    budget = 8_000_000
    cov_obs, target, unc, daily = daily_rating(n_obs=150, seed=12)
    rating = RatingGP()
    rating.fit(cov_obs, target, target_unc=unc, iterations=10)
    m = len(daily.coords["time"].values)
    seconds = np.full(m, 86400.0)
    low = [float(np.quantile(target.values, q)) for q in (0.3, 0.5, 0.7)]
    kw = dict(threshold=low, weights=seconds, above=False, return_cov=True)
    calls = _record(rating)
    dense, dcov = rating.excess(daily, **kw)
    diag, mu, s2, a, w, g, P = calls[-1]
    Q = _scales(diag, mu, s2, a, w, g, P)
    streamed, scov = rating.excess(daily, streamed=True, **kw)
    assert len(calls) == 1 and rating._plan.excess_panel_rows(m, P, 3) == -(-m // 128) * 128  # the default budget: one panel
    _dataset_close(streamed, scov, dense, dcov, Q, 0.95, ("rating deficit volume",))
    with pytest.raises(NotImplementedError, match="pass streamed=True"):
        rating.excess(daily, max_bytes=budget, **kw)
    small, smcov = rating.excess(daily, max_bytes=budget, streamed=True, **kw)
    R = rating._plan.excess_panel_rows(m, P, 3, max_bytes=budget)  # what the call above picked
    need = int(rating._plan.lib.dgp_posterior_excess_moments_workspace_bytes(rating._plan._h, m, P, 3, R))
    more = int(rating._plan.lib.dgp_posterior_excess_moments_workspace_bytes(rating._plan._h, m, P, 3, R + 128))
    assert 128 <= R < -(-m // 128) * 128 and need <= budget < more and len(calls) == 1
    print(f"rating deficit volume under {budget} bytes: panel rows {R}, work area {need} bytes")
    _dataset_close(small, smcov, dense, dcov, Q, 0.95, ("rating deficit volume, small budget",))
    with pytest.raises(ValueError, match=r"the streamed excess pass needs a work area of \d+ bytes"):
        rating.excess(daily, max_bytes=100_000, streamed=True, **kw)

    cov_obs, target, daily = daily_loadest(n_obs=200, seed=11)
    model = LoadestGP()
    model.fit(cov_obs, target, iterations=10)
    wf = flux_weights(daily, {"units": "mg/l"})
    limit = [0.8 * float(np.median(wf)), 1.1 * float(np.median(wf))]
    calls = _record(model)
    dense, dcov = model.excess_load(daily, limit=limit, return_cov=True)
    diag, mu, s2, a, w, g, P = calls[-1]
    Q = _scales(diag, mu, s2, a, w, g, P)
    streamed, scov = model.excess_load(daily, limit=limit, return_cov=True, streamed=True)
    _dataset_close(streamed, scov, dense, dcov, Q, 0.95, ("loadest excess_load",))
    with pytest.raises(NotImplementedError, match="pass streamed=True"):
        model.excess_load(daily, limit=limit, max_bytes=budget)
    small, smcov = model.excess_load(daily, limit=limit, return_cov=True, max_bytes=budget, streamed=True)
    md = len(daily.coords["time"].values)
    assert model._plan.excess_panel_rows(md, P, 2, max_bytes=budget) < -(-md // 128) * 128 and len(calls) == 1
    _dataset_close(small, smcov, dense, dcov, Q, 0.95, ("loadest excess_load, small budget",))
