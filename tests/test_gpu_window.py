"""GPU parity of ``dgp_window_moments`` (exact moments of rolling-window means) and of the API above it:
``MarginalHIP.rolling_mean`` and the ``window=`` keyword of ``exceedance`` / ``duration_curve``.

The kernel is checked against the formulas in plain numpy float64 with an explicit dense W
(tests/window_helpers.py::dense_window_moments) on the SAME ``dgp_posterior_cov`` buffer, symmetrised from its lower
triangle; float32 buffers against the same reference on the float32 values cast to double (outputs and accumulation are
double, so both dtypes share one bound).  Bounds: mode 0, 1e-12 of max |C| for the covariance and 1e-13 of max |mu| for the
mean -- each entry is a normalised double sum of at most w^2 terms, 2 w eps <= 2.3e-13 at w = 523; mode 1, 1e-11 of the
reference covariance's max-norm (a few ulp per exp / expm1 term on top of the sum).  Measured on MI355X: see DESIGN.md.
"""
import numpy as np
import pytest
import torch

from discontinuum_amd.backend import MODE_LINEAR, MODE_LOG, GPPlan, exceedance_moments, period_moments, window_moments
from oracle import gp_oracle as orc
from tests.exceedance_helpers import dense_exceedance_moments
from tests.flux_helpers import symmetrise_lower
from tests.window_helpers import dense_window_moments, ragged, trailing, window_cases

pytestmark = pytest.mark.gpu

SIZES = (1, 127, 130, 257, 523)
S2 = 0.7


def _buffers(dev, dtype, ms, n=160, d=2, seed=0):
    """[(M, M) dgp_posterior_cov buffer, (m,) latent mean] per entry of ``ms``, from one factorised loadest plan; the test
    points are sorted in time, so that neighbours are highly correlated."""
    X, y = orc.synth_loadest(n, d, seed=seed)
    X, y = torch.tensor(X), torch.tensor(y)
    theta = torch.full((orc.loadest_ntheta(d),), 0.6931471805599453, dtype=torch.float64)
    plan = GPPlan("loadest", n, d, dtype=dtype, device=dev)
    plan.set_inputs(X.to(dev, dtype).contiguous())
    plan.factorize(theta, (y - y.mean()).to(dev, dtype).contiguous(), torch.full((n,), 0.05, dtype=dtype, device=dev))
    g = torch.Generator().manual_seed(seed + 1)
    out = []
    for m in ms:
        Xs = torch.rand(m, d, generator=g, dtype=torch.float64) * 4 - 2
        Xs[:, 0] = torch.sort(Xs[:, 0]).values
        mean, cov = plan.posterior_cov(theta, Xs.to(dev, dtype).contiguous())
        out.append((cov, mean))
    return out


_CACHE = {}


def _shared(dev, dtype):
    """The buffers of ``SIZES`` and their float64 symmetric copies, computed once per dtype and left unchanged."""
    if dtype not in _CACHE:
        bufs = _buffers(dev, dtype, SIZES)
        _CACHE[dtype] = {m: (cov, mu, symmetrise_lower(cov[:m, :m].double()).cpu().numpy(), mu.double().cpu().numpy())
                         for m, (cov, mu) in zip(SIZES, bufs)}
    return _CACHE[dtype]


def _dev(a, dev):
    return None if a is None else torch.tensor(a, device=dev)


def _lower(S, q):
    return np.tril(S.cpu().numpy()[:q, :q])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_kernel_matches_the_dense_formula(dtype, gpu_device):
    dev = gpu_device
    worst = {0: [0.0, 0.0], 1: [0.0, 0.0]}
    for m, (cov, mu, C, mu_h) in _shared(dev, dtype).items():
        cmax, mumax = float(np.abs(C).max()), float(np.abs(mu_h).max())
        for name, (lo, hi, a) in window_cases(m).items():
            q = len(lo)
            for mode in (MODE_LINEAR, MODE_LOG):
                mean, S = window_moments(cov, m, mu, _dev(lo, dev), _dev(hi, dev), a=_dev(a, dev), mode=mode, scale2=S2)
                rmean, rS = dense_window_moments(C, mu_h, lo, hi, a, mode, S2)
                assert tuple(mean.shape) == (q,) and S.shape[0] == S.shape[1] == -(-q // 128) * 128
                if mode == MODE_LINEAR:
                    em = float(np.abs(mean.cpu().numpy() - rmean).max()) / (mumax if mumax > 0 else 1.0)
                    ec = float(np.abs(_lower(S, q) - np.tril(rS)).max()) / cmax
                    tol_m, tol_c = 1e-13, 1e-12
                else:
                    smax = float(np.abs(rS).max())
                    em = float(np.abs(mean.cpu().numpy() - rmean).max()) / max(float(np.abs(rmean).max()), 1e-300)
                    ec = float(np.abs(_lower(S, q) - np.tril(rS)).max()) / (smax if smax > 0 else 1.0)
                    tol_m, tol_c = 1e-13, 1e-11
                worst[mode] = [max(worst[mode][0], em), max(worst[mode][1], ec)]
                assert em <= tol_m, (m, name, mode, "mean", em)
                assert ec <= tol_c, (m, name, mode, "cov", ec)
                empty = (hi <= lo) | (np.array([(np.ones(m) if a is None else a)[l:h].sum() for l, h in zip(lo, hi)]) <= 0)
                if empty.any():  # mean 0, a zero row and column
                    Sl = _lower(S, q)
                    assert np.all(mean.cpu().numpy()[empty] == 0) and np.all(Sl[empty, :] == 0) and np.all(Sl[:, empty] == 0)
    print(f"{dtype}: mode 0 worst mean {worst[0][0]:.3e} cov {worst[0][1]:.3e}; mode 1 worst mean {worst[1][0]:.3e} cov {worst[1][1]:.3e}")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_unit_windows_return_the_input_bitwise(dtype, gpu_device):
    """w = 1 with unit weights: the lower triangle of the result is that of the input converted to double, the mean is mu --
    the symmetric read and the tile edges move every entry to its place."""
    dev = gpu_device
    for m, (cov, mu, _C, _mu_h) in _shared(dev, dtype).items():
        lo, hi = trailing(m, 1)
        mean, S = window_moments(cov, m, mu, _dev(lo, dev), _dev(hi, dev))
        assert torch.equal(mean, mu.double()), m
        assert torch.equal(torch.tril(S[:m, :m]), torch.tril(cov[:m, :m].double())), m


def test_one_window_is_a_period_sum(gpu_device):
    """One window [0, m) with weights a against ``dgp_period_moments`` with one group and weights a / sum a: 1e-13 relative,
    both modes (mode 0 with scale2 = 1: the period pass multiplies by it)."""
    dev = gpu_device
    rng = np.random.default_rng(3)
    for m, (cov, mu, _C, _mu_h) in _shared(dev, torch.float64).items():
        a = rng.uniform(0.2, 3.0, m)
        if m > 4:
            a[[1, m // 2]] = 0.0
        lo, hi = np.zeros(1, np.int32), np.full(1, m, np.int32)
        g = torch.zeros(m, dtype=torch.int32, device=dev)
        for mode, s2 in ((MODE_LINEAR, 1.0), (MODE_LOG, S2)):
            mean, S = window_moments(cov, m, mu, _dev(lo, dev), _dev(hi, dev), a=_dev(a, dev), mode=mode, scale2=s2)
            pmean, pcov = period_moments(cov, m, mu, s2, torch.tensor(a / a.sum(), device=dev), g, 1, mode)
            assert abs(float(mean[0]) - float(pmean[0])) <= 1e-13 * abs(float(pmean[0])), (m, mode)
            assert abs(float(S[0, 0]) - float(pcov[0, 0])) <= 1e-13 * abs(float(pcov[0, 0])), (m, mode)


def test_structure_repeatable_symmetric_padded_batch_independent(gpu_device):
    dev = gpu_device
    m = 257
    bufs = _buffers(dev, torch.float64, (m, m, m), seed=3)
    cases = window_cases(m)
    picks = [cases["w30"], cases["ragged"], cases["weights"]]
    a3 = np.stack([np.ones(m) if a is None else a for _lo, _hi, a in picks])
    lo3, hi3 = np.stack([p[0] for p in picks]), np.stack([p[1] for p in picks])
    cov3 = torch.stack([b[0] for b in bufs]).contiguous()
    mu3 = torch.stack([b[1] for b in bufs]).contiguous()
    for mode in (MODE_LINEAR, MODE_LOG):
        s2 = torch.tensor([0.7, 0.5, 0.9], dtype=torch.float64)
        args = (cov3, m, mu3, _dev(lo3, dev), _dev(hi3, dev))
        mean_a, S_a = window_moments(*args, a=_dev(a3, dev), mode=mode, scale2=s2)
        mean_b, S_b = window_moments(*args, a=_dev(a3, dev), mode=mode, scale2=s2)
        assert torch.equal(mean_a, mean_b) and torch.equal(S_a, S_b)
        Q = S_a.shape[-1]
        assert Q == 384
        for b in range(3):
            mean1, S1 = window_moments(bufs[b][0], m, bufs[b][1], _dev(lo3[b], dev), _dev(hi3[b], dev), a=_dev(a3[b], dev), mode=mode,
                                       scale2=float(s2[b]))
            assert torch.equal(mean_a[b], mean1) and torch.equal(S_a[b], S1), (mode, b)
            for k in range(Q // 128):  # the diagonal 128-blocks are exactly symmetric
                blk = S1[k * 128:(k + 1) * 128, k * 128:(k + 1) * 128]
                assert torch.equal(blk, blk.T), (mode, b, k)
            low = torch.tril(S1)
            assert torch.equal(low[m:, :], torch.eye(Q, dtype=torch.float64, device=dev)[m:, :]), (mode, b)  # the pad is the identity


def test_windowed_covariance_feeds_the_exceedance_pass(gpu_device):
    """``exceedance_moments`` on the windowed covariance at m = 523 against the dense exceedance reference on the reference
    windowed covariance, inside the bounds of tests/test_gpu_exceedance.py (mean 1e-13 W_g, covariance 1e-11 W_g W_h).
    Neighbouring windows are correlated at rho -> 1: the pair function's expansion branch carries the sums."""
    dev = gpu_device
    m = 523
    cov, mu, C, mu_h = _shared(dev, torch.float64)[m]
    rng = np.random.default_rng(9)
    for name, (lo, hi) in (("w30", trailing(m, 30)), ("ragged", ragged(m))):
        q, P, L = len(lo), 3, 3
        wmean, S = window_moments(cov, m, mu, _dev(lo, dev), _dev(hi, dev))
        rmean, rS = dense_window_moments(C, mu_h, lo, hi)
        g = (np.arange(q) * P // q).astype(np.int32)
        g[(hi - lo) < (10 if name == "ragged" else 30)] = -1  # partial and empty windows are excluded
        assert (g == -1).any() and all((g == p).any() for p in range(P))
        sd = np.sqrt(np.clip(np.diagonal(rS), 1e-300, None))
        u = rmean[None, :] + sd[None, :] * rng.normal(0.0, 1.0, (L, 1))
        w = np.ones(q)
        got_mean, got_cov = exceedance_moments(S, q, wmean, torch.tensor(u), torch.tensor(w), torch.tensor(g), P)
        keep = g >= 0
        rho = rS[np.ix_(keep, keep)] / np.outer(sd[keep], sd[keep])
        assert np.max(rho[np.tril_indices(keep.sum(), -1)]) > 0.99
        emean, ecov = dense_exceedance_moments(rS, rmean, u, w, g, P)
        W = np.bincount(g[keep], minlength=P).astype(np.float64)
        dm, dc = np.abs(got_mean.cpu().numpy() - emean), np.abs(got_cov.cpu().numpy() - ecov)
        print(f"{name}: mean error / W = {np.max(dm / W[None, :]):.3e}, cov error / (W_g W_h) = {np.max(dc / (W[:, None] * W[None, :])[None]):.3e}")
        assert np.all(dm <= 1e-13 * W[None, :]), name
        assert np.all(dc <= 1e-11 * (W[:, None] * W[None, :])[None]), name


# ------------------------------------------------------------------------------------------------ the engine
def _windowed_reference(mu, cov, lo, hi, keep, u, groups, P):
    """The dense references chained: the windowed moments of (mu, cov), then the exceedance moments of the qualifying outputs."""
    wm, S = dense_window_moments(cov, mu, lo, hi)
    g = np.where(keep, groups, -1).astype(np.int32)
    mean, pc = dense_exceedance_moments(S, wm, np.broadcast_to(np.asarray(u)[:, None], (len(u), len(wm))), np.ones(len(wm)), g, P)
    return wm, S, mean, pc


def test_loadest_rolling_products_end_to_end(gpu_device):
    """``rolling_mean``, ``exceedance(window=)`` and ``duration_curve(window=)`` of a log target on the device against the
    dense references fed from the ORACLE's posterior at the fitted parameters: the end-to-end tolerances of
    tests/test_gpu_exceedance.py (1e-8 of the period's weight; 1e-8 relative for the rolling mean itself).  Then
    ``window="1D"`` on the gap-free daily record: the daily product, bitwise."""
    from scipy.stats import norm

    from discontinuum_amd.loadest_gp import LoadestGP
    from discontinuum_amd.loads import period_groups, target_transform
    from tests.flux_helpers import daily_loadest
    from tests.test_gpu_exceedance import _oracle_posterior

    cov_obs, target, daily = daily_loadest()
    model = LoadestGP()
    model.fit(cov_obs, target, iterations=10)
    _mode, s, t = target_transform(model.dm)
    omu, ocov = _oracle_posterior(model, daily)
    m = len(omu)
    assert m == 1096
    lo, hi = trailing(m, 30)
    keep = (hi - lo) == 30
    time = daily.coords["time"].values
    _o, groups, labels, _n, _d = period_groups(time, np.ones(m), "YE")
    wm = dense_window_moments(ocov, omu, lo, hi)[0]
    tau = np.quantile(np.exp(s * wm[keep] + t), [0.35, 0.7])
    u = (np.log(tau) - t) / s
    wm, S, rmean, rcov = _windowed_reference(omu, ocov, lo, hi, keep, u, groups, len(labels))

    ds, got_S = model.rolling_mean(daily, "30D", return_cov=True)
    sd = np.sqrt(np.diagonal(S)[keep])
    z = norm.ppf(0.975)
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))  # noqa: E731
    e = (rel(ds["mean"].values, np.exp(s * wm[keep] + t)), rel(ds["lower"].values, np.exp(s * (wm[keep] - z * sd) + t)),
         rel(ds["upper"].values, np.exp(s * (wm[keep] + z * sd) + t)), float(np.abs(got_S - S[np.ix_(keep, keep)]).max() / np.abs(S).max()))
    print(f"loadest rolling_mean vs oracle posterior: mean {e[0]:.2e} lower {e[1]:.2e} upper {e[2]:.2e} cov {e[3]:.2e}")
    assert max(e) <= 1e-8 and np.array_equal(ds.coords["time"].values, time[keep]) and np.all(ds["n_points"].values == 30)

    ex, pcov = model.exceedance(daily, threshold=tau, window="30D", freq="YE", return_cov=True)
    n = np.bincount(groups[keep], minlength=len(labels)).astype(np.float64)
    assert np.array_equal(ex["n_points"].values, n)
    print("loadest windowed exceedance vs oracle posterior:", float(np.abs(ex["mean"].values - rmean).max()), float(np.abs(pcov - rcov).max()))
    assert np.all(np.abs(ex["mean"].values - rmean) <= 1e-8 * n[None, :])
    assert np.all(np.abs(pcov - rcov) <= 1e-8 * (n[:, None] * n[None, :])[None])

    dc = model.duration_curve(daily, levels=tau, window="30D")
    _wm, _S, dmean, dcov = _windowed_reference(omu, ocov, lo, hi, keep, u, np.zeros(m, np.int32), 1)
    nk = float(keep.sum())
    print("loadest windowed duration curve vs oracle posterior:", float(np.abs(dc["mean"].values * nk - dmean[:, 0]).max()),
          float(np.abs((dc["se"].values * nk) ** 2 - dcov[:, 0, 0]).max()))
    assert np.all(np.abs(dc["mean"].values * nk - dmean[:, 0]) <= 1e-8 * nk)
    assert np.all(np.abs((dc["se"].values * nk) ** 2 - dcov[:, 0, 0]) <= 1e-8 * nk * nk)

    daily_ds, daily_cov = model.exceedance(daily, threshold=tau, freq="YE", return_cov=True)
    one_ds, one_cov = model.exceedance(daily, threshold=tau, freq="YE", return_cov=True, window="1D")
    assert np.array_equal(one_cov, daily_cov)
    for k in ("mean", "se", "lower", "upper", "n_points"):
        assert np.array_equal(one_ds[k].values, daily_ds[k].values), k


def test_rating_seven_day_mean_flow(gpu_device):
    from scipy.stats import norm

    from discontinuum_amd.loads import target_transform
    from discontinuum_amd.rating_gp import RatingGP
    from tests.flux_helpers import daily_rating
    from tests.test_gpu_exceedance import _oracle_posterior

    cov_obs, target, unc, daily = daily_rating()
    model = RatingGP()
    model.fit(cov_obs, target, target_unc=unc, iterations=10)
    _mode, s, t = target_transform(model.dm)
    omu, ocov = _oracle_posterior(model, daily)
    m = len(omu)
    lo, hi = trailing(m, 7)
    keep = (hi - lo) == 7
    wm, S = dense_window_moments(ocov, omu, lo[keep], hi[keep])
    ds, got_S = model.rolling_mean(daily, "7D", return_cov=True)
    sd = np.sqrt(np.diagonal(S))
    z = norm.ppf(0.975)
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))  # noqa: E731
    e = (rel(ds["mean"].values, np.exp(s * wm + t)), rel(ds["lower"].values, np.exp(s * (wm - z * sd) + t)),
         rel(ds["upper"].values, np.exp(s * (wm + z * sd) + t)), float(np.abs(got_S - S).max() / np.abs(S).max()))
    print(f"rating rolling_mean vs oracle posterior: mean {e[0]:.2e} lower {e[1]:.2e} upper {e[2]:.2e} cov {e[3]:.2e}")
    assert max(e) <= 1e-8 and ds["mean"].values.shape == (m - 6,)


def test_interval_censored_fit_takes_the_same_path(gpu_device):
    """An interval-censored fit (n = 60, 30 % censored rows: non-detects, "greater than" rows and brackets) needs no special
    case: ``exceedance(window="30D")`` against the references fed from the engine's own ``posterior_cov`` (the Laplace
    posterior), rtol 1e-9; ``predict`` gives the same bits before and after."""
    from discontinuum_amd.loadest_gp import LoadestGP, censoring_from_bounds
    from discontinuum_amd.loads import period_groups, target_transform
    from tests import interval_helpers as ih
    from tests.flux_helpers import daily_loadest

    cov_obs, target, daily = daily_loadest(seed=4)
    vals = np.asarray(target.values, dtype=np.float64)
    _y, side, _v, _m, _upper = ih.synth(np.zeros((len(vals), 2)), 0.3, seed=2)  # which rows are censored, and how
    low, high = vals.copy(), vals.copy()
    low[side == -1], high[side == -1] = 0.0, vals[side == -1] * 1.1
    low[side == 1], high[side == 1] = vals[side == 1] * 0.9, np.inf
    low[side == 2], high[side == 2] = vals[side == 2] * 0.8, vals[side == 2] * 1.3
    tgt, codes, upper = censoring_from_bounds(low, type(target)(high, dims=target.dims, coords=target.coords, name=target.name,
                                                               attrs=target.attrs))
    assert 15 <= (codes != 0).sum() <= 21 and (codes == 2).sum() >= 4 and (codes == -1).sum() >= 4
    model = LoadestGP()
    model.fit(cov_obs, tgt, iterations=8, censored=codes, target_upper=upper)
    before = [a.values.copy() for a in model.predict(daily)]
    _mode, s, t = target_transform(model.dm)
    tau = np.quantile(before[0], [0.4, 0.7])
    ex, pcov = model.exceedance(daily, threshold=tau, window="30D", freq="YE", return_cov=True)
    x = torch.tensor(model.dm.Xnew(daily), dtype=model.dtype).to(model.device).contiguous()
    model._eval_ready(x)
    with torch.no_grad():
        kmean, cov = model._plan.posterior_cov(model._factor_theta, x)
        mu = (kmean + model.model.prior_mean(x)).double().cpu().numpy()
    m = len(mu)
    C = symmetrise_lower(cov[:m, :m].double()).cpu().numpy()
    lo, hi = trailing(m, 30)
    keep = (hi - lo) == 30
    _o, groups, labels, _n, _d = period_groups(daily.coords["time"].values, np.ones(m), "YE")
    _wm, _S, rmean, rcov = _windowed_reference(mu, C, lo, hi, keep, (np.log(tau) - t) / s, groups, len(labels))
    print("interval-censored windowed exceedance:", float(np.max(np.abs(ex["mean"].values - rmean) / np.abs(rmean))),
          float(np.max(np.abs(pcov - rcov) / np.abs(rcov).max())))
    assert np.allclose(ex["mean"].values, rmean, rtol=1e-9, atol=1e-12)
    assert np.allclose(pcov, rcov, rtol=1e-9, atol=1e-9 * float(np.abs(rcov).max()))
    after = [a.values for a in model.predict(daily)]
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
