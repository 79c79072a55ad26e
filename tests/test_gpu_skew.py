"""GPU parity of ``dgp_period_third_moments`` (the exact third central moment of period sums) and of the API above it:
``LoadestGP.annual_flux(interval="three-moment")``, ``annual_flux_many``.

The kernel is checked against the dense closed form (tests/skew_helpers.py::dense_third_moments) in torch fp64 on the SAME
``dgp_posterior_cov`` buffer, symmetrised from its lower triangle -- the bounds ``tests/test_gpu_flux.py`` holds
``dgp_period_moments`` to: 1e-11 relative to the largest output entry for fp64 buffers, 1e-9 for fp32 buffers against the fp64
formula on the same fp32 values -- on both tile cores; the API against the oracle posterior plus the dense formulas (1e-8).
"""
import numpy as np
import pytest
import torch

from discontinuum_amd.backend import MODE_LOG, GPPlan, period_moments, period_third_moments
from discontinuum_amd.loadest_gp import LoadestGP, annual_flux_many
from discontinuum_amd.loads import period_groups, target_transform, three_moment_intervals
from oracle import gp_oracle as orc
from tests.flux_helpers import daily_loadest, dense_period_moments, symmetrise_lower
from tests.skew_helpers import dense_third_moments

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 127, 129, 257)


def _posterior_buffers(dev, dtype, ms, n=200, d=2, seed=0):
    """{m: (M, M) dgp_posterior_cov buffer} from one factorised loadest plan."""
    X, y = orc.synth_loadest(n, d, seed=seed)
    X, y = torch.tensor(X), torch.tensor(y)
    theta = torch.full((orc.loadest_ntheta(d),), 0.6931471805599453, dtype=torch.float64)
    plan = GPPlan("loadest", n, d, dtype=dtype, device=dev)
    plan.set_inputs(X.to(dev, dtype).contiguous())
    plan.factorize(theta, (y - y.mean()).to(dev, dtype).contiguous(), torch.full((n,), 0.05, dtype=dtype, device=dev))
    g = torch.Generator().manual_seed(seed + 1)
    out = {}
    for m in ms:
        Xs = (torch.rand(m, d, generator=g, dtype=torch.float64) * 4 - 2).to(dev, dtype).contiguous()
        _mean, cov = plan.posterior_cov(theta, Xs)
        out[m] = cov
    return out


def _layouts(m):
    """One period; every point its own period; ragged periods whose ends straddle 64 and 128; the same with excluded points
    at both ends, inside a period and over a period's end."""
    i = np.arange(m)
    ragged = np.searchsorted(np.array([50, 70, 120, 135, 200]), i, side="right")
    holes = ragged.copy()
    holes[: min(3, m)] = -1
    holes[m // 2] = -1
    holes[60:72] = -1
    holes[max(0, m - 2):] = -1
    out = {"one": np.zeros(m, np.int32), "each": i, "ragged": ragged}
    if m > 5:
        out["holes"] = holes
    return out


def _ngroups(g):
    return int(max(g.max(), 0)) + 1


def _rel(a, b):
    scale = float(b.abs().max())
    return float((a - b).abs().max()) / (scale if scale > 0 else 1.0)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_kernel_matches_the_dense_formula(dtype, gpu_device):
    dev = gpu_device
    bufs = _posterior_buffers(dev, dtype, SIZES)
    tol = 1e-11 if dtype == torch.float64 else 1e-9
    rng = np.random.default_rng(5)
    worst = 0.0
    for m in SIZES:
        cov = bufs[m]
        C = symmetrise_lower(cov[:m, :m].double())
        mu = torch.tensor(0.3 * rng.standard_normal(m), dtype=dtype, device=dev)
        w = torch.tensor(rng.uniform(0.5, 2.0, m), dtype=torch.float64, device=dev)
        ev = torch.tensor(rng.uniform(0.0, 0.1, m), dtype=dtype, device=dev)
        for name, g in _layouts(m).items():
            P = _ngroups(g)
            gt = torch.tensor(g, dtype=torch.int32, device=dev)
            for extra in (None, ev) if name in ("ragged", "holes") else (None,):
                ref = dense_third_moments(C, mu.double(), 0.7, w, gt, P, None if extra is None else extra.double())
                assert float(ref.max()) > 0
                for tile in (0, 64, 128):
                    k3 = period_third_moments(cov, m, mu, 0.7, w, gt, P, extra_var=extra, tile=tile)
                    err = _rel(k3, ref)
                    worst = max(worst, err)
                    assert err <= tol, (m, name, extra is not None, tile, err)
                    if name == "holes":
                        assert float(k3[ref == 0].abs().max() if bool((ref == 0).any()) else 0.0) == 0.0
    print(f"dgp_period_third_moments against the dense formula, {dtype}: worst {worst:.2e} (bound {tol:.0e})")


def test_repeatable_batch_independent_and_core_independent(gpu_device):
    dev = gpu_device
    sizes = (300, 200, 130)
    bufs = [_posterior_buffers(dev, torch.float64, (300,), seed=s)[300] for s in (3, 4, 5)]
    rng = np.random.default_rng(7)
    mus = [torch.tensor(0.3 * rng.standard_normal(300), device=dev) for _ in sizes]
    ws = [torch.tensor(rng.uniform(0.5, 2.0, 300), device=dev) for _ in sizes]
    gs = [np.where(np.arange(300) < mb, np.arange(300) // 45, -1).astype(np.int32) for mb in sizes]
    P = max(_ngroups(g) for g in gs)
    cov3 = torch.stack(bufs).contiguous()
    s2 = torch.tensor([0.7, 0.5, 0.9], dtype=torch.float64)
    args = (cov3, 300, torch.stack(mus), s2, torch.stack(ws), torch.tensor(np.stack(gs), device=dev), P)
    for tile in (0, 64, 128):
        a, b = period_third_moments(*args, tile=tile), period_third_moments(*args, tile=tile)
        assert torch.equal(a, b), tile  # bitwise
    k64, k128 = period_third_moments(*args, tile=64), period_third_moments(*args, tile=128)
    assert _rel(k64, k128) <= 1e-11  # the two cores sum k in different orders: the bound of the kernel test
    batch = period_third_moments(*args)
    worst = 0.0
    for b, mb in enumerate(sizes):
        Mb = -(-mb // 128) * 128
        single = bufs[b][:Mb, :Mb].contiguous()
        pb = _ngroups(gs[b][:mb])
        for tile, many in ((0, batch), (128, k128)):
            k1 = period_third_moments(single, mb, mus[b][:mb], float(s2[b]), ws[b][:mb], torch.tensor(gs[b][:mb], device=dev), pb,
                                      tile=tile)
            worst = max(worst, _rel(many[b, :pb], k1))
            assert _rel(many[b, :pb], k1) <= 1e-12, (b, tile)
        if pb < P:
            assert float(batch[b, pb:].abs().max()) == 0.0
    print(f"a site alone against the same site in a ragged batch of 3: worst {worst:.2e}")


def _oracle_reference(model, daily, weights, freq, ci=0.95):
    """Oracle posterior at the daily points + the dense formulas: skewness and the three-moment interval."""
    model._ensure_factor()
    x = model._train_x.cpu().double()
    with torch.no_grad():
        r = (model._train_y - model.model.prior_mean(model._train_x)).cpu().double()
        noise = model.likelihood.train_noise(torch.device("cpu"), torch.float64).reshape(-1)
        xs = torch.tensor(model.dm.Xnew(daily), dtype=torch.float64)
        kmean, cov = orc.posterior(model._plan.model, x, r, noise, model._factor_theta.cpu().double(), xs, full_cov=True)
        mu = kmean + model.model.prior_mean(xs.to(model.device)).cpu().double()
    mode, s, t = target_transform(model.dm)
    assert mode == MODE_LOG
    order, groups, labels, _n, _d = period_groups(daily.coords["time"].values, weights, freq)
    assert np.array_equal(order, np.arange(len(order)))
    mean, pcov = dense_period_moments(cov, s * mu + t, s * s, torch.tensor(weights), groups, len(labels), mode)
    var = np.diagonal(pcov.numpy())
    skew = dense_third_moments(cov, s * mu + t, s * s, torch.tensor(weights), groups, len(labels)).numpy() / var ** 1.5
    return skew, three_moment_intervals(mean.numpy(), var, skew, ci)


def _close(a, b):
    return _rel(torch.tensor(np.asarray(a)), torch.tensor(np.asarray(b)))


def test_annual_flux_end_to_end_and_default_untouched(gpu_device):
    cov_obs, target, daily = daily_loadest(n_obs=300, seed=11)
    model = LoadestGP()
    model.fit(cov_obs, target, iterations=20)
    before = model.annual_flux(daily)
    ds = model.annual_flux(daily, interval="three-moment")
    after = model.annual_flux(daily)
    for key in ("mean", "se", "lower", "upper", "n_points"):  # the default before and after a three-moment call: bitwise
        assert np.array_equal(before[key].values, after[key].values), key
    assert "skewness" not in after and "interval" not in after.attrs
    assert np.array_equal(ds["mean"].values, before["mean"].values) and np.array_equal(ds["se"].values, before["se"].values)
    w = np.asarray(daily["flow"].values) * 86400 * 1e-3
    skew, (lo, hi, clipped) = _oracle_reference(model, daily, w, "YE")
    print(f"annual_flux three-moment against the oracle: skewness {_close(ds['skewness'].values, skew):.2e}, lower "
          f"{_close(ds['lower'].values, lo):.2e}, upper {_close(ds['upper'].values, hi):.2e}; skewness {skew}")
    assert _close(ds["skewness"].values, skew) <= 1e-8
    assert _close(ds["lower"].values, lo) <= 1e-8 and _close(ds["upper"].values, hi) <= 1e-8
    assert ds.attrs["interval"] == "three-moment" and ds.attrs["clipped_lower"] == clipped


def test_annual_flux_many_matches_single_sites(gpu_device):
    specs = [(150, "2012-01-01", "2014-01-01"), (200, "2011-06-01", "2013-01-01"), (120, "2012-01-01", "2013-07-01")]
    models, dailies = [], []
    for k, (n, start, end) in enumerate(specs):
        cov_obs, target, daily = daily_loadest(n_obs=n, start=start, end=end, seed=20 + k)
        mdl = LoadestGP()
        mdl.fit(cov_obs, target, iterations=10)
        models.append(mdl)
        dailies.append(daily)
    singles = [mdl.annual_flux(d, freq="YE-SEP", interval="three-moment") for mdl, d in zip(models, dailies)]
    many = annual_flux_many(models, dailies, freq="YE-SEP", interval="three-moment")
    for one, ds in zip(singles, many):
        assert np.array_equal(one.coords["time"].values, ds.coords["time"].values)
        for key in ("mean", "se", "skewness", "lower", "upper"):
            assert _close(ds[key].values, one[key].values) <= 1e-8, key
        assert ds.attrs["interval"] == "three-moment"


def test_censored_fit_takes_the_same_path(gpu_device):
    """A fit with non-detects: the skewness is the dense formula on the latent (Laplace) posterior covariance the plan holds."""
    cov_obs, target, daily = daily_loadest(n_obs=120, end="2014-01-01", seed=5)
    vals = np.asarray(target.values, dtype=np.float64)
    order = np.argsort(vals)
    mask = np.zeros(120, dtype=bool)
    mask[order[:18]] = True
    reported = vals.copy()
    reported[mask] = vals[order[18]]
    reported = type(target)(reported, dims=target.dims, coords=target.coords, name=target.name, attrs=target.attrs)
    model = LoadestGP()
    model.fit(cov_obs, reported, iterations=10, censored=mask)
    ds = model.annual_flux(daily, interval="three-moment")
    plain = model.annual_flux(daily)
    assert np.array_equal(ds["mean"].values, plain["mean"].values) and np.array_equal(ds["se"].values, plain["se"].values)
    with torch.no_grad():
        xs = torch.tensor(model.dm.Xnew(daily), dtype=model.dtype).to(model.device).contiguous()
        m = xs.shape[0]
        kmean, cov = model._plan.posterior_cov(model._factor_theta, xs)
        mu = (kmean + model.model.prior_mean(xs)).double()
    _mode, s, t = target_transform(model.dm)
    w = torch.tensor(np.asarray(daily["flow"].values) * 86400 * 1e-3, device=cov.device)
    _o, groups, labels, _n, _d = period_groups(daily.coords["time"].values, w.cpu().numpy(), "YE")
    C = symmetrise_lower(cov[:m, :m].double())
    _mean, pcov = dense_period_moments(C, s * mu + t, s * s, w, groups, len(labels), MODE_LOG)
    skew = dense_third_moments(C, s * mu + t, s * s, w, groups, len(labels)) / pcov.diagonal() ** 1.5
    assert _close(ds["skewness"].values, skew.cpu().numpy()) <= 1e-8
    assert np.all(ds["skewness"].values > 0) and np.all(ds["lower"].values < ds["mean"].values)
