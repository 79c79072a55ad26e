"""GPU parity of the streamed value of additional samples: ``dgp_posterior_sample_value`` (the gain map with the posterior
covariance produced in row panels), ``dgp_posterior_cov_columns``, ``dgp_lowrank_period_moments`` and the ``streamed=True``
path of ``sample_value`` / ``design_value`` / ``design`` above them.

1. The gain map against the DIRECT double sum (``design_helpers.direct_gain``, never the series) on the dense
   ``posterior_cov`` buffer of the same plan, symmetrised from its lower triangle, with the conditioning done by a dense solve.
   The bounds are tests/test_gpu_design.py's: per entry 1e-12 (sum_{i in p} |A_i|)^2 max(1, expm1 beta), ``var_out`` 1e-14 of
   max(C_cc + tau^2).  One thing differs by the entry's own definition: the streamed pass takes C_cc from the PREDICTED
   variance, never from a panel's diagonal, so the reference carries ``predict``'s variance on the diagonal of the buffer;
   everything off the diagonal is the buffer's.  The two diagonals are two roundings of k(x, x) - sum V^2: a float32 plan stores
   them 6e-8 relative apart, a float64 plan up to 1.2e-14 of C_cc where C_cc << k(x, x) (measured: rating, n = 300, m = 1), which
   is above ``var_out``'s 1e-14 although the entry reproduces its own definition to the last bit or two.  float64 plans are
   ALSO held to the unmodified buffer for the gain map, at the same bound; ``var_out`` against the buffer's diagonal is printed.
2. Regrouping (panels of 128 rows against one panel), repeated calls, ragged batches against single-site plans (bitwise where the
   factorisation is),
   independence of the batch companions, a work area full of NaN, ``predict`` before and after.
3. ``posterior_cov_columns`` against the dense buffer at 1e-8 of its largest entry: the tolerance
   tests/test_gpu_sample.py::test_posterior_cov_fp64 holds ``posterior_cov`` itself to against the oracle.
4. ``lowrank_period_moments`` against ``period_moments`` on the dense R = B^T B (torch GEMM): 1e-11 of the largest entry.
5. The C entries through ctypes: sizes, alignment, ``panel_rows``, no factorisation.
6. ``LoadestGP`` / ``RatingGP`` with ``streamed=True`` against the default path.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from discontinuum_amd.backend import GPPlan, _ptr, _stream, lowrank_period_moments, period_moments, series_terms
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.rating_gp import RatingGP
from tests.design_helpers import direct_gain, linear_gain, rows_by_cholesky
from tests.flux_helpers import daily_loadest, daily_rating, symmetrise_lower
from tests.test_gpu_design import _ratio
from tests.test_gpu_exceedance import _groups
from tests.test_gpu_exceedance_stream import _held, _points
from tests.test_gpu_influence import _ragged
from tests.test_gpu_stages import make_case

pytestmark = pytest.mark.gpu

MS = (1, 127, 129, 300, 385)  # one block; one short of full; two blocks, a one-row second panel; 3 and 4 blocks
NROWS = (0, 1, 5, 64)
PANELS = (128, 256, 512)      # one-, two- and multi-panel runs; 512 >= M is the single-panel run


def _dense(plan, theta, xs, m):
    """(symmetric C (m, m) float64 from the dense buffer, predicted variance (m,) float64)."""
    _kmean, cov = plan.posterior_cov(theta, xs)
    var = plan.predict(theta, xs)[1]
    return symmetrise_lower(cov[:m, :m].double()).cpu().numpy(), var.double().cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the direct double sum
@pytest.mark.parametrize("n", [1, 129, 300])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", ["loadest", "rating"])
def test_streamed_gain_map_matches_the_direct_sum(name, dtype, n, gpu_device):
    """Worst error / bound measured on MI355X: see DESIGN.md, "Streamed value of additional samples"."""
    dev = gpu_device
    plan, _model, d, _X, _r, _noise, theta = _held(name, n, dev, dtype=dtype)
    rng = np.random.default_rng(11)
    worst = {"series": 0.0, "K=64": 0.0, "K=1": 0.0, "var": 0.0}
    dv = lambda x, dt=torch.float64: None if x is None else torch.tensor(x, dtype=dt, device=dev)  # noqa: E731
    for im, m in enumerate(MS):
        xs = _points(name, d, m, seed=3 + m).to(dev, dtype).contiguous()
        Cbuf, varp = _dense(plan, theta, xs, m)
        Cs = Cbuf.copy()
        np.fill_diagonal(Cs, varp)  # (see the module docstring)
        diag = np.diagonal(Cs).copy()
        worst["diag"] = max(worst.get("diag", 0.0), float(np.abs(varp - np.diagonal(Cbuf)).max() / (1e-14 * np.diagonal(Cbuf).max())))
        a = rng.uniform(0.5, 2.0, m)
        if m > 4:
            a[3] = 0.0
        ov_t = torch.tensor(rng.uniform(0.5, 2.0, m) * diag.max(), dtype=dtype, device=dev)
        if m >= 127:
            ov_t[40] = -2.0 * float(diag[40]) - 1.0  # v'_40 < 0 on both sides: a candidate that carries nothing
        ov = ov_t.double().cpu().numpy()
        for ip, P in enumerate((3, 40) if m == 385 else (1, 3, 40)):
            g = _groups(m, P)
            top = diag[g >= 0].max() if (g >= 0).any() else diag.max()
            beta = (1.65, 0.5)[(im + ip) % 2]
            s2 = beta / top
            K = series_terms(beta)
            nrows = NROWS[(im + ip) % 4]
            for it, (tau2, tau2_t, nr) in enumerate(((None, None, 0), (ov, ov_t, nrows))):
                pool = np.setdiff1d(np.arange(m), [40]) if m >= 127 else np.arange(m)
                S = rng.choice(pool, nr, replace=nr > len(pool)) if nr else np.zeros(0, dtype=np.int64)
                B = rows_by_cholesky(Cs, S, tau2) if nr else None
                ref, _vref = direct_gain(Cs, a, s2, g, P, tau2, S)
                lin = linear_gain(Cs, a, s2, g, P, tau2, S)
                buf = direct_gain(Cbuf, a, s2, g, P, tau2, S)[0] if dtype == torch.float64 else None  # (rows B: both within 1e-14)
                tag = (name, dtype, n, m, P, nr, tau2 is not None)
                rot = PANELS[(im + ip + it) % 3]
                runs = [("series", K, ref, R) for R in PANELS] + [("K=64", 64, ref, rot), ("K=1", 1, lin, rot)]
                for what, nt, want, R in runs:
                    gain, var = plan.posterior_sample_value(theta, xs, dv(a), s2, dv(g, torch.int32), P, obs_var=tau2_t, rows=dv(B),
                                                            nterms=nt, panel_rows=R)
                    gain, var = gain.cpu().numpy(), var.cpu().numpy()
                    r = _ratio(gain, want, a, g, P, beta)
                    worst[what] = max(worst[what], r)
                    vwant = diag - (0.0 if B is None else (B ** 2).sum(axis=0)) + (0.0 if tau2 is None else tau2)
                    verr = float(np.abs(var - np.clip(vwant, 0.0, None)).max() / (1e-14 * (diag + (0.0 if tau2 is None else tau2)).max()))
                    worst["var"] = max(worst["var"], verr)
                    print(f"{tag} {what} R={R}: gain error / bound {r:.3e}, var error / bound {verr:.3e}")
                    assert r <= 1.0, (tag, what, R, r)
                    assert verr <= 1.0, (tag, what, R, "var", verr)
                    if buf is not None and what != "K=1":
                        rb = _ratio(gain, buf, a, g, P, beta)
                        worst["buffer"] = max(worst.get("buffer", 0.0), rb)
                        assert rb <= 1.0, (tag, what, R, "against the unmodified buffer", rb)
                    if m >= 127 and tau2 is not None:
                        assert np.all(gain[:, 40] == 0) and var[40] == 0, tag
                    assert np.all(np.isfinite(gain)) and np.all(gain >= 0), tag
    print(f"{name} {dtype} n={n}: worst error / bound: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


def test_nan_weight_poisons_its_own_group_only(gpu_device):
    dev, m, P = gpu_device, 300, 3
    plan, _model, d, _X, _r, _noise, theta = _held("loadest", 129, dev)
    xs = _points("loadest", d, m, seed=5).to(dev).contiguous()
    g = _groups(m, P)  # (group 1 is empty)
    a = np.random.default_rng(1).uniform(0.5, 2.0, m)
    day = int(np.nonzero(g == 2)[0][7])
    a[day] = np.nan
    a[0] = np.nan  # an excluded day: its weight is never read into a sum
    assert g[0] < 0
    for R in (128, 384):
        gain, var = plan.posterior_sample_value(theta, xs, torch.tensor(a), 0.7, torch.tensor(g), P, nterms=12, panel_rows=R)
        assert torch.isnan(gain[2]).all() and torch.isfinite(gain[0]).all() and torch.isfinite(var).all()
        assert bool((gain[1] == 0).all())


# ------------------------------------------------------------------------------------------------ 2. regrouping, determinism
def test_regrouping_repeats_work_area_and_the_held_fit(gpu_device):
    dev, m, P, K = gpu_device, 385, 3, 21
    plan, _model, d, _X, _r, _noise, theta = _held("loadest", 300, dev)
    xs = _points("loadest", d, m, seed=8).to(dev).contiguous()
    rng = np.random.default_rng(2)
    a, g = torch.tensor(rng.uniform(0.5, 2.0, m)), torch.tensor(_groups(m, P))
    rows = torch.tensor(rng.normal(0.0, 0.02, (5, m)), device=dev)
    before = plan.predict(theta, xs)
    var = before[1].double()
    beta = 1.65
    s2 = beta / float(var.max())
    ov = (0.5 * var.max() * torch.ones(m, device=dev, dtype=torch.float64)).contiguous()
    call = lambda R: plan.posterior_sample_value(theta, xs, a, s2, g, P, obs_var=ov, rows=rows, nterms=K, panel_rows=R)  # noqa: E731
    g128, v128 = call(128)
    gfull, vfull = call(512)
    r = _ratio(g128.cpu().numpy(), gfull.cpu().numpy(), a.numpy(), g.numpy(), P, beta)
    print(f"panels of 128 rows against one panel: difference / bound {r:.3e}")
    assert r <= 2.0 and torch.equal(v128, vfull)
    again = call(128)
    assert torch.equal(again[0], g128) and torch.equal(again[1], v128)
    plan._psv_ws.fill_(255)  # every double and float of the work area a NaN
    dirty = call(128)
    assert torch.equal(dirty[0], g128) and torch.equal(dirty[1], v128)
    after = plan.predict(theta, xs)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


def test_ragged_batch_equals_single_sites(gpu_device):
    """A ragged batch of three sites (300, 129, 257 training rows) against single-site plans.  The pass itself is
    batch-independent to the bit (the companions test below); whether a single-site PLAN gives the same bits is decided
    upstream, by the factorisation: a plan of order 129 pads to N = 256 and runs another blocked schedule than site 1 of the
    batch, padded to N = 384, so its V -- and everything after it -- agrees to rounding only (tests/test_gpu_excess_stream.py
    holds the streamed excess to 1e-11 there).  Every site whose own padded order is the batch's must agree bitwise; every site within the
    gain map's bound; which sites agreed bitwise is printed."""
    dev, sizes, m, P, K = gpu_device, (300, 129, 257), 300, 3, 21
    pb, cases, theta, Xs = _ragged("loadest", 3, sizes, m, dev, seed0=40)
    xs = Xs.to(dev).contiguous()
    rng = np.random.default_rng(3)
    a = torch.tensor(rng.uniform(0.5, 2.0, (3, m)))
    g = torch.tensor(np.stack([_groups(m, P)] * 3))
    rows = torch.tensor(rng.normal(0.0, 0.02, (3, 5, m)), device=dev)
    ov = torch.tensor(rng.uniform(0.01, 0.05, (3, m)), device=dev)
    var_b = pb.predict(theta, xs)[1]
    s2 = torch.tensor([0.9, 1.1, 1.3], dtype=torch.float64)
    gain, var = pb.posterior_sample_value(theta, xs, a, s2, g, P, obs_var=ov, rows=rows, nterms=K, panel_rows=128)
    assert gain.shape == (3, P, m) and torch.isfinite(gain).all()
    again = pb.posterior_sample_value(theta, xs, a, s2, g, P, obs_var=ov, rows=rows, nterms=K, panel_rows=128)
    assert torch.equal(again[0], gain) and torch.equal(again[1], var)
    for b, nb in enumerate(sizes):
        X, r, noise, th = cases[b]
        p1 = GPPlan("loadest", nb, 3, device=dev)
        p1.set_inputs(X.to(dev).contiguous())
        p1.factorize(th, r.to(dev).contiguous(), noise.to(dev).contiguous())
        g1, v1 = p1.posterior_sample_value(th, xs[b].contiguous(), a[b], float(s2[b]), g[b], P, obs_var=ov[b], rows=rows[b], nterms=K,
                                           panel_rows=128)
        bitwise = torch.equal(gain[b], g1) and torch.equal(var[b], v1)
        beta = float(s2[b]) * float(var_b[b].max())
        ratio = _ratio(gain[b].cpu().numpy(), g1.cpu().numpy(), a[b].numpy(), g[b].numpy(), P, beta)
        print(f"site {b} (n = {nb}): bitwise {bitwise}, difference / bound {ratio:.3e}")
        assert bitwise or -(-nb // 128) < -(-max(sizes) // 128), b  # (257 pads to the batch's 384: bitwise)
        assert ratio <= 1.0, (b, ratio)
    # other companions: site 1's bits stay
    a2, ov2, rows2, xs2 = a.clone(), ov.clone(), rows.clone(), xs.clone()
    a2[0], a2[2], ov2[0], rows2[2], xs2[0] = 5.0, 0.1, 0.3, 0.0, xs[2]
    gain2, var2 = pb.posterior_sample_value(theta, xs2, a2, s2, g, P, obs_var=ov2, rows=rows2, nterms=K, panel_rows=128)
    assert torch.equal(gain2[1], gain[1]) and torch.equal(var2[1], var[1])


# ------------------------------------------------------------------------------------------------ 3. columns
@pytest.mark.parametrize("name", ["loadest", "rating"])
def test_columns_match_the_dense_buffer(name, gpu_device):
    """Tolerance: 1e-8 of the largest entry, tests/test_gpu_sample.py::test_posterior_cov_fp64's for ``posterior_cov`` itself."""
    dev = gpu_device
    plan, _model, d, _X, _r, _noise, theta = _held(name, 300, dev)
    for m in (129, 300, 385):
        xs = _points(name, d, m, seed=3 + m).to(dev).contiguous()
        Cs, _var = _dense(plan, theta, xs, m)
        edge = [0, 127, 128, m - 1]
        for idx in ([m - 1], edge + [int(i) for i in np.random.default_rng(m).integers(0, m, 60)]):
            cols = plan.posterior_cov_columns(theta, xs, idx)
            assert cols.shape == (len(idx), m) and cols.dtype == torch.float64
            err = float(np.abs(cols.cpu().numpy() - Cs[idx, :]).max() / np.abs(Cs).max())
            print(f"{name} m={m} ncols={len(idx)}: max |column - buffer| / max |C| = {err:.3e}")
            assert err <= 1e-8
            assert torch.equal(cols, plan.posterior_cov_columns(theta, xs, idx))
    with pytest.raises(ValueError, match="out of range"):
        plan.posterior_cov_columns(theta, xs, [m])
    with pytest.raises(ValueError, match="1 .. 64 columns"):
        plan.posterior_cov_columns(theta, xs, list(range(65)))


# ------------------------------------------------------------------------------------------------ 4. low-rank moments
@pytest.mark.parametrize("mode", [0, 1])
def test_lowrank_period_moments_match_the_dense_r(mode, gpu_device):
    dev = gpu_device
    rng = np.random.default_rng(4)
    worst = 0.0
    for im, m in enumerate(MS):
        M = -(-m // 128) * 128
        for ip, P in enumerate((1, 3, 40)):
            nrows = (1, 4, 12, 64)[(im + ip) % 4]
            rows = torch.tensor(rng.normal(0.0, 0.3 / np.sqrt(nrows), (nrows, m)), device=dev)
            mu = torch.tensor(rng.normal(0.0, 0.3, m), device=dev)
            w, g = torch.tensor(rng.uniform(0.5, 2.0, m)), torch.tensor(_groups(m, P))
            R = torch.zeros(M, M, dtype=torch.float64, device=dev)
            R[:m, :m] = rows.T @ rows
            rmean, rcov = period_moments(R, m, mu, 1.3, w, g, P, mode)
            mean, cov = lowrank_period_moments(rows, m, mu, 1.3, w, g, P, mode)
            scale = float(rcov.abs().max())
            err = float((cov - rcov).abs().max()) / scale if scale > 0 else float((cov - rcov).abs().max())
            merr = float((mean - rmean).abs().max() / rmean.abs().max().clamp_min(1e-300))
            worst = max(worst, err)
            assert err <= 1e-11 and merr <= 1e-13, (m, P, nrows, err, merr)
            assert torch.equal(cov, cov.T)
            again = lowrank_period_moments(rows, m, mu, 1.3, w, g, P, mode)
            assert torch.equal(again[0], mean) and torch.equal(again[1], cov)
    print(f"mode {mode}: worst covariance error / largest entry {worst:.3e}")
    # a batch of two equals the single calls bitwise
    m, P = 300, 3
    rows = torch.tensor(rng.normal(0.0, 0.1, (2, 12, m)), device=dev)
    mu, w = torch.tensor(rng.normal(0.0, 0.3, (2, m)), device=dev), torch.tensor(rng.uniform(0.5, 2.0, (2, m)))
    g = torch.tensor(np.stack([_groups(m, P)] * 2))
    mean2, cov2 = lowrank_period_moments(rows, m, mu, torch.tensor([1.3, 0.7], dtype=torch.float64), w, g, P, mode)
    for b, s2 in enumerate((1.3, 0.7)):
        mean1, cov1 = lowrank_period_moments(rows[b], m, mu[b], s2, w[b], g[b], P, mode)
        assert torch.equal(mean2[b], mean1) and torch.equal(cov2[b], cov1)


# ------------------------------------------------------------------------------------------------ 5. the C entries
def test_c_entries_sizes_and_refusals(gpu_device):
    dev, n, m, P, K = gpu_device, 129, 300, 3, 8
    lib = _lib.load()
    plan, _model, d, X, _r, _noise, theta = _held("rating", n, dev)
    xs = _points("rating", d, m, seed=1).to(dev).contiguous()
    th = plan._theta(theta)
    a = torch.ones(m, dtype=torch.float64, device=dev)
    s2 = torch.ones(1, dtype=torch.float64, device=dev)
    g = torch.tensor(_groups(m, P), dtype=torch.int32, device=dev)
    gain, var = torch.empty(P, m, dtype=torch.float64, device=dev), torch.empty(m, dtype=torch.float64, device=dev)
    need = int(lib.dgp_posterior_sample_value_workspace_bytes(plan._h, m, P, 0, K, 128))
    M, N, e = 384, 256, 8
    assert need > 0 and need >= e * (2 * N * M + 128 * M) + 8 * (M * (2 + P * K) + P)
    buf = torch.empty(need + 512, dtype=torch.uint8, device=dev)
    base = buf.data_ptr() + (-buf.data_ptr()) % 256

    def sv(work, nbytes, R=128, p=plan):
        return lib.dgp_posterior_sample_value(p._h, th, _ptr(xs), m, _ptr(a), _ptr(s2), _ptr(g), P, None, None, 0, K, R,
                                              C.c_void_p(work), nbytes, _ptr(gain), _ptr(var), _stream())

    assert sv(base, need) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(gain).all()
    assert sv(base, need - 1) == _lib.E_WORKSPACE
    assert sv(base + 8, need) == _lib.E_ARG
    assert sv(base, need, R=100) == _lib.E_ARG and b"multiple of 128" in lib.dgp_last_error()
    assert lib.dgp_posterior_sample_value_workspace_bytes(plan._h, m, P, 0, K, 100) == 0
    fresh = GPPlan("rating", n, d, device=dev)
    fresh.set_inputs(X.to(dev).contiguous())
    assert sv(base, need, p=fresh) == _lib.E_STATE
    idx = torch.tensor([0, 5], dtype=torch.int32, device=dev)
    cols = torch.empty(2, m, dtype=torch.float64, device=dev)
    cneed = int(lib.dgp_posterior_cov_columns_workspace_bytes(plan._h, m, 2))
    assert 0 < cneed <= need

    def cc(work, nbytes, p=plan):
        return lib.dgp_posterior_cov_columns(p._h, th, _ptr(xs), m, _ptr(idx), 2, C.c_void_p(work), nbytes, _ptr(cols), _stream())

    assert cc(base, cneed) == 0
    assert cc(base, cneed - 1) == _lib.E_WORKSPACE and cc(base + 8, cneed) == _lib.E_ARG and cc(base, cneed, p=fresh) == _lib.E_STATE
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. the engines
_FITS = {}


def _loadest(days, n_obs, seed):
    key = (days, n_obs, seed)
    if key not in _FITS:
        end = np.datetime64("2012-01-01") + np.timedelta64(days, "D")
        cov_obs, target, daily = daily_loadest(n_obs=n_obs, end=str(end), seed=seed)
        model = LoadestGP()
        model.fit(cov_obs, target, iterations=5)
        _FITS[key] = (model, daily)
    return _FITS[key]


def _count(plan, name):
    calls, real = [], getattr(plan, name)

    def spy(*args, **kwargs):
        calls.append(kwargs.get("panel_rows"))
        return real(*args, **kwargs)

    setattr(plan, name, spy)
    return calls


def _same_datasets(dense, streamed, gain_tol):
    for key in dense:
        x, y = np.asarray(dense[key].values), np.asarray(streamed[key].values)
        if x.dtype.kind not in "fc":
            assert np.array_equal(x, y), key
            continue
        tol = gain_tol if key in ("variance_reduction",) else 1e-9 * max(float(np.abs(x).max()), 1e-300)
        assert np.all(np.abs(x - y) <= tol), (key, float(np.abs(x - y).max()), tol)


def _gain_bound(model, daily, weights, freq):
    """1e-12 (sum |A_i|)^2 max(1, expm1 beta) per period, from the dense path's own inputs."""
    from discontinuum_amd import design as dsg
    from discontinuum_amd.loads import DEFAULT_MAX_BYTES

    fit = dsg._prepare(model, daily, weights, freq, None, DEFAULT_MAX_BYTES)
    a, g = fit.a.cpu().numpy(), np.asarray(fit.groups)
    beta = fit.s2 * float(fit.diag.max())
    SA = np.bincount(g[g >= 0], weights=np.abs(a)[g >= 0], minlength=fit.P)
    return 1e-12 * SA ** 2 * max(1.0, np.expm1(beta)), fit


def test_engines_streamed_sample_value_matches_the_default_path(gpu_device):
    model, daily = _loadest(300, 60, 21)
    cov_obs, target, unc, rdaily = daily_rating(n_obs=60, end="2013-01-01", seed=12)
    rating = RatingGP()
    rating.fit(cov_obs, target, target_unc=unc, iterations=5)
    volume = np.full(len(rdaily.coords["time"].values), 86400.0)  # runoff volume per day of discharge
    for eng, args, weights, data in ((model, (daily,), model._flux_weights(daily), daily), (rating, (rdaily, volume), volume, rdaily)):
        tol, fit = _gain_bound(eng, data, weights, "YE")
        dense = eng.sample_value(*args)
        plan = eng._plan
        M = int(plan.lib.dgp_padded_n(fit.m))
        size = lambda R: int(plan.lib.dgp_posterior_sample_value_workspace_bytes(plan._h, fit.m, fit.P, 64, fit.nterms, R))  # noqa: E731
        budget = size(128) + 10
        assert M > 128 and plan.sample_value_panel_rows(fit.m, fit.P, 64, fit.nterms, budget) == 128
        calls = _count(plan, "posterior_sample_value")
        try:
            streamed = eng.sample_value(*args, streamed=True, max_bytes=budget)
        finally:
            del plan.posterior_sample_value
        assert calls == [128]
        gain_d, gain_s = dense["variance_reduction"].values, streamed["variance_reduction"].values
        r = float((np.abs(gain_d - gain_s) / tol[:, None]).max())
        print(f"{type(eng).__name__}: streamed against dense gain, error / bound {r:.3e}")
        assert r <= 1.0
        _same_datasets(dense, streamed, np.inf)
        with pytest.raises(ValueError, match=r"needs a work area of \d+ bytes"):
            eng.sample_value(*args, streamed=True, max_bytes=1000)


def test_engines_streamed_design_value_and_design(gpu_device):
    model, daily = _loadest(300, 60, 21)
    S = np.random.default_rng(1).choice(300, 12, replace=False)
    for k in (1, 4, 12):
        _ds, V = model.design_value(daily, S[:k], sample_var=0.02, return_cov=True)
        _ds2, V2 = model.design_value(daily, S[:k], sample_var=0.02, return_cov=True, streamed=True)
        err = float(np.abs(V - V2).max() / np.abs(V).max())
        print(f"|S| = {k}: max |V streamed - V dense| / max |V| = {err:.3e}")
        assert err <= 1e-11
    short, sdaily = _loadest(129, 40, 22)
    time = sdaily.coords["time"].values
    for kwargs in (dict(objective="relative"), dict(objective="absolute"), dict(objective="relative", given=time[[20, 77]])):
        plan = short._plan
        tops, real = [], plan.sample_value

        def spy(*a, **kw):
            gain, var = real(*a, **kw)
            tops.append((gain, var))
            return gain, var

        plan.sample_value = spy
        try:
            dense = short.design(sdaily, 6, freq="ME", sample_var=0.02, **kwargs)
        finally:
            del plan.sample_value
        # the dense path's own separation: the smallest relative gap of its top two scores over the steps
        gaps = []
        from discontinuum_amd import design as dsg
        from discontinuum_amd.loads import DEFAULT_MAX_BYTES

        fit = dsg._prepare(short, sdaily, short._flux_weights(sdaily), "ME", 0.02, DEFAULT_MAX_BYTES, extra_buffers=1)
        omega = torch.as_tensor(dsg._objective_weights(fit, kwargs["objective"]), device=tops[0][0].device)
        taken = set(int(i) for i in dsg._day_indices(fit, kwargs.get("given"), "given"))
        for (gain, _var), pick in zip(tops, dense["index"].values):
            score = (omega @ gain).cpu().numpy()
            score[list(taken)] = -np.inf
            best, second = np.sort(score)[::-1][:2]
            gaps.append((best - second) / best)
            taken.add(int(np.nonzero(fit.order == pick)[0][0]))
        print(f"{kwargs['objective']}{' given' if 'given' in kwargs else ''}: smallest relative gap of the dense path's top two {min(gaps):.3e}")
        assert min(gaps) > 1e-6
        streamed = short.design(sdaily, 6, freq="ME", sample_var=0.02, streamed=True, **kwargs)
        assert streamed["index"].values.tolist() == dense["index"].values.tolist()
        ve, ve2 = dense["variance_explained"].values, streamed["variance_explained"].values
        assert np.all(np.abs(ve - ve2) <= 1e-11 * np.abs(ve).max())
