"""GPU parity of the streamed rolling means: the band producer (``dgp_posterior_cov_block``), the variance contraction on a
dense matrix (``dgp_window_variances``), the streamed pass (``dgp_posterior_window_variances``) and ``streamed=True`` of
``rolling_mean`` / ``exceedance_probability(window=)`` above them.

1. Band bits.  loadest d = 2, n = 150 (N = 256), m = 385 (M = 512): every entry of a block on or below the diagonal is
   bitwise ``posterior_cov``'s (float64); a float32 block errs against the float64 dense block at most 2 x what dense float32
   ``posterior_cov`` errs (the factor allows for regrouping only); the sites of a ragged batch have their single-site plans' bits.
2. Dense contraction.  ``window_variances`` on a random SPD matrix against the diagonal of tests/window_helpers.py's
   ``dense_window_moments`` and against the diagonal ``dgp_window_moments`` returns, with tests/test_gpu_window.py's bounds:
   mode 0, 1e-13 of max |mu| for the mean and 1e-12 of max |C| for the variance; mode 1, 1e-11 of the reference's max-norm.
3. Streamed pass.  Against ``window_variances`` on the same plan's dense ``posterior_cov`` with its diagonal replaced by the
   predicted variance, the same bounds, ``panel_rows`` 128 / 256 / 512; repeats, a ragged batch, the held fit, a NaN work area.
4. Reach guard: windows of 200 points declared with reach = 64 are an ordinary refusal (the column clamp keeps every read
   inside the band).
5. End to end: ``streamed=True`` against the dense call, rtol 1e-8 as in tests/test_gpu_window.py.

Measured on MI355X: see EXPERIMENTS.md ("Streamed rolling means").
"""
import ctypes as C

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from discontinuum_amd.backend import MODE_LINEAR, MODE_LOG, GPPlan, _ptr, _stream, window_moments, window_variances
from tests.test_gpu_influence import _ragged
from tests.test_gpu_stages import make_case
from tests.window_helpers import dense_window_moments, trailing, window_cases
from tests.window_stream_helpers import window_stream_bytes

pytestmark = pytest.mark.gpu

N_OBS, D, M_PTS = 150, 2, 385
BLOCKS = ((0, 128, 0), (128, 384, 0), (256, 512, 128), (384, 512, 384))
S2 = 0.7
_CACHE = {}


def _points(m, seed=2):
    """Test points sorted in time (neighbours highly correlated), float64 on the host."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(-2.0, 2.0, m))
    return torch.tensor(np.concatenate([t[:, None], rng.standard_normal((m, D - 1))], axis=1))


def _plan(dev, dtype=torch.float64):
    """The factorised loadest plan of the module and what the tests compare against, computed once per dtype and left
    unchanged: -> dict(plan, theta, xs, mean (m,), var (m,), cov (M, M))."""
    if dtype not in _CACHE:
        X, r, noise, theta = make_case("loadest", D, N_OBS, seed=0, perturb=0.2)
        plan = GPPlan("loadest", N_OBS, D, dtype=dtype, device=dev)
        plan.set_inputs(X.to(dev, dtype).contiguous())
        out = plan.factorize(theta, r.to(dev, dtype).contiguous(), noise.to(dev, dtype).contiguous())
        assert int(out[_lib.OUT_INFO]) == 0 and plan.N == 256
        xs = _points(M_PTS).to(dev, dtype).contiguous()
        mean, cov = plan.posterior_cov(theta, xs)
        _kmean, var = plan.predict(theta, xs)
        _CACHE[dtype] = dict(plan=plan, theta=theta, xs=xs, mean=mean, var=var, cov=cov)
    return _CACHE[dtype]


def _lower_mask(row0, row1, col0, dev):
    r = torch.arange(row0, row1, device=dev)[:, None]
    c = torch.arange(col0, row1, device=dev)[None, :]
    return r >= c


def _dev(a, dev):
    return None if a is None else torch.tensor(a, device=dev)


# ------------------------------------------------------------------------------------------------ 1. band bits
@pytest.mark.parametrize("block", BLOCKS)
def test_block_entries_are_posterior_covs_bits(block, gpu_device):
    dev = gpu_device
    c = _plan(dev)
    row0, row1, col0 = block
    got = c["plan"].posterior_cov_block(c["theta"], c["xs"], row0, row1, col0)
    assert tuple(got.shape) == (row1 - row0, row1 - col0) and c["cov"].shape[0] == 512
    mask = _lower_mask(row0, row1, col0, dev)
    ref = c["cov"][row0:row1, col0:row1]
    assert torch.equal(got[mask].view(torch.int64), ref[mask].view(torch.int64)), int((got[mask] != ref[mask]).sum())
    assert torch.equal(got, c["plan"].posterior_cov_block(c["theta"], c["xs"], row0, row1, col0))


def test_float32_block_error_is_dense_float32s(gpu_device):
    """Both float32 products against the float64 dense block: the band may err at most 2 x what ``posterior_cov`` errs."""
    dev = gpu_device
    c64, c32 = _plan(dev), _plan(dev, torch.float32)
    for row0, row1, col0 in BLOCKS:
        mask = _lower_mask(row0, row1, col0, dev)
        ref = c64["cov"][row0:row1, col0:row1][mask]
        band = c32["plan"].posterior_cov_block(c32["theta"], c32["xs"], row0, row1, col0)
        eb = float((band.double()[mask] - ref).abs().max())
        ed = float((c32["cov"][row0:row1, col0:row1].double()[mask] - ref).abs().max())
        print(f"float32 block {(row0, row1, col0)}: band error {eb:.3e}, dense float32 posterior_cov error {ed:.3e}")
        assert eb <= 2 * ed, (row0, row1, col0, eb, ed)


def test_ragged_batch_blocks_have_the_single_site_bits(gpu_device):
    dev, sizes = gpu_device, [150, 64, 1]
    pb, cases, theta, Xs = _ragged("loadest", D, sizes, M_PTS, dev, seed0=80)
    xs = Xs.to(dev).contiguous()
    for row0, row1, col0 in ((128, 384, 0), (384, 512, 384)):
        got = pb.posterior_cov_block(theta, xs, row0, row1, col0)
        assert tuple(got.shape) == (3, row1 - row0, row1 - col0)
        mask = _lower_mask(row0, row1, col0, dev)
        for b, (nb, case) in enumerate(zip(sizes, cases)):
            p1 = GPPlan("loadest", nb, D, device=dev)
            p1.set_inputs(case[0].to(dev).contiguous())
            p1.factorize(case[3], case[1].to(dev).contiguous(), case[2].to(dev).contiguous())
            one = p1.posterior_cov_block(case[3], xs[b], row0, row1, col0)
            assert torch.equal(got[b][mask].view(torch.int64), one[mask].view(torch.int64)), (b, nb, row0)


# ------------------------------------------------------------------------------------------------ 2. the dense contraction
def _spd(m, seed):
    """A random SPD matrix with a unit-scale diagonal in ``posterior_cov``'s layout ((M, M), identity pad) and a mean."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((m, m + 5))
    Cm = G @ G.T / (m + 5)
    M = -(-m // 128) * 128
    full = np.eye(M)
    full[:m, :m] = Cm
    return full, rng.normal(0.0, 1.0, m)


def _errors(mean, var, rmean, rvar, mode, mumax, cmax):
    if mode == MODE_LINEAR:
        return (float(np.abs(mean - rmean).max()) / (mumax if mumax > 0 else 1.0), float(np.abs(var - rvar).max()) / cmax, 1e-13, 1e-12)
    smax = float(np.abs(rvar).max())
    return (float(np.abs(mean - rmean).max()) / max(float(np.abs(rmean).max()), 1e-300),
            float(np.abs(var - rvar).max()) / (smax if smax > 0 else 1.0), 1e-13, 1e-11)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_window_variances_match_the_dense_formula_and_window_moments(dtype, gpu_device):
    dev = gpu_device
    worst = {0: [0.0, 0.0], 1: [0.0, 0.0]}
    for m in (1, 127, 128, 129, 385):
        full, mu_h = _spd(m, seed=m)
        cov = torch.tensor(full, device=dev).to(dtype).contiguous()
        mu = torch.tensor(mu_h, device=dev).to(dtype).contiguous()
        Cm, mu_r = cov[:m, :m].double().cpu().numpy(), mu.double().cpu().numpy()  # the values the kernel reads
        cmax, mumax = float(np.abs(Cm).max()), float(np.abs(mu_r).max())
        for name, (lo, hi, a) in window_cases(m).items():
            q = len(lo)
            for mode in (MODE_LINEAR, MODE_LOG):
                args = (cov, m, mu, _dev(lo, dev), _dev(hi, dev))
                mean, var = window_variances(*args, a=_dev(a, dev), mode=mode, scale2=S2)
                assert tuple(mean.shape) == (q,) and tuple(var.shape) == (q,) and var.dtype == torch.float64
                rmean, rS = dense_window_moments(Cm, mu_r, lo, hi, a, mode, S2)
                em, ev, tol_m, tol_v = _errors(mean.cpu().numpy(), var.cpu().numpy(), rmean, np.diagonal(rS), mode, mumax, cmax)
                worst[mode] = [max(worst[mode][0], em), max(worst[mode][1], ev)]
                assert em <= tol_m and ev <= tol_v, (m, name, mode, em, ev)
                dmean, dS = window_moments(*args, a=_dev(a, dev), mode=mode, scale2=S2)
                em, ev, tol_m, tol_v = _errors(mean.cpu().numpy(), var.cpu().numpy(), dmean.cpu().numpy(),
                                               torch.diagonal(dS)[:q].cpu().numpy(), mode, mumax, cmax)
                assert em <= tol_m and ev <= tol_v, (m, name, mode, "window_moments", em, ev)
                empty = (hi <= lo) | (np.array([(np.ones(m) if a is None else a)[l:h].sum() for l, h in zip(lo, hi)]) <= 0)
                if empty.any():
                    assert np.all(mean.cpu().numpy()[empty] == 0) and np.all(var.cpu().numpy()[empty] == 0)
    print(f"{dtype}: mode 0 worst mean {worst[0][0]:.3e} var {worst[0][1]:.3e}; mode 1 worst mean {worst[1][0]:.3e} var {worst[1][1]:.3e}")


# ------------------------------------------------------------------------------------------------ 3. the streamed pass
def _dense_reference(c):
    """``posterior_cov``'s buffer with the predicted variance on its diagonal: what the streamed pass contracts."""
    cov = c["cov"].clone()
    cov.diagonal()[:M_PTS] = c["var"]
    return cov


@pytest.mark.parametrize("panel_rows", [128, 256, 512])
def test_streamed_pass_matches_the_dense_contraction(panel_rows, gpu_device):
    dev = gpu_device
    c = _plan(dev)
    plan, theta, xs, mu = c["plan"], c["theta"], c["xs"], c["mean"]
    cov = _dense_reference(c)
    cmax, mumax = float(cov[:M_PTS, :M_PTS].abs().max()), float(mu.abs().max())
    worst = {0: [0.0, 0.0], 1: [0.0, 0.0]}
    cases = window_cases(M_PTS)
    assert int((cases["w200"][1] - cases["w200"][0]).max()) == 200 and int((cases["wm"][1] - cases["wm"][0]).max()) == M_PTS
    for name, (lo, hi, a) in cases.items():
        for mode in (MODE_LINEAR, MODE_LOG):
            kw = dict(a=_dev(a, dev), mode=mode, scale2=S2)
            mean, var = plan.posterior_window_variances(theta, xs, mu, _dev(lo, dev), _dev(hi, dev), panel_rows=panel_rows, **kw)
            rmean, rvar = window_variances(cov, M_PTS, mu, _dev(lo, dev), _dev(hi, dev), **kw)
            em, ev, tol_m, tol_v = _errors(mean.cpu().numpy(), var.cpu().numpy(), rmean.cpu().numpy(), rvar.cpu().numpy(), mode, mumax, cmax)
            worst[mode] = [max(worst[mode][0], em), max(worst[mode][1], ev)]
            assert em <= tol_m and ev <= tol_v, (name, mode, panel_rows, em, ev)
            again = plan.posterior_window_variances(theta, xs, mu, _dev(lo, dev), _dev(hi, dev), panel_rows=panel_rows, **kw)
            assert torch.equal(mean, again[0]) and torch.equal(var, again[1]), (name, mode)
    print(f"panel_rows {panel_rows}: mode 0 worst mean {worst[0][0]:.3e} var {worst[0][1]:.3e}; mode 1 worst mean {worst[1][0]:.3e} "
          f"var {worst[1][1]:.3e}")


@pytest.mark.parametrize("sizes", [[150, 200, 129], [150, 64, 1]])
def test_ragged_batch_matches_the_single_site_plans_bitwise(sizes, gpu_device):
    """A site of a ragged batch against its single-site plan.  The band has the single-site plan's bits whatever the sizes
    (``test_ragged_batch_blocks_have_the_single_site_bits``), and so has the contraction; the PREDICTED variance that the pass
    takes for C_jj is ``dgp_predict``'s, which sums V^2 over N / 32-row slabs of the PADDED training size N -- a site of 64
    rows is summed in other groups inside a batch padded to N = 256 than in its own plan with N = 128 (measured: the variances
    of the sites n = 64 and n = 1 of the second batch differ from their plans' in the last bits, the means do not).  So the
    bitwise statement is made where the padded sizes agree -- all of [150, 200, 129], and the first site of [150, 64, 1] -- and
    the other two sites are held to the pass's own bounds against their single-site plans."""
    dev = gpu_device
    pb, site_cases, theta, Xs = _ragged("loadest", D, sizes, M_PTS, dev, seed0=80)
    xs = Xs.to(dev).contiguous()
    mu = pb.predict_mean(theta, xs)
    cases = window_cases(M_PTS)
    picks = [cases["w30"], cases["centred31"], cases["weights"]]
    lo3, hi3 = np.stack([p[0] for p in picks]), np.stack([p[1] for p in picks])
    a3 = np.stack([np.ones(M_PTS) if p[2] is None else p[2] for p in picks])
    s2 = [0.7, 0.5, 0.9]
    for mode in (MODE_LINEAR, MODE_LOG):
        mean, var = pb.posterior_window_variances(theta, xs, mu, _dev(lo3, dev), _dev(hi3, dev), a=_dev(a3, dev), mode=mode, scale2=s2,
                                                  panel_rows=128)
        assert tuple(mean.shape) == (3, M_PTS) and torch.isfinite(var).all()
        for b, (nb, case) in enumerate(zip(sizes, site_cases)):
            p1 = GPPlan("loadest", nb, D, device=dev)
            p1.set_inputs(case[0].to(dev).contiguous())
            p1.factorize(case[3], case[1].to(dev).contiguous(), case[2].to(dev).contiguous())
            one = p1.posterior_window_variances(case[3], xs[b], mu[b], _dev(lo3[b], dev), _dev(hi3[b], dev), a=_dev(a3[b], dev), mode=mode,
                                                scale2=s2[b], panel_rows=128)
            if p1.N == pb.N:
                assert torch.equal(mean[b], one[0]) and torch.equal(var[b], one[1]), (mode, b, nb)
            else:  # (mode 1: the mean holds exp(s2 C_jj / 2) too)
                scale = float(p1.posterior_cov(case[3], xs[b])[1].abs().max()) if mode == MODE_LINEAR else float(one[1].abs().max())
                em = float((mean[b] - one[0]).abs().max()) / float(one[0].abs().max())
                ev = float((var[b] - one[1]).abs().max()) / scale
                print(f"sizes {sizes} site {b} (n = {nb}, N = {p1.N} alone, {pb.N} in the batch) mode {mode}: mean {em:.3e} variance {ev:.3e}")
                assert em <= 1e-13 and ev <= (1e-12 if mode == MODE_LINEAR else 1e-11), (mode, b, nb, em, ev)


def test_work_area_contents_do_not_matter_and_the_held_fit_survives(gpu_device):
    dev = gpu_device
    X, r, noise, theta = make_case("loadest", D, N_OBS, seed=0, perturb=0.2)
    plan = GPPlan("loadest", N_OBS, D, device=dev)
    plan.set_inputs(X.to(dev).contiguous())
    out, _dr, _dn = plan.fit_step(theta, r.to(dev), noise.to(dev))
    assert int(out[_lib.OUT_INFO]) == 0
    xs = _points(M_PTS).to(dev).contiguous()
    bufs = (_lib.BUF_A, _lib.BUF_T, _lib.BUF_ALPHA)
    before = [plan.buffer(b).clone() for b in bufs]
    mu = plan.predict_mean(theta, xs)
    lo, hi, a = window_cases(M_PTS)["w200"]
    for mode in (MODE_LINEAR, MODE_LOG):
        for R in (128, 256):
            args = (theta, xs, mu, _dev(lo, dev), _dev(hi, dev))
            first = plan.posterior_window_variances(*args, mode=mode, scale2=S2, panel_rows=R)
            assert torch.isfinite(first[0]).all() and torch.isfinite(first[1]).all()
            ws = plan._pwv_ws[: plan._pwv_ws.numel() // 8 * 8].view(torch.float64)
            ws.fill_(float("nan"))
            dirty = plan.posterior_window_variances(*args, mode=mode, scale2=S2, panel_rows=R)
            assert torch.equal(first[0], dirty[0]) and torch.equal(first[1], dirty[1]), (mode, R)
    after = [plan.buffer(b) for b in bufs]
    for k, (x, y) in enumerate(zip(before, after)):
        assert torch.equal(x.reshape(-1).view(torch.int64), y.reshape(-1).view(torch.int64)), k
    # the documented size
    q = len(lo)
    for R, reach in ((128, 200), (256, 30), (512, 385), (4096, 1)):
        assert int(plan.lib.dgp_posterior_window_variances_workspace_bytes(plan._h, M_PTS, q, reach, R)) == \
            window_stream_bytes(N_OBS, M_PTS, D, q, reach, 8, R), (R, reach)


# ------------------------------------------------------------------------------------------------ 4. the reach guard
def test_a_window_longer_than_reach_is_an_ordinary_refusal(gpu_device):
    dev = gpu_device
    c = _plan(dev)
    plan, theta, xs, mu = c["plan"], c["theta"], c["xs"], c["mean"]
    lo, hi = trailing(M_PTS, 200)
    q = len(lo)
    lo_d, hi_d = _dev(lo, dev), _dev(hi, dev)
    lib = plan.lib
    th = (C.c_double * theta.numel())(*theta.tolist())
    mean_out = torch.empty(q, dtype=torch.float64, device=dev)
    var_out = torch.empty(q, dtype=torch.float64, device=dev)

    def call(reach):
        need = int(lib.dgp_posterior_window_variances_workspace_bytes(plan._h, M_PTS, q, reach, 128))
        work = torch.empty(need + 256, dtype=torch.uint8, device=dev)
        base = work.data_ptr() + (-work.data_ptr()) % 256
        rc = lib.dgp_posterior_window_variances(plan._h, th, _ptr(xs), M_PTS, _ptr(mu), None, None, _ptr(lo_d), _ptr(hi_d), q, 0, reach, 128,
                                                C.c_void_p(base), need, _ptr(mean_out), _ptr(var_out), _stream())
        torch.cuda.synchronize(dev)
        return rc

    assert call(64) == _lib.E_ARG and b"a window holds more than reach points" in lib.dgp_last_error()
    assert call(200) == 0  # the process goes on: the same call with the true reach
    good = plan.posterior_window_variances(theta, xs, mu, lo_d, hi_d, panel_rows=128)
    assert torch.equal(mean_out, good[0]) and torch.equal(var_out, good[1])


# ------------------------------------------------------------------------------------------------ 5. end to end
def _same_dataset(got, ref, tag):
    assert set(got) == set(ref) and got.attrs == ref.attrs, tag
    assert np.array_equal(got.coords["time"].values, ref.coords["time"].values), tag
    assert np.array_equal(got["n_points"].values, ref["n_points"].values), tag
    for k in ("mean", "se", "lower", "upper"):
        x, y = np.asarray(got[k].values, np.float64), np.asarray(ref[k].values, np.float64)
        print(f"{tag} {k}: max relative difference {float(np.max(np.abs(x - y) / np.abs(y))):.2e}")
        assert np.allclose(x, y, rtol=1e-8, atol=0), (tag, k)
        assert got[k].attrs == ref[k].attrs, (tag, k)


def _budget_for_128_rows(model, daily, window):
    """A byte budget under which ``window_panel_rows`` must pick 128 rows: one byte short of what 256 rows need."""
    from discontinuum_amd.rolling import record_windows

    Xnew, _times, lo, hi, out = record_windows(model, daily, window)
    m, q, reach = Xnew.shape[0], len(out), int((hi - lo).max())
    model._eval_ready(Xnew.to(model.device).contiguous())
    plan = model._plan
    budget = int(plan.lib.dgp_posterior_window_variances_workspace_bytes(plan._h, m, q, reach, 256)) - 1
    assert plan.window_panel_rows(m, q, reach, budget) == 128 and m > 256
    return budget


def test_loadest_rolling_mean_streamed_end_to_end(gpu_device):
    from discontinuum_amd.loadest_gp import LoadestGP
    from tests.flux_helpers import daily_loadest

    cov_obs, target, daily = daily_loadest(n_obs=60, start="2012-01-01", end="2013-02-04")
    assert len(daily.coords["time"].values) == 400
    model = LoadestGP()
    model.fit(cov_obs, target, iterations=10)
    budget = _budget_for_128_rows(model, daily, "30D")
    for statistic in (None, "mean"):
        dense = model.rolling_mean(daily, "30D", statistic=statistic)
        streamed = model.rolling_mean(daily, "30D", statistic=statistic, streamed=True, max_bytes=budget)
        _same_dataset(streamed, dense, f"loadest 30D {statistic}")
        assert np.all(streamed["n_points"].values == 30)
    with pytest.raises(ValueError, match="dense path"):
        model.rolling_mean(daily, "30D", streamed=True, return_cov=True)
    tau = float(np.median(model.rolling_mean(daily, "30D")["mean"].values))
    p_dense = model.exceedance_probability(daily, tau, window="30D")
    p_streamed = model.exceedance_probability(daily, tau, window="30D", streamed=True, max_bytes=budget)
    print("loadest exceedance_probability(window=30D): max difference", float(np.abs(p_streamed.values - p_dense.values).max()))
    assert np.allclose(p_streamed.values, p_dense.values, rtol=0, atol=1e-8) and p_streamed.attrs == p_dense.attrs
    assert np.array_equal(p_streamed.coords["time"].values, p_dense.coords["time"].values)
    assert float(p_dense.values.max()) > 0.5 > float(p_dense.values.min())  # the threshold is the median rolling mean


def test_censored_fit_takes_the_same_path(gpu_device):
    from discontinuum_amd.loadest_gp import LoadestGP
    from tests.flux_helpers import daily_loadest

    cov_obs, target, daily = daily_loadest(n_obs=60, start="2012-01-01", end="2013-02-04", seed=4)
    vals = np.asarray(target.values, dtype=np.float64)
    order = np.argsort(vals)
    mask = np.zeros(60, dtype=bool)
    mask[order[:12]] = True
    reported = vals.copy()
    reported[mask] = vals[order[12]]  # one detection limit: the 12 lowest samples are non-detects
    reported = type(target)(reported, dims=target.dims, coords=target.coords, name=target.name, attrs=target.attrs)
    model = LoadestGP()
    model.fit(cov_obs, reported, iterations=8, censored=mask)
    before = [a.values.copy() for a in model.predict(daily)]
    budget = _budget_for_128_rows(model, daily, "30D")
    _same_dataset(model.rolling_mean(daily, "30D", streamed=True, max_bytes=budget), model.rolling_mean(daily, "30D"), "censored 30D")
    after = [a.values for a in model.predict(daily)]
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_rating_seven_day_mean_flow_on_an_hourly_record(gpu_device):
    from discontinuum_amd.rating_gp import RatingGP
    from discontinuum_amd.xr_compat import DataArray, Dataset

    rng = np.random.default_rng(0)
    hours = np.datetime64("2012-01-01T00", "ns") + np.arange(400) * np.timedelta64(3600 * 10 ** 9, "ns")
    stage_all = 1.0 + 3.0 * rng.beta(2, 5, 400)
    pick = np.sort(rng.choice(400, 40, replace=False))
    flow = np.exp(1.6 * np.log(stage_all[pick]) + 0.05 * rng.standard_normal(40))
    cov_obs = Dataset({"stage": ("time", stage_all[pick])}, coords={"time": hours[pick]})
    target = DataArray(flow, dims=("time",), coords={"time": hours[pick]}, name="discharge", attrs={"units": "cfs"})
    unc = DataArray(np.full(40, 1.05), dims=("time",), coords={"time": hours[pick]}, name="discharge_unc")
    record = Dataset({"stage": ("time", stage_all)}, coords={"time": hours})
    model = RatingGP()
    model.fit(cov_obs, target, target_unc=unc, iterations=10)
    budget = _budget_for_128_rows(model, record, "7D")
    dense = model.rolling_mean(record, "7D")
    streamed = model.rolling_mean(record, "7D", streamed=True, max_bytes=budget)
    assert dense["mean"].values.shape == (400 - 167,) and np.all(dense["n_points"].values == 168)
    _same_dataset(streamed, dense, "rating 7D hourly")
