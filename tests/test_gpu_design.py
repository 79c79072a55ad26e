"""GPU parity of ``dgp_sample_value`` (the exact value of one more sample for the period sums' variance) and of the API above
it: ``design_value``, the greedy ``design``, ``LoadestGP`` / ``RatingGP`` methods.

References (tests/design_helpers.py, numpy): the DIRECT double sum sum_{i,j in p} A_i A_j expm1(s^2 b_ic b_jc) -- never the
series -- on the SAME ``dgp_posterior_cov`` buffer, symmetrised from its lower triangle, with the conditioning done by a
DENSE SOLVE C[:, S] (C_SS + D)^-1 C[S, :] -- never the recurrence.  float32 buffers are compared with the same reference on
the float32 values cast to double: the arithmetic after the loads is double.

Bound of a gain entry: 1e-12 (sum_{i in p} |A_i|)^2 max(1, expm1(beta)), beta = s^2 max C_ii over the included days -- the
pairwise term is at most A_i A_j expm1(beta); the series' rounding is about (beta + a few) eps of it, plus the 2^-53
truncation rule, times ten for summation order, summed over the pairs.  The hypothetical samples' noise is of the size of
the largest posterior variance, so that C_SS + D is well conditioned (below about 130) and the dense solve and the rows given
to the kernel describe the same covariance to 1e-14.  Worst ratios measured on MI355X: see DESIGN.md section 7.
"""
import numpy as np
import pytest
import torch

from discontinuum_amd.backend import sample_value, series_terms
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.loads import target_transform
from discontinuum_amd.rating_gp import RatingGP
from discontinuum_amd.xr_compat import Dataset
from tests.design_helpers import design_value_ref, direct_gain, greedy_ref, linear_gain, rows_by_cholesky
from tests.flux_helpers import daily_loadest, daily_rating, symmetrise_lower
from tests.test_gpu_exceedance import _groups, _posterior_buffers

pytestmark = pytest.mark.gpu

MS = (1, 2, 63, 65, 127, 129, 300)
NROWS = (0, 1, 5, 64)


def _ratio(got, ref, a, g, P, beta):
    """max |got - ref| / bound over the entries; an empty group must hold exact zeros."""
    SA = np.bincount(g[g >= 0], weights=np.abs(a)[g >= 0], minlength=P)
    tol = 1e-12 * SA ** 2 * max(1.0, np.expm1(beta))
    assert np.all(got[SA == 0] == 0)
    live = SA > 0
    return float((np.abs(got - ref)[live] / tol[live, None]).max()) if live.any() else 0.0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("model", ["loadest", "rating"])
def test_gain_map_matches_the_direct_sum(model, dtype, gpu_device):
    dev = gpu_device
    bufs = _posterior_buffers(model, dev, dtype, MS)
    rng = np.random.default_rng(11)
    worst = {"series": 0.0, "K=64": 0.0, "K=1": 0.0, "var": 0.0}
    dv = lambda x, dt=torch.float64: None if x is None else torch.tensor(x, dtype=dt, device=dev)  # noqa: E731
    for im, m in enumerate(MS):
        cov = bufs[m][0].clone()
        if m >= 127:  # a zero-variance point: its row and column of the lower triangle, and the diagonal
            cov[40, :41] = 0
            cov[40:, 40] = 0
        Cs = symmetrise_lower(cov[:m, :m].double()).cpu().numpy()
        diag = np.diagonal(Cs)
        a = rng.uniform(0.5, 2.0, m)
        if m > 4:
            a[3] = 0.0
        ov_t = torch.tensor(rng.uniform(0.5, 2.0, m) * diag.max(), dtype=dtype, device=dev)
        if m >= 127:
            ov_t[40] = 0
        ov = ov_t.double().cpu().numpy()
        # P = 700 at m = 300: enough workgroups without slabs -- the path a 31-year record takes
        for ip, P in enumerate((1, 3, 40, 700) if m == 300 else (1, 3, 40)):
            g = _groups(m, P)
            top = diag[g >= 0].max() if (g >= 0).any() else diag.max()
            beta = (1.65, 0.5)[(im + ip) % 2]
            s2 = beta / top
            K = series_terms(beta)
            nrows = NROWS[(im + ip) % 4]
            for tau2, tau2_t, nr in ((None, None, 0), (ov, ov_t, nrows)):
                pool = np.setdiff1d(np.arange(m), [40]) if m >= 127 else np.arange(m)
                S = rng.choice(pool, nr, replace=nr > len(pool)) if nr else np.zeros(0, dtype=np.int64)
                B = rows_by_cholesky(Cs, S, tau2) if nr else None
                ref, _vref = direct_gain(Cs, a, s2, g, P, tau2, S)
                lin = linear_gain(Cs, a, s2, g, P, tau2, S)
                tag = (model, dtype, m, P, nr, tau2 is not None)
                for name, nt, want in (("series", K, ref), ("K=64", 64, ref), ("K=1", 1, lin)):
                    gain, var = sample_value(cov, m, dv(a), s2, dv(g, torch.int32), P, obs_var=tau2_t, rows=dv(B), nterms=nt)
                    gain, var = gain.cpu().numpy(), var.cpu().numpy()
                    r = _ratio(gain, want, a, g, P, beta)
                    assert r <= 1.0, (tag, name, r)
                    worst[name] = max(worst[name], r)
                    vwant = diag - (0.0 if B is None else (B ** 2).sum(axis=0)) + (0.0 if tau2 is None else tau2)
                    verr = float(np.abs(var - np.clip(vwant, 0.0, None)).max() / (1e-14 * (diag + (0.0 if tau2 is None else tau2)).max()))
                    assert verr <= 1.0, (tag, name, "var", verr)
                    worst["var"] = max(worst["var"], verr)
                    if m >= 127:
                        assert np.all(gain[:, 40] == 0) and var[40] == 0, tag
                    assert np.all(np.isfinite(gain)) and np.all(gain >= 0), tag
    print(f"{model} {dtype}: worst error / bound: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


def test_repeatable_and_batch_independent(gpu_device):
    dev = gpu_device
    m = 300
    bufs = [_posterior_buffers("loadest", dev, torch.float64, (m,), seed=s)[m][0].clone() for s in (3, 4, 5)]
    M = bufs[0].shape[0]
    upper = torch.triu(torch.ones(M, M, dtype=torch.bool, device=dev), 1)
    for cov, junk in zip(bufs, (float("nan"), 1e30, None)):  # only the lower triangle of the first m rows is ever USED (the rest is loaded in bounds and dropped)
        if junk is not None:
            cov[upper] = junk
            cov[m:, :] = junk
    rng = np.random.default_rng(2)
    a = torch.tensor(rng.uniform(0.5, 2.0, (3, m)), device=dev)
    ov = torch.tensor(rng.uniform(0.01, 0.05, (3, m)), device=dev)
    cov3 = torch.stack(bufs).contiguous()
    tops = torch.stack([torch.diagonal(c)[:m].max() for c in bufs])
    s2 = (1.65 / tops).cpu()
    for P, nr in ((3, 5), (700, 0)):  # slabs and partial sums in the work area; one slab per group
        g = torch.tensor(np.stack([_groups(m, P)] * 3), dtype=torch.int32, device=dev)
        rows = torch.tensor(rng.normal(0.0, 0.02, (3, nr, m)), device=dev) if nr else None
        gain_a, var_a = sample_value(cov3, m, a, s2, g, P, obs_var=ov, rows=rows, nterms=21)
        gain_b, var_b = sample_value(cov3, m, a, s2, g, P, obs_var=ov, rows=rows, nterms=21)
        assert torch.equal(gain_a, gain_b) and torch.equal(var_a, var_b)
        assert gain_a.shape == (3, P, m) and torch.isfinite(gain_a).all() and torch.isfinite(var_a).all()
        for b in range(3):
            gain1, var1 = sample_value(bufs[b], m, a[b], float(s2[b]), g[b], P, obs_var=ov[b], rows=None if rows is None else rows[b],
                                       nterms=21)
            assert torch.equal(gain_a[b], gain1) and torch.equal(var_a[b], var1), (P, b)
    # NaN in, NaN out: a NaN variance poisons its own candidate, in every group with days, and no other
    bad = bufs[2].clone()
    bad[17, 17] = float("nan")
    g = torch.tensor(_groups(m, 3), dtype=torch.int32, device=dev)
    gain, var = sample_value(bad, m, a[2], float(s2[2]), g, 3, nterms=21)
    assert torch.isnan(var[17]) and torch.isnan(gain[[0, 2], 17]).all() and torch.isfinite(var[:17]).all()  # (group 1 is empty)
    assert torch.isfinite(gain[:, :17]).all() and torch.isfinite(gain[:, 18:]).all()


# ------------------------------------------------------------------------------------------------ the product layer
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


def _record(model):
    """Make the model's plan keep the arguments of its ``period_moments`` calls."""
    calls, real = [], model._plan.period_moments

    def spy(cov, m, mu, scale2, w, groups, ngroups, mode, extra_var=None):
        calls.append((cov, m, mu, scale2, w, groups, ngroups, mode))
        return real(cov, m, mu, scale2, w, groups, ngroups, mode, extra_var=extra_var)

    model._plan.period_moments = spy
    return calls


def _device_posterior(model, daily, freq):
    """(C symmetric, A_i, s^2, groups, P, Var(L_p)) as the device formed them for ``daily``'s loads."""
    calls = _record(model)
    try:
        flux, pcov = model.annual_flux(daily, freq=freq, return_cov=True)
    finally:
        del model._plan.period_moments
    cov, m, mapped, s2, w, groups, P, _mode = calls[-1]
    Cs = symmetrise_lower(cov[:m, :m].double()).cpu().numpy()
    a = np.asarray(w) * np.exp(mapped.double().cpu().numpy() + 0.5 * s2 * np.diagonal(Cs))
    return Cs, a, s2, np.asarray(groups), P, np.diagonal(pcov).copy(), flux


def test_law_of_total_variance_on_the_device(gpu_device):
    """``design_value`` for nested designs of 1, 4 and 12 samples: V(S) matches the dense reference within
    ``period_moments``' own bound (1e-11 of the largest entry), grows along the prefixes and stays below Var(L_p)."""
    model, daily = _loadest(425, 80, 21)
    Cs, a, s2, groups, P, var_now, _flux = _device_posterior(model, daily, "YE")
    assert P == 2
    S = np.random.default_rng(1).choice(len(a), 12, replace=False)
    tau2 = 0.02
    prev = np.zeros(P)
    for k in (1, 4, 12):
        ds, V = model.design_value(daily, S[:k], sample_var=tau2, return_cov=True)
        ref = design_value_ref(Cs, a, s2, groups, P, S[:k], np.full(len(a), tau2))
        err = float(np.abs(V - ref).max() / np.abs(ref).max())
        print(f"|S| = {k}: max |V - ref| / max |ref| = {err:.3e}")
        assert err <= 1e-11
        ve = ds["variance_explained"].values
        assert np.all(ve >= prev) and np.all(ve <= var_now) and np.all(ve > 0)
        assert np.allclose(ds["se_expected"].values, np.sqrt(var_now - ve), rtol=1e-12, atol=0)
        prev = ve


def test_greedy_picks_match_a_numpy_greedy_on_the_same_buffer(gpu_device):
    model, daily = _loadest(129, 40, 22)
    Cs, a, s2, groups, P, var_now, _flux = _device_posterior(model, daily, "ME")
    m = len(a)
    assert m == 129 and P == 5
    time = daily.coords["time"].values
    tau2 = np.full(m, 0.02)
    runs = {}
    for objective, omega in (("relative", 1.0 / var_now), ("absolute", np.ones(P))):
        picks, tops = greedy_ref(Cs, a, s2, groups, P, 6, omega, tau2)
        gaps = [(best - second) / best for best, second in tops]
        print(f"{objective}: picks {picks}, smallest relative gap of the top two scores {min(gaps):.3e}")
        assert min(gaps) > 1e-9  # the reference itself separates every choice
        ds = model.design(daily, 6, objective=objective, freq="ME", sample_var=0.02)
        assert ds["index"].values.tolist() == picks and np.array_equal(ds["time"].values, time[picks])
        assert len(set(ds["index"].values.tolist())) == 6  # replicates=False never repeats a day
        assert np.allclose(ds["score"].values, [best for best, _s in tops], rtol=1e-8, atol=0)
        for j in (0, 5):
            ref = np.diagonal(design_value_ref(Cs, a, s2, groups, P, picks[: j + 1], tau2))
            assert np.all(np.abs(ds["variance_explained"].values[j] - ref) <= 1e-11 * ref.max())
        runs[objective] = ds
    full = runs["relative"]
    cont = model.design(daily, 3, given=time[full["index"].values[:3]], freq="ME", sample_var=0.02)
    assert cont["index"].values.tolist() == full["index"].values[3:].tolist()
    assert np.allclose(cont["variance_explained"].values, full["variance_explained"].values[3:], rtol=1e-10, atol=0)


def test_model_level_methods(gpu_device):
    model, daily = _loadest(425, 80, 21)
    flux = model.annual_flux(daily)
    sv = model.sample_value(daily)
    m = len(daily.coords["time"].values)
    assert sv["variance_reduction"].values.shape == (2, m) and np.array_equal(sv["se_now"].values, flux["se"].values)
    var = flux["se"].values ** 2
    gain = sv["variance_reduction"].values
    assert np.all(gain >= 0) and np.all(gain <= var[:, None] * (1 + 1e-9)) and np.all(np.isfinite(sv["score"].values))
    best = int(np.argmax(sv["score"].values))
    one = model.design_value(daily, [best])
    assert np.allclose(one["variance_explained"].values, gain[:, best], rtol=1e-9, atol=1e-12 * var.max())
    assert np.array_equal(one["se_now"].values, flux["se"].values)
    picked = model.design(daily, 2)
    assert int(picked["index"].values[0]) == best and np.all(picked["se_expected"].values <= flux["se"].values[None, :])
    # every day of a short, well-separated record sampled exactly: nothing is left to learn
    days = np.arange(5) * 80
    five = Dataset({"flow": ("time", np.asarray(daily["flow"].values)[days], {"units": "cubic meters per second"})},
                   coords={"time": daily.coords["time"].values[days]})
    now = model.annual_flux(five)["se"].values ** 2
    left = model.design_value(five, np.arange(5), sample_var=0.0)["se_expected"].values ** 2
    print("five exact samples: remaining / original variance =", (left / now).tolist())
    assert np.all(left <= 1e-8 * now)

    cov_obs, target, unc, rdaily = daily_rating(n_obs=60, end="2013-01-01", seed=12)
    rating = RatingGP()
    rating.fit(cov_obs, target, target_unc=unc, iterations=5)
    volume = np.full(len(rdaily.coords["time"].values), 86400.0)  # runoff volume per day of discharge
    agg = rating.aggregate(rdaily, volume)
    rsv = rating.sample_value(rdaily, volume)
    assert np.array_equal(rsv["se_now"].values, agg["se"].values) and np.all(rsv["variance_reduction"].values >= 0)
    rbest = int(np.argmax(rsv["score"].values))
    rds = rating.design(rdaily, volume, 3)
    rval = rating.design_value(rdaily, volume, rds["time"].values)
    assert int(rds["index"].values[0]) == rbest
    assert np.allclose(rval["variance_explained"].values, rds["variance_explained"].values[-1], rtol=1e-9, atol=0)
    _mode, s, _t = target_transform(rating.dm)
    assert s > 0 and np.all(rval["fraction"].values > 0) and np.all(rval["fraction"].values < 1)
