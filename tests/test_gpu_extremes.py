"""GPU tests of the orthant sweep (``dgp_orthant_probability``) and of ``extreme_probability`` / ``extreme_quantiles`` above it.

The reference is ``tests/extremes_helpers.orthant_ref``: the same estimator in numpy / scipy on the SAME generators and shifts,
so device and host walk the same points and differ by rounding only.  Tolerance of the parity tests (PARITY_RTOL): ten times
the worst relative difference measured over the cases of ``test_sweep_parity_on_identical_points`` on an MI355X
(EXPERIMENTS.md, "Orthant sweep"), and never more than 1e-9 -- perturbing L by one ulp moves the estimate by 4e-16 relative,
so anything near 1e-9 is a wrong tail branch, not rounding.
"""
import numpy as np
import pytest
import torch
from scipy.special import ndtr

from discontinuum_amd.backend import bvn_excess, orthant_level_chunks, orthant_probability, orthant_shifts, richtmyer_generators
from discontinuum_amd.exceedance import _output_groups
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.rolling import time_windows
from discontinuum_amd.xr_compat import Dataset
from tests.extremes_helpers import equicorrelated_factor, equicorrelated_truth, factor_layout, orthant_ref
from tests.flux_helpers import daily_loadest

pytestmark = pytest.mark.gpu

MEASURED_WORST = 3.625e-14  # the worst relative difference of test_sweep_parity_on_identical_points on an MI355X (EXPERIMENTS.md)
PARITY_RTOL = min(10 * MEASURED_WORST, 1e-9)
PARITY_ATOL = 1e-300  # an estimate that is exactly 0 on the host is exactly 0 on the device


def _parity(got, ref, scale=None):
    """|got - ref| <= PARITY_RTOL * scale (default |ref|).  The standard error is a root-mean-square DIFFERENCE of the shifts'
    estimates, so its rounding error is relative to the estimates, not to itself (measured at m = 2: the estimate agrees to one
    ulp, 1e-16, and the standard error of 1.8e-4 then differs by those 1e-16, 6e-13 of itself): it is held at the scale
    max(|prob|, |se|)."""
    return abs(got - ref) <= PARITY_RTOL * (abs(ref) if scale is None else scale) + PARITY_ATOL


def _wishart(m, seed):
    """A Wishart matrix whose condition number is about 200: m x 1.3 m normals (the Marchenko-Pastur edges give about 210),
    plus the ridge that caps it at 200."""
    rng = np.random.default_rng(seed)
    n = int(1.3 * m) + 2
    A = rng.standard_normal((m, n))
    C = A @ A.T / n
    ev = np.linalg.eigvalsh(C)
    ridge = max((ev[-1] - 200.0 * ev[0]) / 199.0, 0.0)
    return C + ridge * np.eye(m)


def _ar1(m, rho=0.9):
    t = np.arange(m)
    return rho ** np.abs(t[:, None] - t[None, :])


def _levels(C, kind, seed):
    """Three levels of centred limits for a covariance ``C``, per ``kind``."""
    m = C.shape[0]
    sd = np.sqrt(np.diag(C))
    rng = np.random.default_rng(seed)
    inf = np.full(m, np.inf)
    wob = 1.0 + 0.2 * rng.random(m)
    if kind == "one-sided":
        return np.stack([-inf, 0.5 * sd * wob, -inf]), np.stack([1.5 * sd * wob, inf, 2.5 * sd])
    if kind == "two-sided":
        return np.stack([-1.5 * sd * wob, 0.2 * sd, -inf]), np.stack([2.0 * sd, 3.0 * sd * wob, inf])  # (level 2: all-infinite)
    lo, hi = np.stack([-inf, -inf, -2.0 * sd]), np.stack([40.0 * sd, -40.0 * sd, 2.0 * sd])  # level 1: 40 sigma out
    lo[2, m // 2], hi[2, m // 2] = 1.0, -1.0  # level 2: lo > hi somewhere
    return lo, hi


def _rel(got, ref):
    return abs(got - ref) / max(abs(ref), 1e-300) if ref != 0 else abs(got)


@pytest.fixture(scope="module")
def parity_cases():
    """(tag, (M, M) poisoned factor, m, lo, hi, gen, shifts, npoints, reference (prob, se) per level) -- computed once."""
    cases = []
    for m in (1, 2, 127, 128, 129, 300):
        for name, C in (("wishart", _wishart(m, m)), ("ar1", _ar1(m))):
            Lm = np.linalg.cholesky(C)
            for kind, npoints in (("one-sided", 200), ("two-sided", 256), ("degenerate", 200)):
                lo, hi = _levels(C, kind, m)
                gen, shifts = richtmyer_generators(m), orthant_shifts(m, 4, seed=m).numpy()
                ref = [orthant_ref(Lm, lo[l], hi[l], gen, shifts, npoints) for l in range(3)]
                cases.append((f"{name}-m{m}-{kind}-N{npoints}", factor_layout(Lm), m, lo, hi, npoints, ref))
    return cases


def test_sweep_parity_on_identical_points(gpu_device, parity_cases):
    dev = gpu_device
    worst = (0.0, "")
    for tag, Lbuf, m, lo, hi, npoints, ref in parity_cases:
        Ld = torch.tensor(Lbuf, dtype=torch.float64, device=dev)
        prob, se = orthant_probability(Ld, m, lo, hi, npoints=npoints, nshifts=4, seed=m)
        prob2, se2 = orthant_probability(Ld, m, lo, hi, npoints=npoints, nshifts=4, seed=m)
        assert torch.equal(prob, prob2) and torch.equal(se, se2), tag  # bitwise repeatable
        prob, se = prob.cpu().numpy(), se.cpu().numpy()
        assert np.all(np.isfinite(prob)) and np.all(np.isfinite(se)), (tag, prob, se)
        for l in range(3):
            scale = max(abs(ref[l][0]), abs(ref[l][1]))
            rp, rs = _rel(prob[l], ref[l][0]), (abs(se[l] - ref[l][1]) / scale if scale else abs(se[l]))
            print(f"{tag} level {l}: prob {prob[l]:.12g} (rel {rp:.2e}) se {se[l]:.3e} (diff / scale {rs:.2e})")
            worst = max(worst, (rp, f"{tag} level {l} prob"), (rs, f"{tag} level {l} se"))
            assert _parity(prob[l], ref[l][0]), (tag, l, prob[l], ref[l][0])
            assert _parity(se[l], ref[l][1], scale), (tag, l, se[l], ref[l][1])
        if "two-sided" in tag:
            assert prob[2] == 1.0 and se[2] == 0.0, tag  # an unconstrained level: exactly 1, error 0
        if "degenerate" in tag:
            assert prob[1] == 0.0 and se[1] == 0.0 and prob[2] == 0.0 and se[2] == 0.0, tag  # impossible levels
    print(f"worst relative difference: {worst[0]:.3e} ({worst[1]})")
    # one level per call under a byte budget: the same shifts, the same numbers, bit for bit
    tag, Lbuf, m, lo, hi, npoints, ref = next(c for c in parity_cases if c[0].startswith("wishart-m300-one-sided"))
    Ld = torch.tensor(Lbuf, dtype=torch.float64, device=dev)
    per_call, one = orthant_level_chunks(m, 3, 4, npoints, max_bytes=None)
    assert per_call == 3 and orthant_level_chunks(m, 3, 4, npoints, max_bytes=one)[0] == 1
    whole = orthant_probability(Ld, m, lo, hi, npoints=npoints, nshifts=4, seed=m)
    split = orthant_probability(Ld, m, lo, hi, npoints=npoints, nshifts=4, seed=m, max_bytes=one)
    assert torch.equal(whole[0], split[0]) and torch.equal(whole[1], split[1])
    with pytest.raises(ValueError, match="bytes for ONE level"):
        orthant_probability(Ld, m, lo, hi, npoints=npoints, nshifts=4, seed=m, max_bytes=one - 1)


def test_closed_forms_on_the_device(gpu_device):
    dev = gpu_device
    # 1. diagonal L: the integrand is constant
    m = 200
    sig = np.linspace(0.5, 2.0, m)
    Ld = torch.tensor(factor_layout(np.diag(sig)), dtype=torch.float64, device=dev)
    prob, se = orthant_probability(Ld, m, np.full(m, -np.inf), np.full(m, 3.0), npoints=256, nshifts=8)
    truth = np.prod(ndtr(3.0 / sig))
    print(f"diagonal: {prob.item():.16g} vs {truth:.16g}, se {se.item():.2e}")
    assert abs(prob.item() - truth) <= 1e-13 and se.item() <= 1e-15
    # 2. equicorrelated blocks against the one-dimensional quadrature
    for m, rho, b in ((300, 0.5, 2.5), (130, 0.9, 1.0)):
        Lm = equicorrelated_factor(m, rho)
        truth = equicorrelated_truth(m, rho, b)
        lo, hi = np.full(m, -np.inf), np.full(m, b)
        prob, se = orthant_probability(torch.tensor(factor_layout(Lm), dtype=torch.float64, device=dev), m, lo, hi, npoints=2048,
                                       nshifts=8, seed=0)
        rp, rs = orthant_ref(Lm, lo, hi, richtmyer_generators(m), orthant_shifts(m, 8, 0).numpy(), 2048)
        print(f"equicorrelated m={m} rho={rho} b={b}: {prob.item():.6f} +- {se.item():.1e} (host {rp:.6f} +- {rs:.1e}), truth {truth:.6f}")
        assert abs(prob.item() - truth) <= 4 * se.item() and se.item() <= 3e-3 and se.item() <= 2 * rs
    # m = 2 against Phi2 = D(h, k, rho) + Phi(h) Phi(k) from the pair function of the exceedance counts
    for rho, h, k in ((0.6, 0.3, -0.4), (-0.8, 1.2, 0.5), (0.95, -0.5, 0.1)):
        Lm = np.linalg.cholesky(np.array([[1.0, rho], [rho, 1.0]]))
        dv = lambda a: torch.tensor([a], dtype=torch.float64, device=dev)  # noqa: E731
        phi2 = bvn_excess(dv(h), dv(k), dv(rho)).item() + ndtr(h) * ndtr(k)
        prob, se = orthant_probability(torch.tensor(factor_layout(Lm), dtype=torch.float64, device=dev), 2, np.full(2, -np.inf),
                                       np.array([h, k]), npoints=2048, nshifts=8, seed=0)
        print(f"bivariate rho={rho}: {prob.item():.8f} +- {se.item():.1e} vs Phi2 {phi2:.8f}")
        assert abs(prob.item() - phi2) <= 4 * se.item() and se.item() <= 1e-3


# ------------------------------------------------------------------------------------------------ from a fitted model
class LoadestGP32(LoadestGP):
    dtype = torch.float32


def _record(seed=21):
    """160 samples over two years and a 300-day record across the turn of the year (150 + 150 days: two periods), with excluded
    points -- a missing time stamp -- at the head, in the middle and at the tail, where tests/test_gpu_exceedance.py::_groups
    places them."""
    cov_obs, target, daily = daily_loadest(n_obs=160, start="2012-01-01", end="2014-01-01", seed=seed)
    t = daily.coords["time"].values
    first = int(np.searchsorted(t, np.datetime64("2013-01-01"))) - 150
    time = t[first:first + 300].copy()
    flow = np.asarray(daily["flow"].values)[first:first + 300]
    for k in (0, 1, 150, 299):
        time[k] = np.datetime64("NaT")
    rec = Dataset({"flow": ("time", flow, {"units": "cubic meters per second"})}, coords={"time": time})
    return cov_obs, target, rec


def _capture(model):
    """The plan-level hook: every ``orthant_probability`` call's device inputs, copied (the factor buffer is reused)."""
    calls = []
    model._plan._orthant_hook = lambda d: calls.append({k: (v.detach().clone().cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    return calls


def _restate(call):
    m = call["m"]
    Lm = np.tril(call["L"][:m, :m])
    return Lm, np.array([orthant_ref(Lm, call["lo"][l], call["hi"][l], call["gen"], call["shifts"], call["npoints"])
                         for l in range(call["lo"].shape[0])])


@pytest.fixture(scope="module", params=[torch.float64, torch.float32], ids=["fp64", "fp32"])
def fitted(request, gpu_device):
    cov_obs, target, rec = _record()
    model = (LoadestGP if request.param == torch.float64 else LoadestGP32)()
    model.fit(cov_obs, target, iterations=5)
    return model, rec, target


KW = dict(npoints=512, nshifts=8, seed=3)


def test_extreme_probability_from_a_fitted_plan(fitted):
    """Three levels in the interior of the peak's distribution.  (The bounds below compare with the REPORTED error, which the
    same points estimate: a level whose probability lies within about 1 / (npoints x nshifts) of 1 is not resolved by the rule
    -- at the 98 % quantile of the samples every point returns 1 - 1e-16 with an error of 8e-17 while min_i Phi_i = 1 - 6e-10,
    on the device and in the restatement alike; DESIGN.md says so.)"""
    model, rec, target = fitted
    levels = np.quantile(np.asarray(target.values), [0.65, 0.75, 0.85])
    calls = _capture(model)
    ds = model.extreme_probability(rec, threshold=levels, **KW)
    never, anyp, err = ds["prob_never"].values, ds["prob_any"].values, ds["error"].values
    assert never.shape == (3, 2) and list(ds["n_points"].values) == [148, 148] and len(calls) == 2
    assert ds.attrs["npoints"] == 512 and ds.attrs["nshifts"] == 8 and ds.attrs["seed"] == 3 and ds.attrs["jitter"] >= 0.0
    assert np.all((never >= 0) & (never <= 1)) and np.allclose(anyp, 1 - never) and np.all(np.isfinite(err))
    for g, call in enumerate(calls):  # the product against the restatement on the device's OWN factor and centred limits
        assert call["m"] == 148 and call["L"].dtype == np.float64 and np.all(np.isneginf(call["lo"]))
        Lm, ref = _restate(call)
        sd = np.sqrt(np.sum(Lm * Lm, axis=1))
        for l in range(3):
            print(f"{model.dtype} period {g} level {l}: {never[l, g]:.10f} +- {err[l, g]:.1e} (host {ref[l, 0]:.10f} +- {ref[l, 1]:.1e})")
            assert _parity(never[l, g], ref[l, 0]) and _parity(err[l, g], ref[l, 1], max(ref[l]))
            marg = ndtr(call["hi"][l] / sd)
            assert marg.min() + 4 * err[l, g] >= never[l, g] >= 1 - np.sum(1 - marg) - 4 * err[l, g]
        for l in range(2):  # non-decreasing along the levels
            assert never[l + 1, g] - never[l, g] >= -4 * np.hypot(err[l, g], err[l + 1, g])
    model._plan._orthant_hook = None
    days = model.exceedance(rec, threshold=levels)["mean"].values  # P(N >= 1) <= E[N]
    assert np.all(anyp <= days + 4 * err)

    # kind="min" at a level equals kind="max" of the negated problem, built by hand at plan level (other points: within errors)
    calls = _capture(model)
    # (levels just under the lowest predicted value of the record: interior probabilities for the period that runs low)
    ok = ~np.isnat(rec.coords["time"].values)
    clean = Dataset({"flow": ("time", np.asarray(rec["flow"].values)[ok], {"units": "cubic meters per second"})},
                    coords={"time": rec.coords["time"].values[ok]})
    low = float(np.min(np.asarray(model.predict(clean)[0].values, dtype=np.float64))) * np.array([0.85, 0.97])
    dmin = model.extreme_probability(rec, threshold=low, kind="min", **KW)
    assert len(calls) == 2 and np.all(np.isposinf(calls[0]["hi"]))
    for g, call in enumerate(list(calls)):
        Lm, ref = _restate(call)
        Ld = torch.tensor(call["L"], device=model._plan.device)
        p, e = model._plan.orthant_probability(Ld, call["m"], np.full_like(call["lo"], -np.inf), -call["lo"], **KW)
        for l in range(2):
            assert _parity(dmin["prob_never"].values[l, g], ref[l, 0])
            assert abs(dmin["prob_never"].values[l, g] - p[l].item()) <= 4 * np.hypot(dmin["error"].values[l, g], e[l].item()) + 1e-12
    assert len(calls) == 4  # (the hand-built calls went through the same hook)

    # a window of 7 points: the restatement on the window_moments buffer's block.  One threshold per day, 1.08 and 1.15 times
    # the day's own predicted value, so that BOTH periods get interior probabilities (the two periods of this record run at
    # different levels: at a common level one of them holds a probability of 1.4e-267 -- a product of 140 factors deep in the
    # tail, whose relative rounding grows like 2 ln(1 / p) ulps of the arguments; measured there on the float32 plan: 6.5e-13
    # relative, outside the bound that the estimates of test 6 set, and no statement about a usable probability)
    calls.clear()
    seen = []
    wm = model._plan.window_moments
    model._plan.window_moments = lambda *a, **k: seen.append(wm(*a, **k)) or seen[-1]
    pred = np.ones(300)
    pred[ok] = np.asarray(model.predict(clean)[0].values, dtype=np.float64)
    try:
        dw = model.extreme_probability(rec, threshold_series=np.stack([1.08 * pred, 1.15 * pred]), window="7D", **KW)
    finally:
        del model._plan.window_moments
        model._plan._orthant_hook = None
    (wmean, S), = seen
    S = S.cpu().numpy()
    n_pts = list(dw["n_points"].values)
    assert len(calls) == 2 and [c["m"] for c in calls] == n_pts and sum(n_pts) < 296 - 6
    order, _lo, _hi, keep = time_windows(rec.coords["time"].values, "7D")
    groups = _output_groups(rec.coords["time"].values[order], keep, "YE")[0]
    Sfull = np.tril(S) + np.tril(S, -1).T
    for g, call in enumerate(calls):
        Lm, ref = _restate(call)
        for l in range(2):
            print(f"{model.dtype} window period {g} level {l}: {dw['prob_never'].values[l, g]:.10g} (host {ref[l, 0]:.10g})")
            assert _parity(dw["prob_never"].values[l, g], ref[l, 0]) and _parity(dw["error"].values[l, g], ref[l, 1], max(ref[l]))
        # the factor is the factor of the period's block of S = W C W^T (plus the jitter the attrs report)
        idx = np.nonzero(groups == g)[0]
        block = Sfull[np.ix_(idx, idx)]
        assert np.abs(Lm @ Lm.T - block).max() <= 1e-10 * np.abs(block).max() + 1.01 * dw.attrs["jitter"]


def test_extreme_quantiles_from_a_fitted_plan(fitted):
    model, rec, _target = fitted
    q = np.array([0.1, 0.5, 0.9])
    dq = model.extreme_quantiles(rec, q=q, **KW)
    value, mass, err = dq["value"].values, dq["bracket_prob"].values, dq["error"].values
    assert value.shape == (3, 2) and np.all(np.isfinite(value)) and np.all(dq["bracket"].values > 0)
    assert np.all(np.diff(value, axis=0) > 0)  # increasing in q
    series = np.repeat(value[:, :1], 300, axis=1)
    t = rec.coords["time"].values
    series[:, t >= np.datetime64("2013-01-01")] = value[:, 1:2]  # every point gets its own period's value
    back = model.extreme_probability(rec, threshold_series=series, **KW)
    F, e2 = back["prob_never"].values, back["error"].values
    print("quantiles:", value.T, "re-evaluated:", F.T, "bracket mass:", mass.T)
    assert np.all(np.abs(F - q[:, None]) <= 4 * np.maximum(err, e2) + mass)


def test_censored_fit_takes_the_same_path(gpu_device):
    """A fit with non-detects (the Laplace posterior) runs through the same call without a special case."""
    cov_obs, target, rec = _record(seed=22)
    vals = np.asarray(target.values, dtype=np.float64)
    order = np.argsort(vals)
    mask = np.zeros(160, dtype=bool)
    mask[order[:24]] = True
    reported = vals.copy()
    reported[mask] = vals[order[24]]
    reported = type(target)(reported, dims=target.dims, coords=target.coords, name=target.name, attrs=target.attrs)
    model = LoadestGP()
    model.fit(cov_obs, reported, iterations=5, censored=mask)
    calls = _capture(model)
    ds = model.extreme_probability(rec, threshold=np.quantile(vals, [0.8, 0.95]), **KW)
    model._plan._orthant_hook = None
    never, err = ds["prob_never"].values, ds["error"].values
    assert np.all((never >= 0) & (never <= 1)) and np.all(np.isfinite(err)) and len(calls) == 2
    for g, call in enumerate(calls):
        _Lm, ref = _restate(call)
        for l in range(2):
            assert _parity(never[l, g], ref[l, 0]) and _parity(err[l, g], ref[l, 1], max(ref[l]))
