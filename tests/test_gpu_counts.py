"""GPU tests of the path-count sweep (``dgp_path_counts``) and of ``exceedance_distribution`` / ``compliance_probability`` above it.

The reference is ``tests/count_helpers.counts_ref``: the same estimator in numpy / scipy on the SAME generators and shifts.  The
device returns integers, so there is no tolerance: the histograms must equal the restatement's, integer for integer, whenever
no path lies within rounding of a threshold.  That condition is asserted FIRST, on the inputs, from the restatement: the
smallest gap min |f_i - c_i| / sd_i over all paths is at least GAP_MIN = 1e-9, against a rounding of the paths of about 1e-13
(an m-term fp64 sum in another order, and Phi^-1 from another library).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from discontinuum_amd import frequency as F
from discontinuum_amd.backend import orthant_shifts, path_count_level_chunks, path_counts, richtmyer_generators
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.xr_compat import Dataset
from tests.count_helpers import counts_ref, make_count_oracle_plan
from tests.extremes_helpers import factor_layout
from tests.flux_helpers import daily_loadest

pytestmark = pytest.mark.gpu

GAP_MIN = 1e-9


def _wishart(m, seed):
    """The Wishart matrix of tests/test_gpu_extremes.py: condition number capped at 200."""
    rng = np.random.default_rng(seed)
    n = int(1.3 * m) + 2
    A = rng.standard_normal((m, n))
    Cm = A @ A.T / n
    ev = np.linalg.eigvalsh(Cm)
    return Cm + max((ev[-1] - 200.0 * ev[0]) / 199.0, 0.0) * np.eye(m)


def _ar1(m, rho=0.9):
    t = np.arange(m)
    return rho ** np.abs(t[:, None] - t[None, :])


def _levels(Cm, seed):
    sd = np.sqrt(np.diag(Cm))
    wob = 1.0 + 0.2 * np.random.default_rng(seed).random(Cm.shape[0])
    return np.stack([-0.5 * sd * wob, 0.5 * sd, 1.5 * sd * wob])


def _link(m):
    link = np.ones(m, dtype=np.int32)
    link[[int(0.3 * m), int(0.7 * m)]] = 0
    return link


@pytest.fixture(scope="module")
def parity_cases():
    """(tag, poisoned factor, m, thr, above, link, npoints, reference histograms, smallest gap) -- computed once."""
    cases = []
    for m in (1, 2, 63, 64, 65, 129, 257):
        gen, shifts = richtmyer_generators(m), orthant_shifts(m, 4, seed=m).numpy()
        for name, Cm in (("wishart", _wishart(m, m)), ("ar1", _ar1(m))):
            Lm = np.linalg.cholesky(Cm)
            thr = _levels(Cm, m)
            for above in (True, False):
                for npoints in (200, 256):
                    link = _link(m) if npoints == 200 else None
                    ref = counts_ref(Lm, thr, above, link, gen, shifts, npoints)
                    cases.append((f"{name}-m{m}-{'above' if above else 'below'}-N{npoints}", factor_layout(Lm), m, thr, above, link,
                                  npoints, ref))
    return cases


def test_sweep_parity_on_identical_points(gpu_device, parity_cases):
    """Both histograms equal the restatement's integer for integer (no tolerance), a second call is identical, every row sums to
    npoints; the factor is poisoned with NaN above the block diagonal, and in a second buffer also in every row >= m."""
    dev = gpu_device
    worst = min((ref[2], tag) for tag, *_rest, ref in parity_cases)
    print(f"smallest gap over the cases: {worst[0]:.3e} ({worst[1]})")
    for tag, Lbuf, m, thr, above, link, npoints, ref in parity_cases:
        assert ref[2] >= GAP_MIN, (tag, ref[2])  # the condition on the inputs
        Ld = torch.tensor(Lbuf, dtype=torch.float64, device=dev)
        kw = dict(above=above, link=link, npoints=npoints, nshifts=4, seed=m)
        ch, sh = path_counts(Ld, m, thr, **kw)
        ch2, sh2 = path_counts(Ld, m, thr, **kw)
        assert ch.dtype == torch.int32 and tuple(ch.shape) == (3, 4, m + 1) == tuple(sh.shape), tag
        assert torch.equal(ch, ch2) and torch.equal(sh, sh2), tag
        ch, sh = ch.cpu().numpy(), sh.cpu().numpy()
        assert np.all(ch.sum(axis=2) == npoints) and np.all(sh.sum(axis=2) == npoints), tag
        assert np.array_equal(ch, ref[0]), (tag, np.abs(ch - ref[0]).sum())
        assert np.array_equal(sh, ref[1]), (tag, np.abs(sh - ref[1]).sum())
        if m % 128:  # rows >= m of the padded buffer hold NaN: nothing in them reaches a result
            Lbuf2 = Lbuf.copy()
            Lbuf2[m:, :] = np.nan
            ch3, sh3 = path_counts(torch.tensor(Lbuf2, dtype=torch.float64, device=dev), m, thr, **kw)
            assert np.array_equal(ch3.cpu().numpy(), ch) and np.array_equal(sh3.cpu().numpy(), sh), tag


def test_special_thresholds_on_the_device(gpu_device):
    """NaN never counts, -inf / +inf count always / never, and a run through every point is cut by the links."""
    m, N = 70, 130
    Lm = np.linalg.cholesky(_ar1(m))
    Ld = torch.tensor(factor_layout(Lm), dtype=torch.float64, device=gpu_device)
    thr = np.stack([np.full(m, np.nan), np.full(m, -np.inf), np.full(m, np.inf)])
    link = np.ones(m, dtype=np.int32)
    link[[10, 50]] = 0
    for above in (True, False):
        ch, sh = (a.cpu().numpy() for a in path_counts(Ld, m, thr, above=above, link=link, npoints=N, nshifts=2, seed=0))
        always, never = (1, 2) if above else (2, 1)
        assert np.all(ch[0, :, 0] == N) and np.all(sh[0, :, 0] == N) and np.all(ch[never, :, 0] == N) and np.all(sh[never, :, 0] == N)
        assert np.all(ch[always, :, m] == N) and np.all(sh[always, :, 40] == N)  # the pieces are 0 .. 9, 10 .. 49, 50 .. 69


def test_levels_do_not_depend_on_each_other(gpu_device):
    """17 levels in one call (two level chunks of the grid), the same levels one at a time, and the same levels under a
    ``max_bytes`` of one work area (calls of 16 + 1): all equal."""
    m, N, S = 129, 200, 4
    Cm = _wishart(m, m)
    sd = np.sqrt(np.diag(Cm))
    Ld = torch.tensor(factor_layout(np.linalg.cholesky(Cm)), dtype=torch.float64, device=gpu_device)
    thr = np.linspace(-1.5, 2.0, 17)[:, None] * sd[None, :]
    kw = dict(above=True, link=_link(m), npoints=N, nshifts=S, seed=5)
    whole = path_counts(Ld, m, thr, **kw)
    per_call, one = path_count_level_chunks(m, 17, S, N)
    assert per_call == 17 and path_count_level_chunks(m, 17, S, N, max_bytes=one)[0] == 16
    split = path_counts(Ld, m, thr, max_bytes=one, **kw)
    assert torch.equal(whole[0], split[0]) and torch.equal(whole[1], split[1])
    for l in range(17):
        single = path_counts(Ld, m, thr[l], **kw)
        assert torch.equal(single[0][0], whole[0][l]) and torch.equal(single[1][0], whole[1][l]), l
    with pytest.raises(ValueError, match="bytes for ONE level"):
        path_counts(Ld, m, thr, max_bytes=one - 1, **kw)


def test_bad_arguments_are_refused_before_any_launch(gpu_device):
    """Through ctypes on real device buffers: bad sizes, an odd ``ld``, a misaligned or small work area -- the error code comes
    back and the histograms still hold what they held."""
    dev = gpu_device
    lib = _lib.load()
    m, S, N = 70, 2, 130
    Ld = torch.tensor(factor_layout(np.linalg.cholesky(_ar1(m))), dtype=torch.float64, device=dev)
    thr = torch.zeros(1, m, dtype=torch.float64, device=dev)
    gen = torch.from_numpy(richtmyer_generators(m)).to(dev)
    sh = orthant_shifts(m, S, 0).to(dev)
    need = int(lib.dgp_path_counts_workspace_bytes(m, 1, S, N))
    ws = torch.empty(need + 512, dtype=torch.uint8, device=dev)
    wp = ws.data_ptr() + (-ws.data_ptr()) % 256
    hist = torch.full((2, S, m + 1), -7, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ok = [p(Ld), m, 128, p(thr), 1, 1, None, p(gen), p(sh), S, N, C.c_void_p(wp), need, p(hist[0]), p(hist[1]), None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.dgp_path_counts(*a)

    for kw in (dict(a1=0), dict(a1=16385), dict(a4=0), dict(a4=65), dict(a9=1), dict(a9=65), dict(a10=0), dict(a10=(1 << 20) + 1),
               dict(a2=127), dict(a2=64), dict(a11=C.c_void_p(wp + 8)), dict(a0=C.c_void_p(Ld.data_ptr() + 8)), dict(a3=None)):
        assert call(**kw) == _lib.E_ARG, kw
    assert call(a12=need - 1) == _lib.E_WORKSPACE and call(a11=None) == _lib.E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((hist == -7).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((hist.sum(dim=2) == N).all())


# ------------------------------------------------------------------------------------------------ from a fitted model
class LoadestGP32(LoadestGP):
    dtype = torch.float32


class LoadestTwin(LoadestGP):
    """The CPU engine double: the oracle plan, with ``path_counts`` answered by the restatement."""
    device = "cpu"
    _plan_factory = staticmethod(make_count_oracle_plan())


def _record(seed=21):
    """The record of tests/test_gpu_extremes.py: 160 samples over two years and a 300-day record across the turn of the year
    (two periods), with excluded points at the head, in the middle and at the tail."""
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
    calls = []
    model._plan._counts_hook = lambda d: calls.append({k: (v.detach().clone().cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    return calls


def _restate(call):
    m = call["m"]
    return counts_ref(np.tril(call["L"][:m, :m]), call["thr"], call["above"], call["link"], call["gen"], call["shifts"], call["npoints"])


KW = dict(npoints=512, nshifts=4, seed=3)


@pytest.fixture(scope="module", params=[torch.float64, torch.float32], ids=["fp64", "fp32"])
def fitted(request, gpu_device):
    cov_obs, target, rec = _record()
    model = (LoadestGP if request.param == torch.float64 else LoadestGP32)()
    model.fit(cov_obs, target, iterations=5)
    return model, rec, target, cov_obs


def _check_calls(calls, ds, n_p):
    """Every captured device call against the restatement on the device's OWN factor, thresholds and links: the integers
    behind the Dataset, recovered from its pmf, equal the restatement's under the gap condition."""
    for g, call in enumerate(calls):
        ch, sh, gap = _restate(call)
        print(f"period {g}: m = {call['m']}, smallest gap {gap:.3e}")
        assert gap >= GAP_MIN
        for l in range(ch.shape[0]):
            st, sp = F.histogram_statistics(ch[l], n_p[g], call["npoints"]), F.histogram_statistics(sh[l], n_p[g], call["npoints"])
            for name, ref in (("pmf", st["pmf"]), ("cdf", st["cdf"]), ("cdf_error", st["cdf_error"]), ("spell_pmf", sp["pmf"]),
                              ("spell_cdf", sp["cdf"]), ("spell_cdf_error", sp["cdf_error"])):
                assert np.array_equal(ds[name].values[l, g, :n_p[g] + 1], ref), (g, l, name)
            assert ds["mean"].values[l, g] == st["mean"] and ds["variance"].values[l, g] == st["variance"]


def test_exceedance_distribution_from_a_fitted_plan(fitted):
    """freq "YE", two levels, 4 shifts x 512 points on the two 148-point periods of the record.  (1) Every device call against
    the restatement on the device's own inputs: exact.  (2) float64: the Dataset against the same call on the CPU engine double
    (the oracle plan, torch's Cholesky, the restatement) at the fitted parameters: the pmfs equal exactly when the double's
    smallest gap is at least GAP_MIN -- the test prints which branch it took --, otherwise within 2 / npoints per bin.
    (3) The cross-checks at 5 standard errors: P(N <= 0) against ``extreme_probability``'s ``prob_never``, ``mean`` and
    ``variance`` against ``exceedance()``'s exact moments.  The levels are chosen so that the rule resolves every (level,
    period) -- asserted on the exact mean: at least 0.1 expected points, where the 2048 paths see a positive count some hundred
    times; a level whose exact mean is 4e-4 is seen by no path, and its estimate 0 comes with an estimated error of 0."""
    model, rec, target, cov_obs = fitted
    levels = np.quantile(np.asarray(target.values), [0.6, 0.75])
    calls = _capture(model)
    try:
        ds = model.exceedance_distribution(rec, threshold=levels, **KW)
    finally:
        model._plan._counts_hook = None
    n_p = list(ds["n_points"].values)
    assert n_p == [148, 148] and len(calls) == 2 and ds["pmf"].values.shape == (2, 2, 149) and ds.attrs["exact"] is False
    assert all(c["L"].dtype == np.float64 and c["above"] is True for c in calls)
    assert all(c["link"][0] == 0 and np.all(c["link"][1:] == 1) for c in calls)  # the excluded points lie at the periods' ends
    _check_calls(calls, ds, n_p)
    assert np.all(ds["cdf"].values[:, :, -1] == 1.0) and np.all(np.diff(ds["cdf"].values, axis=2) >= 0)

    if model.dtype == torch.float64:
        twin = LoadestTwin()
        twin.fit(cov_obs, target, iterations=1)
        for mine, theirs in ((twin.model, model.model), (twin.likelihood, model.likelihood)):
            mine.load_state_dict({k: v.detach().cpu() for k, v in theirs.state_dict().items()})
        plan_cls = LoadestTwin._plan_factory
        plan_cls.calls.clear()
        dt = twin.exceedance_distribution(rec, threshold=levels, **KW)
        gap = min(c["gap"] for c in plan_cls.calls)
        diff = max(float(np.nanmax(np.abs(ds[k].values - dt[k].values))) for k in ("pmf", "spell_pmf"))
        print(f"CPU double: smallest gap {gap:.3e}, largest pmf difference {diff:.3e} -> "
              f"{'exact comparison' if gap >= GAP_MIN else 'within 2 / npoints per bin'}")
        if gap >= GAP_MIN:
            assert diff == 0.0
        else:
            assert diff <= 2.0 / KW["npoints"]

    comp = model.compliance_probability(rec, threshold=levels, allowed=0, max_spell=5, **KW)
    ext = model.extreme_probability(rec, threshold=levels, **KW)
    exact = model.exceedance(rec, threshold=levels)
    print("P(N = 0)", comp["prob"].values, "+-", comp["error"].values, "prob_never", ext["prob_never"].values, "+-", ext["error"].values)
    print("mean", ds["mean"].values, "+-", ds["mean_error"].values, "exact", exact["mean"].values)
    print("variance", ds["variance"].values, "+-", ds["variance_error"].values, "exact", exact["se"].values ** 2)
    assert np.all(exact["mean"].values >= 0.1)  # the condition on the inputs: every (level, period) is resolved
    assert np.array_equal(comp["prob"].values, ds["cdf"].values[:, :, 0]) and np.array_equal(comp["prob_spell"].values, ds["spell_cdf"].values[:, :, 5])
    assert np.all(np.abs(comp["prob"].values - ext["prob_never"].values) <= 5 * np.hypot(comp["error"].values, ext["error"].values))
    assert np.all(np.abs(ds["mean"].values - exact["mean"].values) <= 5 * ds["mean_error"].values)
    assert np.all(np.abs(ds["variance"].values - exact["se"].values ** 2) <= 5 * ds["variance_error"].values)


def test_censored_fit_takes_the_same_path(gpu_device):
    """A fit with non-detects (the Laplace posterior) runs through the same call without a special case; ``above=False`` and a
    7-day window on the way."""
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
    levels = np.quantile(vals, [0.45, 0.55])
    calls = _capture(model)
    try:
        ds = model.exceedance_distribution(rec, threshold=levels, above=False, window="7D", **KW)
    finally:
        model._plan._counts_hook = None
    n_p = list(ds["n_points"].values)
    assert len(calls) == 2 and [c["m"] for c in calls] == n_p and all(c["above"] is False for c in calls) and ds.attrs["window"] == "7D"
    _check_calls(calls, ds, n_p)
    exact = model.exceedance(rec, threshold=levels, above=False, window="7D")
    print("mean", ds["mean"].values, "+-", ds["mean_error"].values, "exact", exact["mean"].values)
    # the condition on the inputs: no (level, period) is saturated at 0 or at all of its points, where no path resolves the rest
    assert np.all(exact["mean"].values >= 0.1) and np.all(exact["mean"].values <= np.asarray(n_p)[None, :] - 0.1)
    assert np.all(np.abs(ds["mean"].values - exact["mean"].values) <= 5 * ds["mean_error"].values)
