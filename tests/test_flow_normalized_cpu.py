"""Flow-normalized loads (``loads.flow_normalized``), ``loads.period_change`` and the path selection of ``aggregate`` on CPU,
with the device plan replaced by an oracle-backed double whose streamed entry is the oracle posterior + the dense formulas;
and the new C entry's argument checks without a device."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch
from scipy.stats import norm

from discontinuum_amd import _lib, loads
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.xr_compat import Dataset
from oracle import gp_oracle as orc
from tests.flux_helpers import FluxOraclePlan, daily_loadest, dense_period_moments


class StreamedOraclePlan(FluxOraclePlan):
    streamed_calls = 0

    def posterior_period_moments(self, theta, Xs, mu, scale2, w, groups, ngroups, mode, extra_var=None):
        StreamedOraclePlan.streamed_calls += 1
        th, r, noise = self._state
        _mu, cov = orc.posterior(self.model, self.X, r, noise, th, Xs.double(), full_cov=True)
        return dense_period_moments(cov, mu, scale2, w, groups, ngroups, mode, extra_var)


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(StreamedOraclePlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)


@pytest.fixture(scope="module")
def fitted():
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(MarginalHIP, "_plan_factory", staticmethod(StreamedOraclePlan))
        mp.setattr(MarginalHIP, "device", "cpu")
        cov_obs, target, daily = daily_loadest(start="2012-01-01", end="2015-01-01")
        model = LoadestGP()
        model.fit(cov_obs, target, iterations=5)
    return model, daily


def _daily(time, flow):
    return Dataset({"flow": ("time", np.asarray(flow, dtype=np.float64), {"units": "cubic meters per second"})},
                   coords={"time": np.asarray(time).astype("datetime64[ns]")})


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def test_point_set_matches_a_pandas_restatement():
    time = pd.date_range("2011-11-01", "2013-03-10", freq="D")
    rng = np.random.default_rng(1)
    flow = rng.uniform(1, 10, len(time))
    flow[[3, 40, 450]] = np.nan
    pts = loads.flow_normalized_points(_daily(time, flow))
    # restatement: key = the date's month-day on a common year, 29 Feb read as 28 Feb
    md = [f"2001-{t.month:02d}-{min(t.day, 28) if t.month == 2 else t.day:02d}" for t in time]
    key = pd.DatetimeIndex(md).dayofyear.to_numpy() - 1
    frame = pd.DataFrame({"time": time, "flow": flow, "key": key})
    sets = frame.dropna().groupby("key")["flow"].apply(list)
    rows = []
    for t, k in zip(time, key):
        for q in sets.get(k, []):
            rows.append((t, q, k, len(sets[k]), t.year))
    ref = pd.DataFrame(rows, columns=["time", "flow", "key", "size", "year"])
    assert np.array_equal(pts["time"], ref["time"].to_numpy().astype("datetime64[ns]"))
    assert np.array_equal(pts["flow"], ref["flow"].to_numpy())
    assert np.array_equal(pts["key"], ref["key"].to_numpy()) and np.array_equal(pts["set_size"], ref["size"].to_numpy())
    assert np.array_equal(pts["group"], ref["year"].to_numpy() - 2011)
    assert np.allclose(pts["weight"], ref["flow"] * 86.4 / ref["size"], rtol=1e-15, atol=0)
    day_sums = pd.Series(pts["weight"]).groupby(pts["time"]).sum()
    day_means = pd.Series(pts["flow"]).groupby(pts["time"]).mean() * 86.4
    assert np.allclose(day_sums.to_numpy(), day_means.to_numpy(), rtol=1e-13)
    conc = loads.flow_normalized_points(_daily(time, flow), kind="concentration")
    assert np.allclose(np.bincount(conc["group"], weights=conc["weight"]), 1.0, rtol=1e-13)
    assert list(conc["n_points"]) == [61, 366, 69]
    leap = pd.Timestamp("2012-02-29")
    assert set(pts["key"][pts["time"] == np.datetime64(leap, "ns")]) == {58}


def _repeating(time, rng):
    base = rng.uniform(2, 20, 365)
    return base[loads.day_keys(time)]


def test_repeating_flows_give_the_plain_loads(fitted):
    model, daily = fitted
    time = daily.coords["time"].values
    rec = _daily(time, _repeating(time, np.random.default_rng(2)))
    fn, fcov = model.flow_normalized_flux(rec, return_cov=True)
    af, acov = model.annual_flux(rec, return_cov=True)
    assert _rel(fn["mean"].values, af["mean"].values) <= 1e-10 and _rel(fcov, acov) <= 1e-10
    assert fn["mean"].attrs["long_name"].startswith("Flow-normalized")
    assert list(fn["n_points"].values) == list(af["n_points"].values)
    fc, ccov = model.flow_normalized_concentration(rec, return_cov=True)
    days = pd.DatetimeIndex(time)
    per_year = pd.Series(1, index=days).groupby(days.year).transform("sum").to_numpy()
    ag, gcov = model.aggregate(rec, 1.0 / per_year, return_cov=True)
    assert _rel(fc["mean"].values, ag["mean"].values) <= 1e-10 and _rel(ccov, gcov) <= 1e-10


def test_flow_window_is_the_base_year_substitution(fitted):
    model, daily = fitted
    time = daily.coords["time"].values
    flow = np.asarray(daily["flow"].values)
    keys = loads.day_keys(time)
    in_2013 = pd.DatetimeIndex(time).year == 2013
    base = np.empty(365)
    base[keys[in_2013]] = flow[in_2013]
    fn, fcov = model.flow_normalized_flux(daily, flow_window=("2013-01-01", "2013-12-31"), return_cov=True)
    af, acov = model.annual_flux(_daily(time, base[keys]), return_cov=True)
    assert _rel(fn["mean"].values, af["mean"].values) <= 1e-10 and _rel(fcov, acov) <= 1e-10


def test_period_change(fitted):
    model, daily = fitted
    for ds, cov in (model.flow_normalized_flux(daily, return_cov=True), model.annual_flux(daily, return_cov=True)):
        out = loads.period_change(ds, cov, "2012", "2014-06-30", ci=0.9)
        mean = ds["mean"].values
        change, se = mean[2] - mean[0], np.sqrt(cov[2, 2] + cov[0, 0] - 2 * cov[0, 2])
        assert out["change"] == pytest.approx(change, rel=1e-14) and out["se"] == pytest.approx(se, rel=1e-14)
        assert out["lower"] == pytest.approx(change - norm.ppf(0.95) * se, rel=1e-12)
        assert out["upper"] == pytest.approx(change + norm.ppf(0.95) * se, rel=1e-12)
        assert pd.Timestamp(out["start"]).year == 2012 and pd.Timestamp(out["end"]).year == 2014
        with pytest.raises(ValueError):
            loads.period_change(ds, cov, "2012", "2030")


def test_errors(fitted):
    model, daily = fitted
    time = daily.coords["time"].values
    with pytest.raises(ValueError, match="daily"):
        model.flow_normalized_flux(_daily(time[::2], np.asarray(daily["flow"].values)[::2]))
    pipes = model.dm.covariate_pipelines
    try:
        model.dm.covariate_pipelines = dict(pipes, baseflow=pipes["flow"])
        with pytest.raises(ValueError, match="baseflow"):
            model.flow_normalized_flux(daily)
    finally:
        model.dm.covariate_pipelines = pipes
    with pytest.raises(RuntimeError, match="hasn't been fitted"):
        LoadestGP().flow_normalized_flux(daily)


def test_tiny_budget_takes_the_streamed_path(fitted):
    model, daily = fitted
    w = np.full(len(daily.coords["time"].values), 2.0)
    before = StreamedOraclePlan.streamed_calls
    dense, dcov = model.aggregate(daily, w, return_cov=True)
    assert StreamedOraclePlan.streamed_calls == before
    streamed, scov = model.aggregate(daily, w, return_cov=True, max_bytes=1024)
    assert StreamedOraclePlan.streamed_calls == before + 1
    assert _rel(streamed["mean"].values, dense["mean"].values) <= 1e-12 and _rel(scov, dcov) <= 1e-12


def test_streamed_abi_without_a_device():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.dgp_plan_create(_lib.MODEL_LOADEST, _lib.F64, 300, 2, C.byref(h)) == 0
    q = lib.dgp_posterior_period_moments_workspace_bytes
    assert q(None, 1000, 3) == 0 and q(h, 0, 3) == 0 and q(h, 1000, 0) == 0 and q(h, 1 << 21, 3) == 0
    assert q(h, 1000, 3) == lib.dgp_predict_workspace_bytes(h, 1000) + lib.dgp_period_moments_workspace_bytes(1000, 3, 1)
    p = C.c_void_p(16)  # never dereferenced: every call below fails its host-side checks
    th = (C.c_double * 9)(*([0.5] * 9))

    def call(plan=h, mode=1, Xs=p, m=1000, ng=3):
        return lib.dgp_posterior_period_moments(plan, th, Xs, m, mode, p, p, p, p, ng, None, p, 1 << 30, p, p, None)

    assert call(plan=None) == -1
    assert call(mode=2) == -1 and b"mode" in lib.dgp_last_error()
    assert call(Xs=None) == -1 and b"null" in lib.dgp_last_error()
    assert call(m=0) == -1 and call(ng=0) == -1 and b"size" in lib.dgp_last_error()
    assert call() == -4 and b"factorisation" in lib.dgp_last_error()  # DGP_E_STATE
    assert lib.dgp_plan_destroy(h) == 0


def test_period_change_follows_the_result_frequency(fitted):
    model, daily = fitted
    ds, cov = model.annual_flux(daily, freq="ME", return_cov=True)
    out = loads.period_change(ds, cov, "2012-01-01", "2012-03-15")
    mean = ds["mean"].values
    assert out["change"] == pytest.approx(mean[2] - mean[0], rel=1e-14)
    assert str(pd.Timestamp(out["start"]).date()) == "2012-01-31" and str(pd.Timestamp(out["end"]).date()) == "2012-03-31"
    yearly, ycov = model.annual_flux(daily, return_cov=True)
    for outside in ("2011-12-31", "2010-12-31", "2015-01-01"):
        with pytest.raises(ValueError, match="none of the periods"):
            loads.period_change(yearly, ycov, outside, "2013")
    quarterly, qcov = model.annual_flux(daily, freq="QE", return_cov=True)
    with pytest.raises(ValueError):
        loads.period_change(quarterly, qcov, "2011-12-31", "2013")
    assert loads.period_change(quarterly, qcov, "2012-01-01", "2012-12-31")["end"] == np.datetime64("2012-12-31", "ns")
