"""Exact period sums (``MarginalHIP.aggregate``, ``LoadestGP.annual_flux``) on CPU: the host logic -- grouping, weights,
transform, intervals -- against a seeded Monte Carlo of the reference workflow (draws from the posterior ->
``concentration_to_flux`` -> period sums), with the device plan replaced by an oracle-backed double; the reference's
``concentration_to_flux``; and the new C entries' argument checks without a device."""
import ctypes as C
import warnings

import numpy as np
import pandas as pd
import pytest
import torch

from discontinuum_amd import _lib
from discontinuum_amd.engines.base import ModelConfig
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP, concentration_to_flux
from discontinuum_amd.loads import period_groups, target_transform
from discontinuum_amd.rating_gp import RatingGP
from discontinuum_amd.xr_compat import DataArray, Dataset
from tests.flux_helpers import FluxOraclePlan, daily_loadest, daily_rating, gaussian_draws, one_hot

NDRAW = 200_000


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(FluxOraclePlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)


def _posterior(model, daily, pred_noise=False):
    """Model-space posterior mean and covariance at the daily points, as the engine sees them."""
    model._ensure_factor()
    x = torch.tensor(model.dm.Xnew(daily), dtype=torch.float64)
    kmean, cov = model._plan.posterior_cov(model._factor_theta, x)
    mu = (kmean + model.model.prior_mean(x)).detach().numpy()
    cov = cov.numpy().copy()
    if pred_noise:
        cov[np.diag_indices_from(cov)] += model.likelihood.predictive_noise(x.shape[0], x.device, torch.float64).detach().numpy()
    return mu, cov


def _scale_shift(model):
    _mode, s, t = target_transform(model.dm)
    return s, t


def _check(exact, sums, name):
    """Means within 5 Monte Carlo standard errors, standard errors within 2 %."""
    mc_mean, mc_sd = sums.mean(axis=0), sums.std(axis=0, ddof=1)
    mean, se = np.asarray(exact["mean"].values), np.asarray(exact["se"].values)
    assert mean.shape == mc_mean.shape, name
    live = mc_sd > 0
    z = np.abs(mean - mc_mean)[live] / (mc_sd[live] / np.sqrt(sums.shape[0]))
    assert np.all(z < 5), (name, z.max())
    assert np.allclose(se[live], mc_sd[live], rtol=0.02, atol=0), (name, np.max(np.abs(se[live] / mc_sd[live] - 1)))
    assert np.all(exact["lower"].values <= mean) and np.all(exact["upper"].values >= mean), name


def test_annual_flux_matches_the_reference_workflow_by_monte_carlo():
    cov_obs, target, daily = daily_loadest()
    model = LoadestGP()
    model.fit(cov_obs, target, iterations=10)
    flow_nan = np.array(daily["flow"].values, dtype=np.float64)
    flow_nan[100] = np.nan  # one missing day in 2012: skipped, like resample().sum()
    daily_nan = Dataset({"flow": ("time", flow_nan, {"units": "cubic meters per second"})},
                        coords={"time": daily.coords["time"].values})
    cases = {
        "YE": (daily, "YE"),
        "YE-SEP": (daily, "YE-SEP"),
        "ME": (daily, "ME"),
        "YE nan": (daily_nan, "YE"),
    }
    exact = {k: model.annual_flux(d, freq=f) for k, (d, f) in cases.items()}
    time = daily.coords["time"].values
    assert list(pd.DatetimeIndex(exact["YE"].coords["time"].values).strftime("%Y-%m-%d")) == ["2012-12-31", "2013-12-31", "2014-12-31"]
    assert list(pd.DatetimeIndex(exact["YE-SEP"].coords["time"].values).year) == [2012, 2013, 2014, 2015]
    assert len(exact["ME"]["mean"].values) == 36
    assert list(exact["YE"]["n_points"].values) == [366, 365, 365]
    assert list(exact["YE nan"]["n_points"].values) == [365, 365, 365]
    assert exact["YE"]["mean"].attrs["units"] == "kilograms" and exact["YE"]["mean"].attrs["standard_name"] == "flux"

    mu, cov = _posterior(model, daily)
    s, t = _scale_shift(model)
    onehots = {}
    for k, (d, f) in cases.items():
        order, groups, labels, _n, _drop = period_groups(time, np.asarray(d["flow"].values), f)
        onehots[k] = np.empty((len(time), len(labels)))
        onehots[k][order] = one_hot(groups, len(labels))  # rows back in time order
    sums = {k: [] for k in cases}
    for f in gaussian_draws(mu, cov, NDRAW, seed=1):
        conc = DataArray(np.exp(s * f + t), dims=("draw", "time"), coords={"draw": np.arange(f.shape[0]), "time": time},
                         attrs={"units": "mg/l"})
        for k, (d, _f) in cases.items():
            flux = concentration_to_flux(conc, d["flow"]).values
            sums[k].append(np.where(np.isfinite(flux), flux, 0.0) @ onehots[k])
    for k in cases:
        _check(exact[k], np.concatenate(sums[k]), k)


def test_standard_transform_is_the_linear_mode():
    cov_obs, target, daily = daily_loadest(seed=3)
    model = LoadestGP(model_config=ModelConfig(transform="standard"))
    model.fit(cov_obs, target, iterations=10)
    assert target_transform(model.dm)[0] == 0
    exact, pcov = model.annual_flux(daily, freq="YE", return_cov=True)
    assert pcov.shape == (3, 3) and np.allclose(pcov, pcov.T)
    assert np.allclose(np.sqrt(np.diag(pcov)), exact["se"].values)
    mu, cov = _posterior(model, daily)
    s, t = _scale_shift(model)
    time = daily.coords["time"].values
    _o, groups, labels, _n, _d = period_groups(time, daily["flow"].values, "YE")
    A = one_hot(groups, len(labels))
    sums = []
    for f in gaussian_draws(mu, cov, NDRAW, seed=2):
        conc = DataArray(s * f + t, dims=("draw", "time"), coords={"draw": np.arange(f.shape[0]), "time": time},
                         attrs={"units": "mg/l"})
        sums.append(concentration_to_flux(conc, daily["flow"]).values @ A)
    _check(exact, np.concatenate(sums), "standard")


def test_rating_aggregate_with_predictive_noise():
    """RatingGP.aggregate with weights = time step: runoff volume per year; pred_noise adds the learned noise."""
    cov_obs, target, unc, daily = daily_rating()
    model = RatingGP()
    model.fit(cov_obs, target, target_unc=unc, iterations=10)
    dt = np.full(len(daily.coords["time"].values), 86400.0)
    latent = model.aggregate(daily, dt, freq="YE")
    noisy = model.aggregate(daily, dt, freq="YE", pred_noise=True)
    assert np.all(noisy["se"].values > latent["se"].values)
    mu, cov = _posterior(model, daily, pred_noise=True)
    s, t = _scale_shift(model)
    _o, groups, labels, _n, _d = period_groups(daily.coords["time"].values, dt, "YE")
    A = one_hot(groups, len(labels)) * dt[:, None]
    sums = [np.exp(s * f + t) @ A for f in gaussian_draws(mu, cov, NDRAW, seed=3)]
    _check(noisy, np.concatenate(sums), "rating pred_noise")


def test_grouping_transform_and_grid_checks():
    time = np.array(["2013-10-02", "2012-03-01", "2012-12-31T12:00", "2013-01-01"], dtype="datetime64[ns]")
    order, groups, labels, n_points, dropped = period_groups(time, [1.0, 2.0, np.nan, 1.0], "YE")
    assert list(groups) == [-1, 0, 1, 1] and list(order) == [2, 1, 0, 3]
    assert list(n_points) == [1, 2] and dropped == 1
    assert list(pd.DatetimeIndex(labels).strftime("%Y-%m-%d")) == ["2012-12-31", "2013-12-31"]
    _o, g, lab, _n, _d = period_groups(time, np.ones(4), "YE-SEP")
    assert list(pd.DatetimeIndex(lab).strftime("%Y-%m-%d")) == ["2012-09-30", "2013-09-30", "2014-09-30"]
    assert np.all(np.diff(g) >= 0)
    with pytest.raises(ValueError):
        period_groups(time, [np.nan] * 4, "YE")
    cov_obs, target, daily = daily_loadest(step_days=2)
    model = LoadestGP()
    model.fit(cov_obs, target, iterations=2)
    irregular = Dataset({"flow": ("time", daily["flow"].values[[0, 1, 3]], {"units": "cubic meters per second"})},
                        coords={"time": daily.coords["time"].values[[0, 1, 3]]})
    with pytest.raises(ValueError, match="regular"):
        model.annual_flux(irregular)
    with pytest.warns(UserWarning, match="cubic meters per second"):
        model.annual_flux(Dataset({"flow": ("time", daily["flow"].values)}, coords={"time": daily.coords["time"].values}))
    model.dm.target_pipeline.steps = [st for st in model.dm.target_pipeline.steps if st[0] != "log"]
    with pytest.raises(NotImplementedError):
        model.annual_flux(daily)
    with pytest.raises(RuntimeError, match="hasn't been fitted"):
        LoadestGP().annual_flux(daily)


def test_concentration_to_flux_is_the_reference_function():
    time = np.arange("2012-01-01", "2012-01-11", dtype="datetime64[D]").astype("datetime64[ns]")
    conc = DataArray(np.linspace(1, 2, 10), dims=("time",), coords={"time": time}, name="concentration",
                     attrs={"units": "mg/l", "long_name": "Nitrate"})
    flow = DataArray(np.full(10, 3.0), dims=("time",), coords={"time": time}, name="flow",
                     attrs={"units": "cubic meters per second"})
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        flux = concentration_to_flux(conc, flow)
    assert np.allclose(flux.values, np.linspace(1, 2, 10) * 3.0 * 86400 * 1e-3)
    assert flux.attrs == {"units": "kilograms", "long_name": "Nitrate", "standard_name": "flux"}
    assert conc.attrs["units"] == "mg/l"  # the input keeps its own attributes
    draws = DataArray(np.outer(np.arange(1, 4), np.ones(10)), dims=("draw", "time"),
                      coords={"draw": np.arange(3), "time": time}, attrs={"units": "mg/l"})
    fd = concentration_to_flux(draws, flow)
    assert fd.values.shape == (3, 10) and fd.dims == ("draw", "time")
    assert np.allclose(fd.values[2], 3 * 3.0 * 86400 * 1e-3)
    with pytest.warns(UserWarning, match="cubic meters per second"):
        concentration_to_flux(conc, DataArray(np.ones(10), dims=("time",), coords={"time": time}, attrs={"units": "cfs"}))
    with pytest.warns(UserWarning, match="mg/l"):
        concentration_to_flux(DataArray(np.ones(10), dims=("time",), coords={"time": time}, attrs={"units": "ug/l"}), flow)
    gap = np.concatenate([time[:5], time[6:]])
    with pytest.warns(UserWarning, match="not constant"):
        try:
            concentration_to_flux(DataArray(np.ones(9), dims=("time",), coords={"time": gap}, attrs={"units": "mg/l"}),
                                  DataArray(np.ones(9), dims=("time",), coords={"time": gap}, attrs=flow.attrs))
        except ValueError:  # the reference's arithmetic cannot broadcast the two time steps either
            pass


def test_period_moments_abi_without_a_device():
    lib = _lib.load()
    assert hasattr(lib, "dgp_period_moments") and hasattr(lib, "dgp_period_moments_workspace_bytes")
    need = lib.dgp_period_moments_workspace_bytes(1000, 3, 2)
    M = lib.dgp_padded_n(1000)
    assert need >= 2 * 8 * (1000 * 3 + 2 * 1000) and need == 2 * 8 * (2 * M + M * 3 + 3)
    assert lib.dgp_period_moments_workspace_bytes(0, 3, 1) == 0 and lib.dgp_period_moments_workspace_bytes(10, 0, 1) == 0
    p = C.c_void_p(16)  # never dereferenced: every call below fails its host-side checks
    args = lambda **kw: [kw.get("dtype", 0), kw.get("mode", 1), kw.get("cov", p), kw.get("m", 1000), kw.get("batch", 2), p, p, p, p,  # noqa: E731
                         kw.get("ng", 3), None, kw.get("work", p), kw.get("wb", need), p, p, None]
    assert lib.dgp_period_moments(*args(dtype=2)) == -1 and b"dtype" in lib.dgp_last_error()
    assert lib.dgp_period_moments(*args(mode=2)) == -1 and b"mode" in lib.dgp_last_error()
    assert lib.dgp_period_moments(*args(cov=None)) == -1 and b"null" in lib.dgp_last_error()
    assert lib.dgp_period_moments(*args(m=0)) == -1
    assert lib.dgp_period_moments(*args(ng=0)) == -1 and b"size" in lib.dgp_last_error()
    assert lib.dgp_period_moments(*args(batch=0)) == -1
    assert lib.dgp_period_moments(*args(wb=need - 1)) == -3 and b"workspace" in lib.dgp_last_error()
    assert lib.dgp_period_moments(*args(work=None)) == -3
