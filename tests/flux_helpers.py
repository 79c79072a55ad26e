"""Builders and dense references shared by the period-moment tests (tests/test_flux_cpu.py, tests/test_gpu_flux.py)."""
from __future__ import annotations

import numpy as np
import torch

from discontinuum_amd.xr_compat import DataArray, Dataset
from oracle import gp_oracle as orc
from tests.helpers import OraclePlan


def dense_period_moments(cov, mu, scale2, w, groups, ngroups, mode, extra_var=None):
    """The closed form of ``dgp_period_moments`` on a dense SYMMETRIC fp64 covariance (m, m), in torch:
    log (mode 1): a = w exp(mu + s2 C_ii / 2), mean = A^T a, cov = A^T (a a^T * expm1(s2 C)) A;
    linear (mode 0): mean = A^T (w mu), cov = s2 A^T (w w^T * C) A, A the one-hot (m, P) group matrix."""
    cov = torch.as_tensor(cov, dtype=torch.float64)
    dev = cov.device
    mu = torch.as_tensor(mu, dtype=torch.float64, device=dev)
    w = torch.as_tensor(w, dtype=torch.float64, device=dev)
    g = torch.as_tensor(groups, dtype=torch.int64, device=dev)
    valid = g >= 0
    A = torch.zeros(g.shape[0], ngroups, dtype=torch.float64, device=dev)
    A[valid.nonzero().reshape(-1), g[valid]] = 1.0
    C = cov.clone()
    if extra_var is not None:
        C.diagonal().add_(torch.as_tensor(extra_var, dtype=torch.float64, device=dev))
    w = torch.where(valid, w, torch.zeros_like(w))
    s2 = float(scale2)
    if mode == 1:
        a = w * torch.exp(mu + 0.5 * s2 * C.diagonal())
        a = torch.where(valid, a, torch.zeros_like(a))
        return A.T @ a, A.T @ ((a[:, None] * torch.expm1(s2 * C) * a[None, :]) @ A)
    mu = torch.where(valid, mu, torch.zeros_like(mu))
    return A.T @ (w * mu), s2 * (A.T @ ((w[:, None] * C * w[None, :]) @ A))


def symmetrise_lower(cov):
    """Full symmetric matrix from a ``dgp_posterior_cov`` buffer (lower triangle valid)."""
    low = torch.tril(cov)
    return low + torch.tril(cov, -1).T


class FluxOraclePlan(OraclePlan):
    """``OraclePlan`` with the two entries ``aggregate`` uses: a dense posterior covariance from the oracle and the
    period moments by the dense formulas."""

    def posterior_cov(self, theta, Xs):
        theta, r, noise = self._state
        mu, cov = orc.posterior(self.model, self.X, r, noise, theta, Xs.double(), full_cov=True)
        return mu.to(self.dtype), cov.to(self.dtype)

    def period_moments(self, cov, m, mu, scale2, w, groups, ngroups, mode, extra_var=None):
        return dense_period_moments(cov, mu, scale2, w, groups, ngroups, mode, extra_var)


def daily_loadest(n_obs=60, start="2012-01-01", end="2015-01-01", seed=0, step_days=1):
    """A sampled concentration record (mg/l) and a daily flow record (m^3/s) over [start, end)."""
    rng = np.random.default_rng(seed)
    days = np.arange(start, end, step_days, dtype="datetime64[D]")
    tday = days.astype("datetime64[ns]")
    season = np.sin(2 * np.pi * np.arange(len(days)) / 365.25)
    flow = np.exp(1.0 + 0.6 * season + 0.3 * np.cumsum(rng.standard_normal(len(days))) / np.sqrt(len(days))) * 10
    pick = np.sort(rng.choice(len(days), n_obs, replace=False))
    conc = np.exp(0.3 * np.log(flow[pick]) + 0.2 * rng.standard_normal(n_obs))
    cov_obs = Dataset({"flow": ("time", flow[pick], {"units": "cubic meters per second"})}, coords={"time": tday[pick]})
    target = DataArray(conc, dims=("time",), coords={"time": tday[pick]}, name="concentration",
                       attrs={"units": "mg/l", "long_name": "Concentration"})
    daily = Dataset({"flow": ("time", flow, {"units": "cubic meters per second"})}, coords={"time": tday})
    return cov_obs, target, daily


def daily_rating(n_obs=40, start="2012-01-01", end="2015-01-01", seed=0):
    rng = np.random.default_rng(seed)
    days = np.arange(start, end, dtype="datetime64[D]").astype("datetime64[ns]")
    stage_daily = 1.0 + 3.0 * rng.beta(2, 5, len(days))
    pick = np.sort(rng.choice(len(days), n_obs, replace=False))
    stage = stage_daily[pick]
    q = np.exp(1.6 * np.log(stage) + 0.05 * rng.standard_normal(n_obs))
    cov_obs = Dataset({"stage": ("time", stage)}, coords={"time": days[pick]})
    target = DataArray(q, dims=("time",), coords={"time": days[pick]}, name="discharge", attrs={"units": "cfs"})
    unc = DataArray(np.full(n_obs, 1.05), dims=("time",), coords={"time": days[pick]}, name="discharge_unc")
    daily = Dataset({"stage": ("time", stage_daily)}, coords={"time": days})
    return cov_obs, target, unc, daily


def one_hot(groups, ngroups):
    g = np.asarray(groups)
    A = np.zeros((g.shape[0], ngroups))
    ok = g >= 0
    A[np.nonzero(ok)[0], g[ok]] = 1.0
    return A


def gaussian_draws(mu, cov, ndraw, seed=0, chunk=20000, rel_cut=1e-12):
    """Seeded numpy draws of N(mu, cov) in chunks (ndraw_chunk, m), through the eigen-decomposition of cov with
    eigenvalues below rel_cut x the largest dropped (they carry no measurable variance)."""
    mu, cov = np.asarray(mu, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    lam, U = np.linalg.eigh(0.5 * (cov + cov.T))
    keep = lam > rel_cut * lam.max()
    B = U[:, keep] * np.sqrt(lam[keep])
    rng = np.random.default_rng(seed)
    done = 0
    while done < ndraw:
        k = min(chunk, ndraw - done)
        yield mu[None, :] + rng.standard_normal((k, B.shape[1])) @ B.T
        done += k
