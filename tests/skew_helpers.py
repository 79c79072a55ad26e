"""Dense references and builders shared by the third-moment tests (tests/test_skew_cpu.py, tests/test_gpu_skew.py)."""
from __future__ import annotations

import numpy as np
import torch

from tests.flux_helpers import FluxOraclePlan


def _prepare(cov, mu, scale2, w, groups, extra_var):
    cov = torch.as_tensor(cov, dtype=torch.float64)
    dev = cov.device
    mu = torch.as_tensor(mu, dtype=torch.float64, device=dev)
    w = torch.as_tensor(w, dtype=torch.float64, device=dev)
    g = torch.as_tensor(groups, dtype=torch.int64, device=dev)
    C = cov.clone()
    if extra_var is not None:
        C.diagonal().add_(torch.as_tensor(extra_var, dtype=torch.float64, device=dev))
    s2 = float(scale2)
    a = w * torch.exp(mu + 0.5 * s2 * C.diagonal())
    return C, a, g, s2


def dense_third_moments(cov, mu, scale2, w, groups, ngroups, extra_var=None):
    """The closed form of ``dgp_period_third_moments`` on a dense SYMMETRIC fp64 covariance (m, m), in torch, period by
    period: with a = w exp(mu + s2 C_ii / 2) and e = expm1(s2 C) restricted to the period,
    k3 = sum_ij a_i a_j e_ij G_ij + 3 sum_i a_i y_i^2, G = e diag(a) e^T, y = e a.  -> (P,) float64."""
    C, a, g, s2 = _prepare(cov, mu, scale2, w, groups, extra_var)
    out = torch.zeros(ngroups, dtype=torch.float64, device=C.device)
    for p in range(ngroups):
        idx = (g == p).nonzero().reshape(-1)
        if idx.numel() == 0:
            continue
        e, ap = torch.expm1(s2 * C[idx][:, idx]), a[idx]
        G = (e * ap[None, :]) @ e.T
        y = e @ ap
        out[p] = (ap[:, None] * ap[None, :] * e * G).sum() + 3.0 * (ap * y * y).sum()
    return out


def brute_third_moments(cov, mu, scale2, w, groups, ngroups, extra_var=None):
    """The same by raw moments (periods of at most 130 points): with E = exp(s2 C),
    M1 = sum a_i, M2 = sum a_i a_j E_ij, M3 = sum a_i a_j a_k E_ij E_ik E_jk (one triple ``einsum``),
    k3 = M3 - 3 M1 M2 + 2 M1^3.  -> (k3 (P,), cv (P,)): the subtraction loses about cv^-3 in relative accuracy."""
    C, a, g, s2 = _prepare(cov, mu, scale2, w, groups, extra_var)
    k3, cv = np.zeros(ngroups), np.zeros(ngroups)
    for p in range(ngroups):
        idx = (g == p).nonzero().reshape(-1)
        if idx.numel() == 0:
            continue
        assert idx.numel() <= 130
        E, ap = torch.exp(s2 * C[idx][:, idx]).numpy(), a[idx].numpy()
        M1 = ap.sum()
        M2 = np.einsum("i,j,ij->", ap, ap, E)
        M3 = np.einsum("i,j,k,ij,ik,jk->", ap, ap, ap, E, E, E, optimize=True)
        k3[p] = M3 - 3.0 * M1 * M2 + 2.0 * M1 ** 3
        cv[p] = np.sqrt(max(M2 - M1 * M1, 0.0)) / M1
    return k3, cv


class SkewOraclePlan(FluxOraclePlan):
    """``FluxOraclePlan`` with a dense ``period_third_moments``; ``third_calls`` counts its calls over all instances."""

    third_calls = 0

    def period_third_moments(self, cov, m, mu, scale2, w, groups, ngroups, extra_var=None, tile=0):
        SkewOraclePlan.third_calls += 1
        return dense_third_moments(cov, mu, scale2, w, groups, ngroups, extra_var)


def storm_record(sd, ell, nobs, flowsd, seed, days=365, rho=0.9, noise=0.01):
    """A synthetic storm-dominated posterior: ``days`` daily points under a Matern-1/2 prior (standard deviation ``sd``,
    length ``ell`` days) conditioned on ``nobs`` evenly spaced samples with noise variance ``noise``; flow weights
    exp(flowsd z) and posterior mean 0.3 flowsd z for a stationary unit-variance AR(1) series z (lag-one correlation
    ``rho``) from ``seed``.  -> (mu (days,), cov (days, days), w (days,))."""
    rng = np.random.default_rng(seed)
    eps = rng.standard_normal(days)
    z = np.empty(days)
    z[0] = eps[0]
    for k in range(1, days):
        z[k] = rho * z[k - 1] + np.sqrt(1.0 - rho * rho) * eps[k]
    t = np.arange(days, dtype=np.float64)
    K = sd * sd * np.exp(-np.abs(t[:, None] - t[None, :]) / ell)
    obs = np.round(np.linspace(0, days - 1, nobs)).astype(int)
    Ko = K[:, obs]
    cov = K - Ko @ np.linalg.solve(K[np.ix_(obs, obs)] + noise * np.eye(nobs), Ko.T)
    return 0.3 * flowsd * z, 0.5 * (cov + cov.T), np.exp(flowsd * z)
