"""References shared by the exceedance tests (tests/test_exceedance_cpu.py, tests/test_gpu_exceedance.py): the pair
function D(h, k, rho) = Phi2(h, k; rho) - Phi(h) Phi(k) by Owen's T function, the dense moments built on it, the design
set of the pair function and the oracle-backed plan double.  Pure numpy / scipy."""
from __future__ import annotations

import numpy as np
from scipy.special import ndtr, owens_t

from tests.flux_helpers import FluxOraclePlan

Z_DET = 38.0  # |z| beyond which a point counts as decided: Phi(-38) = 3e-316, below every bound here


def _owen_a(x, y, rho, s):
    """a = (y - rho x) / (x sqrt(1 - rho^2)) with the +-inf limit at x = 0 (sign of y; both zero: the h = k -> 0 limit)."""
    num = y - rho * x
    with np.errstate(divide="ignore", invalid="ignore"):
        a = num / (x * s)
    zero = x == 0
    both = zero & (y == 0)
    a = np.where(zero, np.where(y > 0, np.inf, -np.inf), a)
    return np.where(both, np.sqrt((1 - rho) / (1 + rho)), a)


def bvn_excess_ref(h, k, rho):
    """D(h, k, rho) = Phi2(h, k; rho) - Phi(h) Phi(k), vectorised:
    Phi2 = Phi(h)/2 + Phi(k)/2 - T(h, a_h) - T(k, a_k) - beta, a_h = (k - rho h) / (h sqrt(1 - rho^2)), a_k likewise,
    beta = 0 if h k > 0, or h k = 0 and h + k >= 0, else 1/2; |rho| = 1 by the closed forms; a point with |z| > 38
    (infinite ones included) is decided and gives 0; NaN in -> NaN out otherwise."""
    h, k, rho = np.broadcast_arrays(np.asarray(h, np.float64), np.asarray(k, np.float64), np.asarray(rho, np.float64))
    rho = np.where(rho > 1, 1.0, np.where(rho < -1, -1.0, rho))
    ph, pk = ndtr(h), ndtr(k)
    inner = np.abs(rho) < 1
    r = np.where(inner, rho, 0.0)
    hh, kk = np.where(np.isfinite(h), h, 0.0), np.where(np.isfinite(k), k, 0.0)
    s = np.sqrt((1 - r) * (1 + r))
    beta = np.where((hh * kk > 0) | ((hh * kk == 0) & (hh + kk >= 0)), 0.0, 0.5)
    phi2 = 0.5 * ndtr(hh) + 0.5 * ndtr(kk) - owens_t(hh, _owen_a(hh, kk, r, s)) - owens_t(kk, _owen_a(kk, hh, r, s)) - beta
    d = phi2 - ndtr(hh) * ndtr(kk)
    d = np.where(rho >= 1, np.minimum(ph, pk) - ph * pk, d)
    d = np.where(rho <= -1, np.maximum(0.0, ph + pk - 1.0) - ph * pk, d)
    d = np.where(np.isnan(h) | np.isnan(k) | np.isnan(rho), np.nan, d)
    return np.where((np.abs(h) > Z_DET) | (np.abs(k) > Z_DET), 0.0, d)


def model_space_z(mu, var, thresh):
    """z (L, m) = (mu - u) / sigma with the decided cases: var <= 0 or u = +-inf -> +-inf (a tie mu = u with var <= 0 is
    "not exceeded": -inf); NaN stays NaN."""
    mu, var, u = np.asarray(mu, np.float64)[None, :], np.asarray(var, np.float64)[None, :], np.asarray(thresh, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (mu - u) / np.sqrt(var)
    decided = (var <= 0) | np.isinf(u)
    zd = np.where(np.isnan(mu) | np.isnan(u), np.nan, np.where(mu > u, np.inf, -np.inf))
    return np.where(decided, zd, z)


def dense_exceedance_moments(cov, mu, thresh, w, groups, P, extra_var=None):
    """Exact mean (L, P) and covariance (L, P, P) of N_g = sum_{i in g} w_i 1[f_i > u_i], f ~ N(mu, cov), on a dense
    SYMMETRIC fp64 covariance (m, m): thresholds ``thresh`` (L, m) in model space, ``groups`` -1 = excluded,
    ``extra_var`` added to the variances only (rho's numerator stays cov_ij)."""
    cov = np.asarray(cov, np.float64)
    mu, w, g = np.asarray(mu, np.float64), np.asarray(w, np.float64), np.asarray(groups).astype(np.int64)
    thresh = np.asarray(thresh, np.float64).reshape(-1, mu.shape[0])
    keep = np.nonzero(g >= 0)[0]
    cov, mu, w, g, thresh = cov[np.ix_(keep, keep)], mu[keep], w[keep], g[keep], thresh[:, keep]
    m, L = len(keep), thresh.shape[0]
    var = np.diagonal(cov) + (0.0 if extra_var is None else np.asarray(extra_var, np.float64)[keep])
    z = model_space_z(mu, var, thresh)
    p = ndtr(z)
    with np.errstate(divide="ignore", invalid="ignore"):
        sinv = np.where(var > 0, 1.0 / np.sqrt(var), np.where(np.isnan(var), np.nan, 0.0))
    A = np.zeros((m, P))
    A[np.arange(m), g] = 1.0
    ii, jj = np.tril_indices(m, -1)
    rho = cov[ii, jj] * sinv[ii] * sinv[jj]
    mean, out = np.empty((L, P)), np.empty((L, P, P))
    for l in range(L):
        D = np.zeros((m, m))
        D[ii, jj] = bvn_excess_ref(z[l, ii], z[l, jj], rho)
        D = D + D.T
        D[np.arange(m), np.arange(m)] = p[l] * (1 - p[l])
        WA = A * w[:, None]
        mean[l] = p[l] @ WA
        c = WA.T @ D @ WA
        out[l] = 0.5 * (c + c.T)
    return mean, out


DESIGN_RHO = (0.0, 1e-8, 0.3, 0.75, 0.9249, 0.9251, 0.99, 0.9999, 1 - 1e-9, 1.0)


def design_set(n_per_rho, seed=0):
    """The pair function's design set: rho in +-DESIGN_RHO; (h, k) ~ N(0, 2^2), plus near-equal pairs k = h + 1e-3 xi,
    h = 0, k = 0 and |h| or |k| = 8.  -> (h, k, rho), each of length 2 len(DESIGN_RHO) n_per_rho (n_per_rho >= 16)."""
    rng = np.random.default_rng(seed)
    hs, ks, rs = [], [], []
    for r0 in DESIGN_RHO:
        for r in (r0, -r0):
            h, k = 2 * rng.standard_normal(n_per_rho), 2 * rng.standard_normal(n_per_rho)
            q = n_per_rho // 8
            k[:q] = h[:q] + 1e-3 * rng.standard_normal(q)
            h[q:q + 2], k[q + 2:q + 4] = 0.0, 0.0
            h[q + 4], k[q + 4] = 0.0, 0.0
            h[q + 5], h[q + 6], k[q + 7], k[q + 8] = 8.0, -8.0, 8.0, -8.0
            hs.append(h), ks.append(k), rs.append(np.full(n_per_rho, r))
    return np.concatenate(hs), np.concatenate(ks), np.concatenate(rs)


class ExceedOraclePlan(FluxOraclePlan):
    """``FluxOraclePlan`` with ``exceedance_moments`` by the dense reference (unbatched)."""

    def exceedance_moments(self, cov, m, mu, thresh, w, groups, ngroups, extra_var=None):
        import torch

        def arr(t):
            return None if t is None else torch.as_tensor(t).detach().cpu().double().numpy()

        C = arr(cov)[:m, :m]
        C = np.tril(C) + np.tril(C, -1).T
        mean, pc = dense_exceedance_moments(C, arr(mu), arr(thresh), arr(w), arr(groups), ngroups, arr(extra_var))
        return torch.tensor(mean), torch.tensor(pc)
