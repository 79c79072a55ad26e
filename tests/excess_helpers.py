"""References shared by the threshold-excess tests (tests/test_excess_cpu.py, tests/test_gpu_excess.py): the covariance of
the excesses (or deficits) of two lognormal points over their thresholds in the four-term form, with
Phi2 = ``bvn_excess_ref`` + Phi Phi from tests/exceedance_helpers.py, the dense period moments built on it and the
oracle-backed plan double.  Pure numpy / scipy."""
from __future__ import annotations

import numpy as np
from scipy.special import ndtr

from tests.exceedance_helpers import Z_DET, ExceedOraclePlan, bvn_excess_ref


def point_terms(mu, v, a, above=True):
    """Per point (m,) and level (L, m): the signed standardised distance h0 = sg (mu - a) / sigma (sg = +1 excess, -1
    deficit), kappa = tau exp(-M), sigma, M = mu + v / 2 and the clipped variance.  Decided points: v <= 0 or a = +-inf give
    h0 = +-inf by the sign of mu - a (a tie: no excess); a point with h0 + 2 sg sigma < -38 has no mass on the threshold's
    side (below 1e-300 of its scale): h0 = -inf, kappa = 0.  NaN stays NaN."""
    sg = 1.0 if above else -1.0
    mu, v = np.asarray(mu, np.float64), np.asarray(v, np.float64)
    a = np.asarray(a, np.float64).reshape(-1, mu.shape[0])
    vp = np.where(v > 0, v, np.where(np.isnan(v), np.nan, 0.0))
    sig, M = np.sqrt(vp), mu + 0.5 * vp
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        h = sg * (mu[None] - a) / sig[None]
        h = np.where((vp[None] <= 0) | np.isinf(a), np.where(mu[None] > a, sg * np.inf, -sg * np.inf), h)
        h = np.where(np.isnan(mu[None]) | np.isnan(a) | np.isnan(vp[None]), np.nan, h)
        kap = np.exp(a - M[None])
        none = h + 2 * sg * sig[None] < -Z_DET
    return np.where(none, -np.inf, h), np.where(none, 0.0, kap), sig, M, vp


def point_moments(h, kap, sig, vp, above=True):
    """Normalised mean E e / exp(M) = sg (Phi(h + sg sigma) - kappa Phi(h)) and variance Var e / exp(2 M) (the pair formula
    at i = j, rho = 1; 0 for a deterministic point)."""
    sg = 1.0 if above else -1.0
    with np.errstate(invalid="ignore", over="ignore"):
        a0, a1, a2 = ndtr(h), ndtr(h + sg * sig), ndtr(h + 2 * sg * sig)
        E = sg * (a1 - kap * a0)
        V = np.exp(vp) * a2 - 2 * kap * a1 + kap * kap * a0 - E * E
    return E, np.where((np.broadcast_to(vp, V.shape) > 0) | np.isnan(h), V, 0.0)


def pair_norm_ref(hi, ki, si, hj, kj, sj, rho, above=True):
    """Cov(e_i, e_j) / exp(M_i + M_j) in the four-term form
    exp(c) P11 - kappa_j P10 - kappa_i P01 + kappa_i kappa_j P00 - E_i E_j,  P_tu = Phi2(h_tu, k_tu; rho),
    h_tu = h0_i + sg (t sigma_i + u rho sigma_j), k_tu = h0_j + sg (u sigma_j + t rho sigma_i), c = rho sigma_i sigma_j."""
    sg = 1.0 if above else -1.0
    rho = np.clip(np.asarray(rho, np.float64), -1.0, 1.0)
    ec = np.exp(rho * si * sj)

    def args(t, u):
        return hi + sg * (t * si + u * rho * sj), hj + sg * (u * sj + t * rho * si)

    def D(t, u):  # Phi2 - Phi Phi, taken in the quadrant where both probabilities are small (Owen's form is accurate to an
        # absolute 1e-16 of the probabilities it combines): D(h, k; r) = D(-h, -k; r) = -D(h, -k; -r) = -D(-h, k; -r)
        h, k = args(t, u)
        fh, fk = np.where(h > 0, -1.0, 1.0), np.where(k > 0, -1.0, 1.0)
        return fh * fk * bvn_excess_ref(fh * h, fk * k, fh * fk * rho)

    def dphi(x, y):  # Phi(x) - Phi(y) from the tails that are small
        return np.where(x + y > 0, ndtr(-y) - ndtr(-x), ndtr(x) - ndtr(y))

    # Phi2 = D + Phi Phi in each term; of sum coef Phi(h) Phi(k) - E_i E_j the kappa_i kappa_j parts cancel exactly
    # (h10 = h1_i, k01 = h1_j, h00 = h0_i, k00 = h0_j), the rest is written with differences of Phi
    with np.errstate(invalid="ignore", over="ignore"):
        h11, k11 = args(1, 1)
        a1i, a1j = ndtr(hi + sg * si), ndtr(hj + sg * sj)
        dpart = ec * D(1, 1) - kj * D(1, 0) - ki * D(0, 1) + ki * kj * D(0, 0)
        bracket = (ec * ndtr(h11) * ndtr(k11) - a1i * a1j) - kj * a1i * dphi(args(1, 0)[1], hj) - ki * a1j * dphi(args(0, 1)[0], hi)
        return dpart + bracket


def pair_cov_ref(mi, vi, ai, mj, vj, aj, cij, above=True):
    """Cov((c_i - tau_i)^+, (c_j - tau_j)^+) -- ``above=False``: of the deficits -- for ln c ~ N((m_i, m_j), [[v_i, c_ij],
    [c_ij, v_j]]) and tau = exp(a), vectorised over pairs."""
    mi, vi, ai, mj, vj, aj, cij = (np.atleast_1d(np.asarray(x, np.float64)) for x in (mi, vi, ai, mj, vj, aj, cij))
    out = np.empty(np.broadcast(mi, vi, ai, mj, vj, aj, cij).shape)
    mi, vi, ai, mj, vj, aj, cij = np.broadcast_arrays(mi, vi, ai, mj, vj, aj, cij)
    for q in range(out.size):  # (point_terms works per record; the pairs here are unrelated points)
        h, kap, sig, M, _vp = point_terms([mi[q], mj[q]], [vi[q], vj[q]], [[ai[q], aj[q]]], above)
        rho = cij[q] * (1.0 / sig[0]) * (1.0 / sig[1]) if sig[0] > 0 and sig[1] > 0 else 0.0  # (the library's order)
        out[q] = np.exp(M[0] + M[1]) * pair_norm_ref(h[0, 0], kap[0, 0], sig[0], h[0, 1], kap[0, 1], sig[1], rho, above)
    return out


def dense_excess_moments(cov, mu, scale2, thresh, w, groups, P, above=True, extra_var=None):
    """Exact mean (L, P), covariance (L, P, P) and total (P,) of E_g = sum_{i in g} w_i (c_i - tau_i)^+ (``above=False``:
    (tau_i - c_i)^+), c = exp(f'), f' ~ N(mu, scale2 (cov + diag(extra_var))) with the MAPPED mean ``mu``, on a dense
    SYMMETRIC fp64 covariance (m, m); ``thresh`` (L, m) = ln tau, ``groups`` -1 = excluded.  total_g = sum w_i exp(M_i)."""
    cov = np.asarray(cov, np.float64)
    mu, w, g = np.asarray(mu, np.float64), np.asarray(w, np.float64), np.asarray(groups).astype(np.int64)
    thresh = np.asarray(thresh, np.float64).reshape(-1, mu.shape[0])
    keep = np.nonzero(g >= 0)[0]
    cov, mu, w, g, thresh = cov[np.ix_(keep, keep)], mu[keep], w[keep], g[keep], thresh[:, keep]
    m, L, s2 = len(keep), thresh.shape[0], float(scale2)
    var = s2 * (np.diagonal(cov) + (0.0 if extra_var is None else np.asarray(extra_var, np.float64)[keep]))
    h, kap, sig, M, vp = point_terms(mu, var, thresh, above)
    E, V = point_moments(h, kap, sig[None], vp[None], above)
    with np.errstate(divide="ignore", invalid="ignore"):
        sinv = np.where(var > 0, 1.0 / np.sqrt(var), np.where(np.isnan(var), np.nan, 0.0))
    W = w * np.exp(M)
    idx = [np.nonzero(g == p)[0] for p in range(P)]  # (sums per group, not matrix products: an infinite or NaN point stays in its group)
    ii, jj = np.tril_indices(m, -1)
    rho = s2 * cov[ii, jj] * sinv[ii] * sinv[jj]
    mean, out = np.empty((L, P)), np.empty((L, P, P))
    for l in range(L):
        N = np.zeros((m, m))
        N[ii, jj] = pair_norm_ref(h[l, ii], kap[l, ii], sig[ii], h[l, jj], kap[l, jj], sig[jj], rho, above)
        N = N + N.T
        N[np.arange(m), np.arange(m)] = V[l]
        with np.errstate(invalid="ignore"):
            mean[l] = [np.sum(E[l, ix] * W[ix]) for ix in idx]
            for p in range(P):
                for q in range(p, P):
                    out[l, p, q] = out[l, q, p] = W[idx[p]] @ N[np.ix_(idx[p], idx[q])] @ W[idx[q]]
    return mean, out, np.array([np.sum(W[ix]) for ix in idx])


def excess_scales(cov, mu, scale2, thresh, w, groups, P, extra_var=None):
    """Q (L, P) of the bounds: Q_g = sum_{i in g} q_i, q_i = w_i (exp(m_i + v_i) + tau_i) over the undecided points (v_i > 0)
    with a finite tau; a mean entry is held to 1e-13 Q_g, a covariance entry to 1e-11 Q_g Q_h."""
    mu, w, g = np.asarray(mu, np.float64), np.asarray(w, np.float64), np.asarray(groups).astype(np.int64)
    thresh = np.asarray(thresh, np.float64).reshape(-1, mu.shape[0])
    var = float(scale2) * (np.diagonal(np.asarray(cov, np.float64)) + (0.0 if extra_var is None else np.asarray(extra_var, np.float64)))
    Q = np.zeros((thresh.shape[0], P))
    for l in range(thresh.shape[0]):
        ok = (g >= 0) & (var > 0) & np.isfinite(thresh[l]) & np.isfinite(mu)
        q = np.abs(w[ok]) * (np.exp(mu[ok] + var[ok]) + np.exp(thresh[l, ok]))
        np.add.at(Q[l], g[ok], q)
    return Q


class ExcessOraclePlan(ExceedOraclePlan):
    """``ExceedOraclePlan`` with ``excess_moments`` by the dense reference (unbatched)."""

    def excess_moments(self, cov, m, mu, scale2, thresh, w, groups, ngroups, above=True, extra_var=None):
        import torch

        def arr(t):
            return None if t is None else torch.as_tensor(t).detach().cpu().double().numpy()

        C = arr(cov)[:m, :m]
        C = np.tril(C) + np.tril(C, -1).T
        mean, pc, total = dense_excess_moments(C, arr(mu), float(torch.as_tensor(scale2, dtype=torch.float64).reshape(-1)[0]), arr(thresh), arr(w),
                                               arr(groups), ngroups, above, arr(extra_var))
        return torch.tensor(mean), torch.tensor(pc), torch.tensor(total)
