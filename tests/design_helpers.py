"""References shared by the monitoring-design tests (tests/test_design_cpu.py, tests/test_gpu_design.py), numpy only: the
gain map by the DIRECT double sum sum A_i A_j expm1(s^2 b_i b_j) (never the series), conditioning by a DENSE SOLVE
C[:, S] (C_SS + D)^-1 C[S, :] (never the recurrence), the value V(S) of a design and a greedy selection built on them, and
the oracle-backed plan double."""
from __future__ import annotations

import numpy as np

from tests.flux_helpers import FluxOraclePlan


def explained_cov(C, S, tau2):
    """R = C[:, S] (C_SS + diag(tau2_S))^-1 C[S, :] by a dense solve; S may repeat a day (replicate samples)."""
    C = np.asarray(C, np.float64)
    S = np.asarray(S, dtype=np.int64).reshape(-1)
    if S.size == 0:
        return np.zeros_like(C)
    G = C[np.ix_(S, S)] + np.diag(np.asarray(tau2, np.float64)[S])
    return C[:, S] @ np.linalg.solve(G, C[S, :])


def rows_by_cholesky(C, S, tau2):
    """Conditioning rows B = L^-1 C[S, :], L L^T = C_SS + D: B^T B = ``explained_cov`` -- what a test hands the kernel."""
    C = np.asarray(C, np.float64)
    S = np.asarray(S, dtype=np.int64).reshape(-1)
    G = C[np.ix_(S, S)] + np.diag(np.asarray(tau2, np.float64)[S])
    return np.linalg.solve(np.linalg.cholesky(G), C[S, :])


def direct_gain(C, a, s2, groups, P, tau2=None, S=(), chunk=16):
    """gain (P, m) and v' (m,) of one more sample on every day c after the samples S, by the direct double sum on the dense
    SYMMETRIC covariance C (m, m): C' = C - ``explained_cov``, v'_c = C'_cc + tau2_c, b_ic = C'_ic / sqrt(v'_c),
    gain[p, c] = sum_{i,j in p} a_i a_j expm1(s2 b_ic b_jc); a candidate with v'_c not > 0 has gain 0 and v' 0."""
    C = np.asarray(C, np.float64)
    m = C.shape[0]
    a, g = np.asarray(a, np.float64), np.asarray(groups).astype(np.int64)
    tau2 = np.zeros(m) if tau2 is None else np.asarray(tau2, np.float64)
    Cc = C - explained_cov(C, S, tau2)
    v = np.diagonal(Cc) + tau2
    live = v > 0
    b = Cc * np.where(live, 1.0 / np.sqrt(np.where(live, v, 1.0)), 0.0)[None, :]  # b[i, c]
    gain = np.zeros((P, m))
    for p in range(P):
        idx = np.nonzero(g == p)[0]
        if not idx.size:
            continue
        ap = a[idx]
        for c0 in range(0, m, chunk):
            bp = b[idx, c0:c0 + chunk]
            E = np.expm1(s2 * bp[:, None, :] * bp[None, :, :])
            gain[p, c0:c0 + chunk] = np.einsum("i,ijc,j->c", ap, E, ap)
    return gain, np.where(live, v, 0.0)


def linear_gain(C, a, s2, groups, P, tau2=None, S=()):
    """The linear target's closed form s2 (sum_{i in p} a_i b_ic)^2 (the kernel at nterms = 1)."""
    C = np.asarray(C, np.float64)
    m = C.shape[0]
    tau2 = np.zeros(m) if tau2 is None else np.asarray(tau2, np.float64)
    Cc = C - explained_cov(C, S, tau2)
    v = np.diagonal(Cc) + tau2
    live = v > 0
    b = Cc * np.where(live, 1.0 / np.sqrt(np.where(live, v, 1.0)), 0.0)[None, :]
    g = np.asarray(groups).astype(np.int64)
    A = np.zeros((m, P))
    A[np.nonzero(g >= 0)[0], g[g >= 0]] = 1.0
    return s2 * ((A * np.asarray(a, np.float64)[:, None]).T @ b) ** 2


def design_value_ref(C, a, s2, groups, P, S, tau2, log=True):
    """V(S) (P, P) = sum_{i in p, j in q} a_i a_j expm1(s2 R_ij) (log) or s2 sum a_i a_j R_ij (linear), R by the dense solve."""
    R = explained_cov(C, S, tau2)
    g = np.asarray(groups).astype(np.int64)
    A = np.zeros((len(g), P))
    A[np.nonzero(g >= 0)[0], g[g >= 0]] = 1.0
    WA = A * np.asarray(a, np.float64)[:, None]
    return WA.T @ (np.expm1(s2 * R) if log else s2 * R) @ WA


def greedy_ref(C, a, s2, groups, P, k, omega, tau2, log=True, allowed=None, given=(), replicates=False):
    """Greedy picks by the references above: at each step the gain map after the samples so far, the score omega @ gain,
    the largest allowed one.  -> (picks, [(best score, runner-up score)] per step)."""
    m = np.asarray(C).shape[0]
    allowed = np.ones(m, dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool).copy()
    S = [int(c) for c in given]
    if not replicates:
        allowed[S] = False
    picks, tops = [], []
    for _ in range(k):
        gain = direct_gain(C, a, s2, groups, P, tau2, S)[0] if log else linear_gain(C, a, s2, groups, P, tau2, S)
        score = np.where(allowed, np.asarray(omega) @ gain, -np.inf)
        rank = np.argsort(-score, kind="stable")
        picks.append(int(rank[0]))
        tops.append((float(score[rank[0]]), float(score[rank[1]])))
        S.append(int(rank[0]))
        if not replicates:
            allowed[rank[0]] = False
    return picks, tops


class DesignOraclePlan(FluxOraclePlan):
    """``FluxOraclePlan`` with ``sample_value`` by the direct double sum (unbatched): the rows it is handed only say WHICH
    covariance is meant -- R = rows^T rows is subtracted densely."""

    def sample_value(self, cov, m, a, scale2, groups, ngroups, obs_var=None, rows=None, nterms=None):
        import torch

        def arr(t):
            return None if t is None else torch.as_tensor(t).detach().cpu().double().numpy()

        C = arr(cov)[:m, :m]
        C = np.tril(C) + np.tril(C, -1).T
        if rows is not None and len(rows):
            B = arr(rows)
            C = C - B.T @ B
        fn = linear_gain if nterms == 1 else direct_gain
        out = fn(C, arr(a), float(scale2), arr(groups), ngroups, arr(obs_var))
        tau2 = np.zeros(m) if obs_var is None else arr(obs_var)
        v = np.diagonal(C) + tau2
        gain = out if nterms == 1 else out[0]
        return torch.tensor(gain), torch.tensor(np.where(v > 0, v, 0.0))
