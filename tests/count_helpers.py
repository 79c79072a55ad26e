"""Host restatements for the exceedance-count tests: the estimator of ``csrc/dgp_counts.hip`` in numpy / scipy, point for point
on the generators and shifts of the orthant sweep (``extremes_helpers.weights``), the closed forms it is held against, and an
oracle plan that answers ``path_counts`` on the host."""
from __future__ import annotations

import numpy as np
from scipy.special import comb, ndtr, ndtri

from tests.extremes_helpers import YMAX, make_oracle_plan, weights


def paths_ref(L, gen, shifts, npoints):
    """f[s, n, i] = sum_{j <= i} L_ij y_j, y = clamp(Phi^-1(w), -38, 38) through the lower half (w > 1/2 -> -Phi^-1(1 - w);
    w = 0 gives -38).  ``L``: (m, m), only its lower triangle is read.  -> (nshifts, npoints, m)."""
    L = np.tril(np.asarray(L, dtype=np.float64))
    m = L.shape[0]
    w = weights(np.asarray(gen, dtype=np.float64)[:m], np.asarray(shifts, dtype=np.float64)[:, :m], npoints)
    upper = w > 0.5
    with np.errstate(divide="ignore"):
        z = np.clip(ndtri(np.where(upper, 1.0 - w, w)), -YMAX, YMAX)
    return np.where(upper, -z, z) @ L.T


def counts_ref(L, thr, above, link, gen, shifts, npoints):
    """The two integer histograms of ``dgp_path_counts`` and how close any path comes to a threshold.
    ``thr``: (levels, m) centred thresholds (NaN never counts); ``link``: (m,) flags or None (no breaks; ``link[0]`` ignored).
    -> (count_hist, spell_hist) int32 (levels, nshifts, m + 1), and the smallest gap min |f_i - c_{l,i}| / sd_i over all
    paths, levels and points with a finite threshold (inf when there is none)."""
    L = np.tril(np.asarray(L, dtype=np.float64))
    m = L.shape[0]
    thr = np.asarray(thr, dtype=np.float64).reshape(-1, m)
    link = np.ones(m, dtype=bool) if link is None else np.asarray(link).reshape(-1) != 0
    f = paths_ref(L, gen, shifts, npoints)  # (S, N, m)
    S = f.shape[0]
    sd = np.sqrt(np.sum(L * L, axis=1))
    nlev = thr.shape[0]
    count_hist = np.zeros((nlev, S, m + 1), dtype=np.int32)
    spell_hist = np.zeros((nlev, S, m + 1), dtype=np.int32)
    gap = np.inf
    for l in range(nlev):
        with np.errstate(invalid="ignore"):
            e = f > thr[l] if above else f < thr[l]  # a comparison with NaN is False
            fin = np.isfinite(thr[l])
            if fin.any():
                gap = min(gap, float(np.min(np.abs(f[:, :, fin] - thr[l][fin]) / sd[fin])))
        N = e.sum(axis=2)
        cur = np.zeros(e.shape[:2], dtype=np.int64)
        best = np.zeros(e.shape[:2], dtype=np.int64)
        for i in range(m):
            cur = np.where(e[:, :, i], (cur + 1) if (i and link[i]) else 1, 0)
            best = np.maximum(best, cur)
        for s in range(S):
            count_hist[l, s] = np.bincount(N[s], minlength=m + 1)
            spell_hist[l, s] = np.bincount(best[s], minlength=m + 1)
    return count_hist, spell_hist, gap


def binomial_pmf(m, p):
    k = np.arange(m + 1)
    return comb(m, k) * p ** k * (1.0 - p) ** (m - k)


def longest_run_cdf(m, p):
    """P(longest run of successes <= r), r = 0 .. m, for m independent trials of probability p: a DP over the length of the
    current run, runs longer than r being absorbed."""
    out = np.zeros(m + 1)
    for r in range(m + 1):
        state = np.zeros(r + 1)  # state[j] = P(current run = j and no run has exceeded r)
        state[0] = 1.0
        for _ in range(m):
            new = np.zeros(r + 1)
            new[0] = (1.0 - p) * state.sum()
            new[1:] = p * state[:-1]
            state = new
        out[r] = state.sum()
    return out


def equicorrelated_count_pmf(m, rho, b, nodes=400):
    """The pmf of N = #{i : f_i > b}, f ~ N(0, (1 - rho) I + rho 11^T): C(m, k) int phi(z) p(z)^k (1 - p(z))^(m - k) dz with
    p(z) = 1 - Phi((b - sqrt(rho) z) / sqrt(1 - rho)), by Gauss-Legendre on [-9, 9]."""
    x, wq = np.polynomial.legendre.leggauss(nodes)
    z = 9.0 * x
    p = ndtr(-(b - np.sqrt(rho) * z) / np.sqrt(1.0 - rho))
    dens = 9.0 * wq * np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi)
    k = np.arange(m + 1)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        logt = k * np.log(p)[None, :] + (m - k) * np.log1p(-p)[None, :]
    logt = np.where(np.isnan(logt), -np.inf, logt)
    return comb(m, k[:, 0]) * (np.exp(logt) @ dens)


def make_count_oracle_plan():
    """``extremes_helpers.make_oracle_plan()``'s class with ``path_counts`` answered on the host by ``counts_ref`` on the
    product's own generators and shifts; the levels are split as the device path splits them (``path_count_level_chunks``),
    and every call's arguments, chunk sizes and smallest gap are kept in ``calls``."""
    import torch

    from discontinuum_amd.backend import orthant_shifts, path_count_level_chunks, richtmyer_generators

    class CountOraclePlan(make_oracle_plan()):
        calls = []

        def path_counts(self, L, m, thr, above=True, link=None, npoints=4096, nshifts=16, seed=0, max_bytes=None):
            thr = np.asarray(thr, dtype=np.float64).reshape(-1, m)
            per_call, _one = path_count_level_chunks(m, thr.shape[0], nshifts, npoints, max_bytes)
            gen, sh = richtmyer_generators(m), orthant_shifts(m, nshifts, seed).numpy()
            Lm = L.numpy()[:m, :m]
            parts = [counts_ref(Lm, thr[l0:l0 + per_call], above, link, gen, sh, npoints) for l0 in range(0, thr.shape[0], per_call)]
            type(self).calls.append(dict(m=m, thr=thr, above=above, link=None if link is None else np.asarray(link).copy(),
                                         per_call=per_call, gap=min(p[2] for p in parts), L=Lm.copy()))
            return (torch.from_numpy(np.concatenate([p[0] for p in parts])), torch.from_numpy(np.concatenate([p[1] for p in parts])))

    CountOraclePlan.calls = []
    return CountOraclePlan
