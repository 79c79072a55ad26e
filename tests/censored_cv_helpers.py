"""Dense CPU references for the cross-validation of censored fits by Laplace cavity folds (TEST INFRASTRUCTURE).

At the Laplace mode f the latent posterior is the GP posterior of the pseudo-data (y~ = m + r~, n~ = 1 / W).  The CAVITY of a
fold F is that posterior with the fold's Gaussian sites deleted: the GP conditioned on the pseudo-data of the rows R that stay,

    V_c  = K_FF - K_FR W_R^1/2 (I + W_R^1/2 K_RR W_R^1/2)^-1 W_R^1/2 K_RF,
    mu_c = m_F  + K_FR W_R^1/2 (I + W_R^1/2 K_RR W_R^1/2)^-1 W_R^1/2 r~_R

(``dense_cavity_cv``: deletion, in the W-form -- a capped row has W ~ 1e-12 / v and simply drops out; ``solve(K_RR + N~_R)``
would lose 1e-6 on it).  The device code never deletes anything: it uses G_F^-1 diag(W_F) Sigma_FF (``identity_cavity`` restates
that in numpy).  ``refit_cv`` is the truth the cavity approximates: Newton's mode search without the fold.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from scipy import special

from tests import censored_helpers as ch
from tests import interval_helpers as ih

PLANES = ("mu", "var", "lpd", "pit_lower", "pit_upper", "dlp", "tilt")


def _condition(K, F, R, W_R, rt_R, m_F):
    """Latent (mean, covariance) at the rows F given the pseudo-data (r~, 1 / W) of the rows R, in the W-form."""
    if len(R) == 0:
        return m_F.copy(), K[np.ix_(F, F)].copy()
    sw = np.sqrt(W_R)
    B = np.eye(len(R)) + sw[:, None] * K[np.ix_(R, R)] * sw[None, :]
    L = np.linalg.cholesky(B)
    A = np.linalg.solve(L, sw[:, None] * K[np.ix_(R, F)])
    z = np.linalg.solve(L, sw * rt_R)
    return m_F + A.T @ z, K[np.ix_(F, F)] - A.T @ A


def row_planes(mu, vc, y, side, v, upper, shift=0.0):
    """The per-row planes from the latent held-out mean / variance (numpy vectors over the same rows), with scipy."""
    mu, vc, y, v = (np.asarray(t, dtype=np.float64) for t in (mu, vc, y, v))
    side = np.asarray(side)
    up = np.full(len(y), np.nan) if upper is None else np.asarray(upper, dtype=np.float64)
    sp2 = vc + v
    sp = np.sqrt(sp2)
    za = (y - mu) / sp
    t = shift * sp
    br = side == 2
    dz = np.where(br, (up - y) / sp, 1.0)
    zb = np.where(br, (up - mu) / sp, 0.0)
    Pa, Pb = special.ndtr(za), special.ndtr(zb)
    with np.errstate(all="ignore"):
        lo_lp, hi_lp = special.log_ndtr(za), special.log_ndtr(-za)
        lo_h = np.exp(-0.5 * za * za - 0.5 * math.log(2 * math.pi) - lo_lp)
        hi_h = np.exp(-0.5 * za * za - 0.5 * math.log(2 * math.pi) - hi_lp)
        iv_lp, iv_mu, _wv, _d3 = ih.interval_pointwise(np.where(br, za, 0.0), dz)
        iv_lp_t = ih.interval_pointwise(np.where(br, za - t, 0.0), dz)[0]
        gauss = -0.5 * za * za - 0.5 * np.log(2 * math.pi * sp2)
        lpd = np.select([side == -1, side == 1, br], [lo_lp, hi_lp, iv_lp], gauss)
        dlp = np.select([side == -1, side == 1, br], [-lo_h / sp, hi_h / sp, iv_mu / sp], (y - mu) / sp2)
        tilt = np.select([side == -1, side == 1, br], [special.log_ndtr(za - t) - lo_lp, special.log_ndtr(t - za) - hi_lp, iv_lp_t - iv_lp], 0.0)
    if shift == 0.0:
        tilt = np.zeros_like(tilt)
    plo = np.select([side == -1], [0.0], Pa)
    phi = np.select([side == -1, side == 1, br], [Pa, 1.0, Pb], Pa)
    return dict(mu=mu, var=sp2, lpd=lpd, pit_lower=plo, pit_upper=phi, dlp=dlp, tilt=tilt)


def _scatter(n, rows):
    out = {k: np.zeros(n) for k in PLANES}
    for F, pl in rows:
        for k in PLANES:
            out[k][F] = pl[k]
    return out


def latent_cavity(K, y, side, v, m, f, groups, upper=None):
    """(mu_c, v_c) of the latent at every held-out row (0 elsewhere) by deletion in the W-form."""
    y, v, m, f = (np.asarray(t, dtype=np.float64) for t in (y, v, m, f))
    g = np.asarray(groups)
    tm = ih.terms(f, y, side, v, m, upper)
    mu, vc = np.zeros(len(y)), np.zeros(len(y))
    for fold in np.unique(g[g >= 0]):
        F, R = np.flatnonzero(g == fold), np.flatnonzero(g != fold)
        mF, cov = _condition(K, F, R, tm["W"][R], tm["rt"][R], m[F])
        mu[F], vc[F] = mF, np.diag(cov)
    return mu, vc


def dense_cavity_cv(K, y, side, v, m, f, groups, upper=None, shift=0.0):
    """Every plane of ``GPPlan.laplace_cross_validate`` (dict of (n,) numpy arrays, 0 where ``groups`` is -1) by dense deletion
    in the W-form and scipy's normal functions.  Independent of the identity the device code uses."""
    g = np.asarray(groups)
    side = np.asarray(side)
    y, v = np.asarray(y, dtype=np.float64), np.asarray(v, dtype=np.float64)
    mu, vc = latent_cavity(K, y, side, v, m, f, g, upper)
    H = np.flatnonzero(g >= 0)
    up = None if upper is None else np.asarray(upper)[H]
    return _scatter(len(y), [(H, row_planes(mu[H], vc[H], y[H], side[H], v[H], up, shift))])


def identity_cavity(K, y, side, v, m, f, groups, upper=None):
    """(mu_c, v_c) of the latent by the identity the device code uses, V_c = G_F^-1 diag(W_F) Sigma_FF and mu_c = f_F - V_c g_F
    with G = (K + N~)^-1 and Sigma = K - K G K (both through (I + W^1/2 K W^1/2)^-1), in numpy."""
    y, v, m, f = (np.asarray(t, dtype=np.float64) for t in (y, v, m, f))
    g = np.asarray(groups)
    tm = ih.terms(f, y, side, v, m, upper)
    W, grad = tm["W"], tm["g"]
    sw = np.sqrt(W)
    L = np.linalg.cholesky(np.eye(len(y)) + sw[:, None] * K * sw[None, :])
    T = np.linalg.solve(L, np.diag(sw))  # G = T^T T
    A = T @ K
    G, Sigma = T.T @ T, K - A.T @ A
    mu, vc = np.zeros(len(y)), np.zeros(len(y))
    for fold in np.unique(g[g >= 0]):
        F = np.flatnonzero(g == fold)
        Vc = np.linalg.solve(G[np.ix_(F, F)], W[F][:, None] * Sigma[np.ix_(F, F)])
        mu[F], vc[F] = f[F] - Vc @ grad[F], np.diag(Vc)
    return mu, vc


def refit_cv(K, y, side, v, m, f, groups, upper=None, shift=0.0, tol=1e-10):
    """The planes with every fold REFITTED: Newton's mode search on the rows outside the fold (warm-started at the full-data
    mode), then the fold conditioned on that mode's pseudo-data.  What the cavity approximates."""
    y, v, m, f = (np.asarray(t, dtype=np.float64) for t in (y, v, m, f))
    side, g = np.asarray(side), np.asarray(groups)
    up = None if upper is None else np.asarray(upper, dtype=np.float64)
    rows = []
    for fold in np.unique(g[g >= 0]):
        F, R = np.flatnonzero(g == fold), np.flatnonzero(g != fold)
        upR = None if up is None else up[R]
        if (side[R] != 0).any():
            fR, _it, _dmax, _halv, conv = ih.newton(K[np.ix_(R, R)], y[R], side[R], v[R], m[R], upR, f0=f[R], tol=tol)
            assert conv
        else:
            fR = m[R]  # (observed rows' terms do not depend on f)
        tm = ih.terms(fR, y[R], side[R], v[R], m[R], upR)
        mF, cov = _condition(K, F, R, tm["W"], tm["rt"], m[F])
        rows.append((F, row_planes(mF, np.diag(cov), y[F], side[F], v[F], None if up is None else up[F], shift)))
    return _scatter(len(y), rows)


def censored_fixture(X, seed, sigma=0.1):
    """The plan-level data of the GPU test: ``ch.synth(X, 0.3, seed)``; five of the censored rows become ``< L`` with
    L = curve + (7.6, 8, 9, 10, 12) sigma (uninformative limits: they end at the cap), a third of the censored rows become
    brackets of width (1e-3, 0.3, 2, 8) sigma.  -> (y, side int32, v, m, upper) with all four row kinds."""
    y, side, v, m = ch.synth(X, 0.3, seed, sigma=sigma)
    c = ch.curve(X)
    cens = np.flatnonzero(side != 0)
    assert len(cens) >= 12
    for k, i in zip((7.6, 8.0, 9.0, 10.0, 12.0), cens[1::5][:5]):
        side[i] = -1
        y[i] = c[i] + k * sigma
    capped = set(cens[1::5][:5].tolist())
    upper = np.full(len(y), np.nan)
    widths = (1e-3, 0.3, 2.0, 8.0)
    j = 0
    for i in cens[::3]:
        if int(i) in capped:
            continue
        side[i] = 2
        upper[i] = y[i] + widths[j % 4] * sigma
        j += 1
    assert (side == 2).sum() >= 4 and (side == 1).any() and (side == -1).any() and (side == 0).any()
    return y, side.astype(np.int32), v, m, upper


class LaplaceCVOraclePlan(ih.IntervalOraclePlan):
    """``IntervalOraclePlan`` that answers ``GPPlan.laplace_cross_validate`` from ``dense_cavity_cv``."""

    def laplace_cross_validate(self, theta, y, mean, noise, side, f, groups, upper=None, shift=0.0, max_group=None):
        self.cavity_calls = getattr(self, "cavity_calls", 0) + 1
        K = ch.gram(self.model, self.X, torch.as_tensor(theta, dtype=torch.float64).detach())
        np_ = lambda t: None if t is None else np.asarray(t.detach().cpu().numpy(), dtype=np.float64)  # noqa: E731
        g = np.asarray(torch.as_tensor(groups).numpy())
        res = dense_cavity_cv(K, np_(y), side.detach().cpu().numpy(), np_(noise), np_(mean), np_(f), g, np_(upper), float(shift))
        out = {k: torch.tensor(res[k], dtype=torch.float64) for k in PLANES}
        out["info"] = torch.zeros(int(g.max()) + 1, dtype=torch.int32)
        return out
