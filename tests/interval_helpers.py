"""Dense CPU restatement of the Laplace fit with INTERVAL-censored rows, for the CPU and GPU suites (TEST INFRASTRUCTURE).

Extends tests/censored_helpers.py by the fourth row kind, side 2: the truth of row i lies in [y_i, upper_i].  With
za = (y - f) / sigma, zb = (upper - f) / sigma, Delta = zb - za, P = Phi(zb) - Phi(za), ra = phi(za) / P, rb = phi(zb) / P:
    log p = log P,   g = (ra - rb) / sigma,   W v = zb rb - za ra + (ra - rb)^2,
    sigma^3 d3 = ra (za^2 - 1) - rb (zb^2 - 1) - (ra - rb)(za ra - zb rb) + 2 (ra - rb) W v
-- mean, one minus the variance and the third central moment of a standard normal truncated to [za, zb].  The same three
regimes and guards as the library (dgp_censored.hip): a bracket whose centre lies right of 0 is reflected; then
    narrow    Delta <= 2 and Delta |c| <= 4 (c the centre): 12-point Gauss-Legendre moments of exp(-c h t - h^2 t^2 / 2) on [-1, 1],
              central moments about the computed mean (no cancellation as Delta -> 0)
    tail      zb <= 0: Mills ratios through erfcx, phi(za) / phi(zb) = exp(Delta c) through exp / expm1
    straddle  za < 0 < zb: P = [erf(zb / sqrt 2) + erf(-za / sqrt 2)] / 2, a sum of positive terms
and the capping rule W v < 1e-12 -> n~ = 1e12 v, d3 = 0.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from scipy import special

from tests import censored_helpers as ch

SQRT1_2 = math.sqrt(0.5)
LOGSQRT2PI = 0.5 * math.log(2.0 * math.pi)
GL_T, GL_W = np.polynomial.legendre.leggauss(12)
NARROW_H, NARROW_A = 1.0, 2.0


def interval_pointwise(za, delta):
    """-> (log P, sigma g, W v, sigma^3 d3) of float64 arrays za, Delta > 0, in the library's formulation."""
    za, delta = np.broadcast_arrays(np.asarray(za, dtype=np.float64), np.asarray(delta, dtype=np.float64))
    zb = za + delta
    flip = za + zb > 0.0
    a = np.where(flip, -zb, za)  # the reflected bracket [a, b], centre c <= 0
    b = np.where(flip, -za, zb)
    h = 0.5 * delta
    c = np.where(flip, -(za + h), za + h)
    narrow = (h <= NARROW_H) & (np.abs(c) * h <= NARROW_A)
    tail = ~narrow & (b <= 0.0)
    with np.errstate(all="ignore"):
        # narrow: moments of w(t) = exp(-c h t - h^2 t^2 / 2) over t in [-1, 1]
        wt = GL_W * np.exp(-(c * h)[..., None] * GL_T - (0.5 * h * h)[..., None] * GL_T * GL_T)
        tot = wt.sum(-1)
        m1 = (wt * GL_T).sum(-1) / tot
        dt = GL_T - m1[..., None]
        m2 = (wt * dt * dt).sum(-1) / tot
        m3 = (wt * dt * dt * dt).sum(-1) / tot
        n_logp = np.log(h) - 0.5 * c * c - LOGSQRT2PI + np.log(tot)
        n_mu, n_wv, n_d3 = c + h * m1, 1.0 - h * h * m2, h * h * h * m3
        # tail: b <= 0.  P = phi(b) D, D = M(b) - rho M(a), M = Phi / phi, rho = phi(a) / phi(b) = exp(Delta c)
        at, bt = np.where(tail, a, -1.0), np.where(tail, b, -0.5)
        ma = math.sqrt(0.5 * math.pi) * special.erfcx(-at * SQRT1_2)
        mb = math.sqrt(0.5 * math.pi) * special.erfcx(-bt * SQRT1_2)
        e1 = np.expm1(np.where(tail, delta * c, -1.0))
        rho = 1.0 + e1
        D = mb - rho * ma
        t_logp = -0.5 * bt * bt - LOGSQRT2PI + np.log(D)
        # straddle: a < 0 < b
        P = 0.5 * (special.erf(b * SQRT1_2) + special.erf(-a * SQRT1_2))
        phia, phib = np.exp(-0.5 * a * a - LOGSQRT2PI), np.exp(-0.5 * b * b - LOGSQRT2PI)
        ra = np.where(tail, rho / D, phia / P)
        rb = np.where(tail, 1.0 / D, phib / P)
        mu = np.where(tail, e1 / D, ra - rb)
        aw, bw = np.where(tail, at, a), np.where(tail, bt, b)
        wv = np.minimum(bw * rb - aw * ra + mu * mu, 1.0)
        d3 = ra * (aw * aw - 1.0) - rb * (bw * bw - 1.0) - mu * (aw * ra - bw * rb) + 2.0 * mu * wv
        logp = np.where(narrow, n_logp, np.where(tail, t_logp, np.log(P)))
        mu = np.where(narrow, n_mu, mu)
        wv = np.where(narrow, n_wv, wv)
        d3 = np.where(narrow, n_d3, d3)
    sgn = np.where(flip, -1.0, 1.0)
    return logp, sgn * mu, wv, sgn * d3


def terms(f, y, side, v, m, upper=None):
    """``censored_helpers.terms`` with the rows of side 2 (the truth in [y, upper]) added."""
    f, y, v, m = (np.asarray(t, dtype=np.float64) for t in (f, y, v, m))
    side = np.asarray(side)
    br = side == 2
    tm = ch.terms(f, y, np.where(br, 0, side), v, m)
    if not br.any():
        return tm
    upper = np.asarray(upper, dtype=np.float64)
    sg = np.sqrt(v)
    za = np.where(br, (y - f) / sg, 0.0)
    dl = np.where(br, (upper - y) / sg, 1.0)
    logp, mu, wv, d3 = interval_pointwise(za, dl)
    capped = br & ~(wv >= ch.CAP)
    nn = np.where(capped, v / ch.CAP, v / np.where(wv > 0, wv, 1.0))
    g = mu / sg
    W = 1.0 / nn
    out = dict(tm)
    out["nn"] = np.where(br, nn, tm["nn"])
    out["W"] = np.where(br, W, tm["W"])
    out["g"] = np.where(br, g, tm["g"])
    out["rt"] = np.where(br, (f + g * nn) - m, tm["rt"])
    out["d3"] = np.where(br, np.where(capped, 0.0, d3 / (sg * v)), tm["d3"])
    out["logp"] = np.where(br, logp, tm["logp"])
    out["corr"] = np.where(br, -logp + 0.5 * np.log(W) - 0.5 * ch.LOG2PI, tm["corr"])
    out["capped"] = tm["capped"] + int(capped.sum())
    out["cens"] = tm["cens"] | br
    return out


def newton(K, y, side, v, m, upper=None, f0=None, maxit=50, tol=1e-10):
    """``censored_helpers.newton`` with bracketed rows.  -> (f, iterations, final max |df|, halvings, converged)."""
    y, v, m = (np.asarray(t, dtype=np.float64) for t in (y, v, m))
    f = m.copy() if f0 is None else np.asarray(f0, dtype=np.float64).copy()
    acur = np.zeros_like(f)
    it, halvings, dmax = 0, 0, math.inf
    while True:
        tm = terms(f, y, side, v, m, upper)
        anew = np.linalg.solve(K + np.diag(tm["nn"]), tm["rt"])
        delta = (m + tm["rt"] - tm["nn"] * anew) - f
        dmax = float(np.max(np.abs(delta)))
        t = 1.0
        if it > 0 and not dmax <= tol:
            def psi(t):
                ft, at = f + t * delta, acur + t * (anew - acur)
                return float(np.sum(terms(ft, y, side, v, np.zeros_like(ft), upper)["logp"] - 0.5 * at * (ft - m)))

            psi0 = psi(0.0)
            floor = psi0 - 1e-9 * (1.0 + abs(psi0))
            j = 0
            while j < len(ch.STEPS) - 1 and not psi(ch.STEPS[j]) >= floor:
                j += 1
            t, halvings = ch.STEPS[j], halvings + j
        f = f + t * delta
        acur = acur + t * (anew - acur)
        it += 1
        if dmax <= tol:
            return f, it, dmax, halvings, True
        if it >= maxit:
            return f, it, dmax, halvings, False


def _np(t):
    return np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t)


def laplace(model, X, y, side, v, m, theta, upper=None, f0=None, maxit=50, tol=1e-10, with_grad=True):
    """``censored_helpers.laplace`` with bracketed rows: everything ``dgp_laplace_interval_fit_step`` returns, densely."""
    from oracle import gp_oracle as orc

    X = torch.as_tensor(X, dtype=torch.float64)
    theta = torch.as_tensor(theta, dtype=torch.float64).detach()
    y, v, m = (_np(t).astype(np.float64) for t in (y, v, m))
    side = _np(side)
    upper = None if upper is None else _np(upper).astype(np.float64)
    K = ch.gram(model, X, theta)
    if not (side != 0).any():
        f, it, dmax, halvings, conv = None, 0, 0.0, 0, True
        tm = terms(m, y, side, v, m, upper)
    else:
        f, it, dmax, halvings, conv = newton(K, y, side, v, m, upper, None if f0 is None else np.asarray(f0), maxit, tol)
        tm = terms(f, y, side, v, m, upper)
    rt, nn = torch.tensor(tm["rt"]), torch.tensor(tm["nn"])
    with torch.enable_grad():
        val, g_theta, alpha, g_noise = orc.nll_data_and_grads(model, X, rt, nn, theta)
    a = alpha.numpy()
    if f is None:
        f = m + tm["rt"] - tm["nn"] * a
    corr = float(np.sum(np.where(tm["cens"], tm["corr"] - 0.5 * tm["nn"] * a * a, 0.0)))
    res = dict(f=f, nll=float(val) + corr, nll_engine=float(val), corr=corr, alpha=a, rt=tm["rt"], nn=tm["nn"], iterations=it, dmax=dmax,
               halvings=halvings, capped=tm["capped"], converged=conv, theta=theta, K=K, terms=tm)
    if with_grad:
        kii = 2.0 * g_noise.numpy() + a * a
        t = -0.5 * (tm["nn"] - tm["nn"] ** 2 * kii) * tm["d3"]
        u = np.linalg.solve(K + np.diag(tm["nn"]), tm["nn"] * t)
        res.update(u=u, dtheta=g_theta.numpy() + ch.bilinear(model, X, theta, u, a), dr=a - u)
    return res


def nll_of_theta(model, X, y, side, v, m, theta, upper, tol=1e-13):
    """The Laplace NLL alone at ``theta`` (for central differences)."""
    return laplace(model, X, y, side, v, m, theta, upper, tol=tol, with_grad=False)["nll"]


def scalar_mode(k, lo_lim, hi_lim, v, m):
    """n = 1, one bracketed row: the root of d/df [log P(f) - (f - m)^2 / (2 k)] by bisection."""
    sg = math.sqrt(v)

    def slope(f):
        mu = interval_pointwise(np.array([(lo_lim - f) / sg]), np.array([(hi_lim - lo_lim) / sg]))[1][0]
        return mu / sg - (f - m) / k

    lo, hi = m - 50.0 * math.sqrt(k) - 50.0, m + 50.0 * math.sqrt(k) + 50.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if slope(mid) > 0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def synth(X, frac, seed, sigma=0.1, mean=0.02):
    """``censored_helpers.synth`` with the censored rows cycling through the kinds -1, +1 and 2; a bracket is [l, l + w sigma]
    with w in {0.05, 0.5, 1.5, 4} around the curve.  -> (y, side int32, v, m, upper) -- upper is NaN off the bracketed rows."""
    y, side, v, m = ch.synth(X, frac, seed, sigma=sigma, sides=(2, -1, 1), mean=mean)
    rng = np.random.default_rng(seed + 1000)
    upper = np.full(len(y), np.nan)
    widths = (0.05, 0.5, 1.5, 4.0)
    for j, i in enumerate(np.flatnonzero(side == 2)):
        w = widths[j % len(widths)] * sigma
        y[i] = y[i] - w * rng.uniform(0.2, 0.8)
        upper[i] = y[i] + w
    return y, side, v, m, upper


class IntervalOraclePlan(ch.LaplaceOraclePlan):
    """``LaplaceOraclePlan`` whose censored entry points take ``upper`` as ``backend.GPPlan``'s do."""

    def _laplace(self, with_grad, theta, y, mean, noise, side, f, maxit, tol, upper=None):
        if upper is None:
            return super()._laplace(with_grad, theta, y, mean, noise, side, f, maxit, tol)
        from discontinuum_amd import _lib

        self.laplace_calls = getattr(self, "laplace_calls", 0) + 1
        self.interval_calls = getattr(self, "interval_calls", 0) + 1
        theta = torch.as_tensor(theta, dtype=torch.float64).detach()
        out = torch.zeros(_lib.OUT_LEN, dtype=self.dtype)
        try:
            res = laplace(self.model, self.X, y.detach(), side, noise.detach(), mean.detach(), theta, upper.detach(),
                          None if f is None else f.detach().numpy(), maxit, tol, with_grad=with_grad)
        except (torch.linalg.LinAlgError, np.linalg.LinAlgError):
            out[_lib.OUT_NLL], out[_lib.OUT_INFO] = float("nan"), 1
            zero = torch.zeros(self.n, dtype=self.dtype)
            stat = (0.0, float("inf"), 0.0, 0.0)
            return (out, zero, mean.detach().clone(), stat) if with_grad else (out, mean.detach().clone(), stat)
        self._state = (theta, torch.tensor(res["rt"]), torch.tensor(res["nn"]))
        self.laplace_stat = (float(res["iterations"]), res["dmax"], float(res["halvings"]), float(res["capped"]))
        if not res["converged"]:
            raise _lib.DGPError(_lib.E_NOCONV, "dgp_laplace_interval_fit_step", "the mode search did not converge")
        out[_lib.OUT_NLL] = res["nll"]
        f_hat = torch.tensor(res["f"], dtype=self.dtype)
        if not with_grad:
            return out, f_hat, self.laplace_stat
        dr = torch.tensor(res["dr"], dtype=self.dtype)
        out[_lib.OUT_DTHETA:_lib.OUT_DTHETA + self.ntheta] = torch.tensor(res["dtheta"])
        out[_lib.OUT_SUM_DR] = dr.sum()
        if getattr(self, "_dr_w", None) is not None:
            out[_lib.OUT_DR_W0] = (dr * self._dr_w[0]).sum()
            out[_lib.OUT_DR_W0 + 1] = (dr * self._dr_w[1]).sum()
        return out, dr, f_hat, self.laplace_stat

    def laplace_fit_step(self, theta, y, mean, noise, side, f=None, maxit=50, tol=1e-10, upper=None):
        self.calls += 1
        return self._laplace(True, theta, y, mean, noise, side, f, maxit, tol, upper)

    def laplace_factorize(self, theta, y, mean, noise, side, f=None, maxit=50, tol=1e-10, upper=None):
        return self._laplace(False, theta, y, mean, noise, side, f, maxit, tol, upper)


class BatchedIntervalOraclePlan(IntervalOraclePlan):
    """``censored_batched_helpers.BatchedLaplaceOraclePlan`` with ``upper``: one ``IntervalOraclePlan`` per site."""

    laplace_calls_total = 0

    def __init__(self, model, n, d, dtype=torch.float64, device="cpu", lookahead=True, batch=1):
        super().__init__(model, n, d, dtype=dtype, device=device, lookahead=lookahead, batch=batch)
        if self.batch > 1:
            self._sites = [IntervalOraclePlan(model, n, d, dtype) for _ in range(self.batch)]

    def _laplace(self, with_grad, theta, y, mean, noise, side, f, maxit, tol, upper=None):
        from discontinuum_amd import _lib

        BatchedIntervalOraclePlan.laplace_calls_total += 1
        if not self._sites:
            return super()._laplace(with_grad, theta, y, mean, noise, side, f, maxit, tol, upper)
        self.laplace_calls = getattr(self, "laplace_calls", 0) + 1
        if upper is not None:
            self.interval_calls = getattr(self, "interval_calls", 0) + 1
        n = self.n
        outs, drs, fs, stats = [], [], [], []
        for b, p in enumerate(self._sites):
            nb = self._sizes[b]
            pad = lambda v, fill=0.0: torch.cat([v, torch.full((n - v.shape[0],), fill, dtype=v.dtype)])  # noqa: E731
            res = p._laplace(with_grad, theta[b], y[b, :nb], mean[b, :nb], noise[b, :nb], side[b, :nb], None if f is None else f[b, :nb],
                             maxit, tol, None if upper is None else upper[b, :nb])
            stat = res[-1] if np.any(np.asarray(side[b, :nb]) != 0) else (0.0, 0.0, 0.0, 0.0)
            outs.append(res[0])
            if with_grad:
                drs.append(pad(res[1]))
            tail = mean[b, nb:] if f is None else f[b, nb:]
            fs.append(torch.cat([res[-2], tail.detach().to(res[-2].dtype)]))
            stats.append(tuple(float(v) for v in stat))
        self.laplace_stat = tuple(stats)
        out, f_hat = torch.stack(outs), torch.stack(fs)
        return (out, torch.stack(drs), f_hat, self.laplace_stat) if with_grad else (out, f_hat, self.laplace_stat)

    def factorize(self, theta, r, noise):
        if not self._sites:
            return super().factorize(theta, r, noise)
        return torch.stack([p.factorize(theta[b], r[b, : self._sizes[b]], noise[b, : self._sizes[b]]) for b, p in enumerate(self._sites)])

    def predict(self, theta, Xs, chunk=4096):
        if not self._sites:
            return super().predict(theta, Xs, chunk)
        rows = [p.predict(theta[b], Xs[b]) for b, p in enumerate(self._sites)]
        return torch.stack([mu for mu, _ in rows]), torch.stack([var for _, var in rows])
