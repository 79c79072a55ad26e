"""Dense CPU restatement of the censored (Tobit) Laplace fit, for the CPU and GPU suites (TEST INFRASTRUCTURE).

Row i is observed (side 0: y_i, Gaussian, variance v_i) or censored at the limit l_i = y_i (side -1: the truth is below it,
+1: above): log p_i = log Phi(z_i), z_i = s_i (f_i - l_i) / sigma_i.  With h = phi(z) / Phi(z):
    g = s h / sigma,   W = h (z + h) / v,   d3 = -(s / sigma^3) h [1 - (z + h)(z + 2 h)]
(observed rows: W = 1 / v, d3 = 0).  Newton: n~ = 1 / W, y~ = f + g / W, a = (K + diag n~)^-1 (y~ - m), f_new = y~ - n~ o a.
The same guards as the library: erfcx forms for z < 0, erfc / log1p forms for z >= 0; a censored row with W v < 1e-12 is
capped (n~ = 1e12 v, d3 = 0); the first Newton step from the given f is taken whole, later ones are halved on
Psi = sum log p - 1/2 a^T (f - m) over t in {1, 1/2, .. 1/64}.  Gram matrices come from ``oracle.gp_oracle``.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from scipy import special

from discontinuum_amd import _lib
from oracle import gp_oracle as orc

from tests.helpers import OraclePlan

CAP = 1e-12
LOG2PI = math.log(2.0 * math.pi)
SQRT1_2 = math.sqrt(0.5)
STEPS = (1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625)


def pointwise(z):
    """-> (log Phi, h, h (z + h), h [1 - (z + h)(z + 2 h)]) of a float64 numpy array, in the library's formulation."""
    z = np.asarray(z, dtype=np.float64)
    neg = z < 0
    zn, zp = np.where(neg, z, -1.0), np.where(neg, 1.0, z)
    e = special.erfcx(-zn * SQRT1_2)
    tail = 0.5 * special.erfc(zp * SQRT1_2)
    h = np.where(neg, math.sqrt(2.0 / math.pi) / e, np.exp(-0.5 * zp * zp) / math.sqrt(2.0 * math.pi) / (1.0 - tail))
    logphi = np.where(neg, -0.5 * zn * zn + np.log(0.5 * e), np.log1p(-tail))
    zh = z + h
    return logphi, h, h * zh, h * (1.0 - zh * (zh + h))


def terms(f, y, side, v, m):
    """The terms kernel: dict of numpy vectors r~ (rt), n~ (nn), g, W, d3, logp, corr (the alpha-free part of the NLL
    correction per row) and the number of capped rows."""
    f, y, v, m = (np.asarray(t, dtype=np.float64) for t in (f, y, v, m))
    side = np.asarray(side)
    cens = side != 0
    sg, sd = np.sqrt(v), side.astype(np.float64)
    logphi, h, q, c3 = pointwise(np.where(cens, sd * (f - y) / sg, 0.0))
    capped = cens & ~(q >= CAP)
    nn = np.where(cens, np.where(capped, v / CAP, v / np.where(q > 0, q, 1.0)), v)
    W = 1.0 / nn
    g = np.where(cens, sd * h / sg, (y - f) / v)
    rt = np.where(cens, (f + g * nn) - m, y - m)
    d3 = np.where(cens & ~capped, -(sd / (sg * v)) * c3, 0.0)
    e = y - f
    logp = np.where(cens, logphi, -0.5 * e * e / v - 0.5 * np.log(2.0 * math.pi * v))
    corr = np.where(cens, -logphi + 0.5 * np.log(W) - 0.5 * LOG2PI, 0.0)
    return dict(rt=rt, nn=nn, g=g, W=W, d3=d3, logp=logp, corr=corr, capped=int(capped.sum()), cens=cens)


def _logp(f, y, side, v):
    return terms(f, y, side, v, np.zeros_like(f))["logp"]


def gram(model, X, theta):
    return orc.GRAMS[model](X, X, torch.as_tensor(theta, dtype=torch.float64)).detach().numpy()


def newton(K, y, side, v, m, f0=None, maxit=50, tol=1e-10):
    """The mode search on a dense K (numpy).  -> (f, iterations, final max |df|, halvings, converged)."""
    y, v, m = (np.asarray(t, dtype=np.float64) for t in (y, v, m))
    f = m.copy() if f0 is None else np.asarray(f0, dtype=np.float64).copy()
    acur = np.zeros_like(f)
    it, halvings, dmax = 0, 0, math.inf
    while True:
        tm = terms(f, y, side, v, m)
        anew = np.linalg.solve(K + np.diag(tm["nn"]), tm["rt"])
        delta = (m + tm["rt"] - tm["nn"] * anew) - f
        dmax = float(np.max(np.abs(delta)))
        t = 1.0
        if it > 0 and not dmax <= tol:
            def psi(t):
                ft, at = f + t * delta, acur + t * (anew - acur)
                return float(np.sum(_logp(ft, y, side, v) - 0.5 * at * (ft - m)))

            psi0 = psi(0.0)
            floor = psi0 - 1e-9 * (1.0 + abs(psi0))
            j = 0
            while j < len(STEPS) - 1 and not psi(STEPS[j]) >= floor:
                j += 1
            t, halvings = STEPS[j], halvings + j
        f = f + t * delta
        acur = acur + t * (anew - acur)
        it += 1
        if dmax <= tol:
            return f, it, dmax, halvings, True
        if it >= maxit:
            return f, it, dmax, halvings, False


def laplace(model, X, y, side, v, m, theta, f0=None, maxit=50, tol=1e-10, with_grad=True):
    """Everything ``dgp_laplace_fit_step`` returns, densely: dict with f, nll, dtheta, dr, u, alpha, rt, nn (torch / numpy
    float64), iterations, dmax, halvings, capped, converged, corr (NLL_L - NLL_engine)."""
    X = torch.as_tensor(X, dtype=torch.float64)
    theta = torch.as_tensor(theta, dtype=torch.float64).detach()
    y, v, m = (np.asarray(torch.as_tensor(t).detach().numpy() if torch.is_tensor(t) else t, dtype=np.float64) for t in (y, v, m))
    side = np.asarray(side.numpy() if torch.is_tensor(side) else side)
    K = gram(model, X, theta)
    if not (side != 0).any():
        f, it, dmax, halvings, conv = None, 0, 0.0, 0, True
        tm = terms(m, y, side, v, m)
    else:
        f, it, dmax, halvings, conv = newton(K, y, side, v, m, None if f0 is None else np.asarray(f0), maxit, tol)
        tm = terms(f, y, side, v, m)
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
        res.update(u=u, dtheta=g_theta.numpy() + bilinear(model, X, theta, u, a), dr=a - u)
    return res


def bilinear(model, X, theta, u, alpha):
    """u^T dK/dtheta_p alpha for every p: autograd on u^T K(theta) alpha with u and alpha detached."""
    th = torch.as_tensor(theta, dtype=torch.float64).detach().clone().requires_grad_(True)
    u, alpha = torch.as_tensor(u, dtype=torch.float64), torch.as_tensor(alpha, dtype=torch.float64)
    with torch.enable_grad():
        val = u @ (orc.GRAMS[model](torch.as_tensor(X, dtype=torch.float64), torch.as_tensor(X, dtype=torch.float64), th) @ alpha)
        (g,) = torch.autograd.grad(val, th)
    return g.numpy()


def nll_direct(res, y, side, v, m):
    """NLL_L by the textbook formula 1/2 a^T (f - m) - sum log p + 1/2 log |I + K W| at the mode in ``res``."""
    y, v, m = (np.asarray(t, dtype=np.float64) for t in (y, v, m))
    tm = terms(res["f"], y, side, v, m)
    a = res["alpha"]
    _sign, logdet = np.linalg.slogdet(np.eye(len(y)) + res["K"] * tm["W"][None, :])
    return float(0.5 * a @ (res["f"] - m) - tm["logp"].sum() + 0.5 * logdet)


def posterior(model, X, res, Xs, full_cov=False):
    """The Laplace posterior of the latent f at Xs (without the prior mean): the GP posterior of the pseudo-data."""
    return orc.posterior(model, torch.as_tensor(X, dtype=torch.float64), torch.tensor(res["rt"]), torch.tensor(res["nn"]), res["theta"],
                         torch.as_tensor(Xs, dtype=torch.float64), full_cov=full_cov)


def scalar_mode(k, limit, s, v, m):
    """n = 1, one censored row: the root of d/df [log Phi(s (f - l) / sigma) - (f - m)^2 / (2 k)] by bisection."""
    sg = math.sqrt(v)

    def slope(f):
        h = pointwise(np.array([s * (f - limit) / sg]))[1][0]
        return s * h / sg - (f - m) / k

    lo, hi = m - 50.0 * math.sqrt(k) - 50.0, m + 50.0 * math.sqrt(k) + 50.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if slope(mid) > 0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def curve(X):
    """The smooth generating curve of the fixtures (small against sigma = 0.1, so that no limit is uninformative)."""
    X = np.asarray(X, dtype=np.float64)
    return 0.15 * np.tanh(X[:, -1]) + 0.05 * np.sin(X[:, 0] / 4.0)


def synth(X, frac, seed, sigma=0.1, sides=(-1, 1), ends=True, mean=0.02):
    """Samples y = curve(X) + sigma eps on the rows of X with about ``frac`` of them censored (rows 0 and n - 1 among them when
    ``ends``), the limits within +-2 sigma of the curve.  -> (y with the limits in place, side int32, v, m) as numpy arrays."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    rng = np.random.default_rng(seed)
    c = curve(X)
    y = c + sigma * rng.standard_normal(n)
    k = min(n, max(1, int(round(frac * n))))
    idx = set(rng.choice(n, size=k, replace=False).tolist())
    if ends and n > 1 and frac < 1.0:
        idx |= {0, n - 1}
    side = np.zeros(n, dtype=np.int32)
    for j, i in enumerate(sorted(idx)):
        side[i] = sides[j % len(sides)]
        y[i] = c[i] + sigma * rng.uniform(-2.0, 2.0)
    return y, side, np.full(n, sigma * sigma), np.full(n, mean)


class LaplaceOraclePlan(OraclePlan):
    """``OraclePlan`` with the censored entry points of ``backend.GPPlan``, answered by ``laplace`` above."""

    def _laplace(self, with_grad, theta, y, mean, noise, side, f, maxit, tol):
        self.laplace_calls = getattr(self, "laplace_calls", 0) + 1
        theta = torch.as_tensor(theta, dtype=torch.float64).detach()
        out = torch.zeros(_lib.OUT_LEN, dtype=self.dtype)
        try:
            res = laplace(self.model, self.X, y.detach(), side, noise.detach(), mean.detach(), theta,
                          None if f is None else f.detach().numpy(), maxit, tol, with_grad=with_grad)
        except (torch.linalg.LinAlgError, np.linalg.LinAlgError):
            out[_lib.OUT_NLL], out[_lib.OUT_INFO] = float("nan"), 1
            zero = torch.zeros(self.n, dtype=self.dtype)
            stat = (0.0, float("inf"), 0.0, 0.0)
            return (out, zero, mean.detach().clone(), stat) if with_grad else (out, mean.detach().clone(), stat)
        self._state = (theta, torch.tensor(res["rt"]), torch.tensor(res["nn"]))
        self.laplace_stat = (float(res["iterations"]), res["dmax"], float(res["halvings"]), float(res["capped"]))
        if not res["converged"]:
            raise _lib.DGPError(_lib.E_NOCONV, "dgp_laplace_fit_step", "the mode search did not converge")
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

    def laplace_fit_step(self, theta, y, mean, noise, side, f=None, maxit=50, tol=1e-10):
        self.calls += 1
        return self._laplace(True, theta, y, mean, noise, side, f, maxit, tol)

    def laplace_factorize(self, theta, y, mean, noise, side, f=None, maxit=50, tol=1e-10):
        return self._laplace(False, theta, y, mean, noise, side, f, maxit, tol)
