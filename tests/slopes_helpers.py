"""Dense references for the posterior of the fit's input derivatives (tests/test_slopes_cpu.py, tests/test_gpu_slopes.py).

Cross planes.  The oracle's Gram functions are torch fp64 functions of the test inputs, so (D_q K)(X, x*) is their autograd
(forward-mode) derivative along column c_q of the test points; the oracle's ``clamp_min`` inside the distance gives the
correct 0 at coincident points.  Nothing of the oracle is changed.

Prior block.  D_a D'_b k(x, x') at x = x' CANNOT come from double autograd -- the same clamp zeroes the second derivative on
the diagonal -- so it is written here in closed form, independently of the device code: mixed second derivatives at 0 of
RBF 1 / l^2, Matern-3/2 3 / l^2, Matern-5/2 5 / (3 l^2), Periodic 4 pi^2 / (p^2 l), products by the Leibniz rule (first
derivatives of stationary factors vanish at 0), the rating's gates and log warp by the chain rule.  tests/test_slopes_cpu.py
checks these forms against the autograd mixed derivative slightly off the diagonal, where the clamp is inactive.

The rest is dense ``cholesky`` / ``solve_triangular``, as in ``terms_helpers.terms_reference``."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

from discontinuum_amd.pipeline import datetime_to_decimal_year
from discontinuum_amd.xr_compat import Dataset
from oracle import gp_oracle as orc
from tests.helpers import OraclePlan
from tests.terms_helpers import pack_cov, unpack_cov  # noqa: F401  (the packing is dgp_predict_terms')


def cross_planes(gram, X, Xs, theta, cols):
    """[K(X, X*), d K / d x*_{c_1}, ...]: (1 + len(cols)) matrices (n, m)."""
    planes = [gram(X, Xs, theta)]
    for c in cols:
        tangent = torch.zeros_like(Xs)
        tangent[:, c] = 1.0
        with fwAD.dual_level():
            _k, dk = fwAD.unpack_dual(gram(X, fwAD.make_dual(Xs, tangent), theta))
        planes.append(dk if dk is not None else torch.zeros_like(planes[0]))
    return planes


# ---- closed-form prior blocks: full (1 + d, 1 + d, m) over (value, every column) ------------------------------------------
def loadest_prior(theta, Xs):
    d, m = Xs.shape[1], Xs.shape[0]
    th = [float(v) for v in theta]
    B = torch.zeros(1 + d, 1 + d, m, dtype=torch.float64)
    os1, lp, per, lm, os2, os3 = th[0], th[1], th[2], th[3], th[4], th[4 + d]
    l2, l3 = th[5:5 + d - 1], th[5 + d:5 + 2 * d]
    B[0, 0] = os1 + os2 + os3
    B[1, 1] = os1 * (4 * math.pi ** 2 / (per ** 2 * lp) + 5 / (3 * lm ** 2)) + 3 * os3 / l3[0] ** 2
    for j in range(1, d):
        B[1 + j, 1 + j] = os2 / l2[j - 1] ** 2 + 3 * os3 / l3[j] ** 2
    return B


def rating_prior(theta, Xs):
    th = [float(v) for v in theta]
    s = Xs[:, 1].double()
    g = 1.0 / (1.0 + torch.exp(orc.GATE_A * (s - th[0])))
    dg = -orc.GATE_A * g * (1 - g)     # d gate / d stage
    h, dh = 1 - g, -dg                 # the inverted gate
    dw = 1.0 / (s + 1e-6)              # d log(stage + 1e-6) / d stage
    low0 = th[1] + th[4]
    low_tt = 3 * th[1] / th[3] ** 2 + 3 * th[4] / th[6] ** 2              # Matern-3/2 in time
    low_ww = 5 * th[1] / (3 * th[2] ** 2) + 5 * th[4] / (3 * th[5] ** 2)  # Matern-5/2 in log stage
    up0, up_ww, up_tt = th[7], 5 * th[7] / (3 * th[8] ** 2), 5 * th[7] / (3 * th[9] ** 2)
    base0, base_ww = th[10], 5 * th[10] / (3 * th[11] ** 2)
    per0 = th[12]
    per_tt = th[12] * (4 * math.pi ** 2 / (th[14] ** 2 * th[13]) + 5 / (3 * th[15] ** 2))
    B = torch.zeros(3, 3, Xs.shape[0], dtype=torch.float64)
    B[0, 0] = g * g * low0 + h * h * up0 + base0 + per0
    B[1, 1] = g * g * low_tt + h * h * up_tt + per_tt
    # d/ds' [g(s) g(s') A(w - w')] at s' = s: g g' A(0) (A'(0) = 0); d/ds d/ds': g'^2 A(0) + g^2 w'^2 (-A''(0))
    B[2, 0] = B[0, 2] = g * dg * low0 + h * dh * up0
    B[2, 2] = dg * dg * low0 + dh * dh * up0 + dw * dw * (g * g * low_ww + h * h * up_ww + base_ww)
    return B


def composite_prior(spec):
    spec = [int(v) for v in spec]

    def prior(theta, Xs):
        th = [float(v) for v in theta]
        d, m = spec[0], Xs.shape[0]
        B = torch.zeros(1 + d, 1 + d, m, dtype=torch.float64)
        i, t = 2, 0
        for _term in range(spec[1]):
            scaled, nfac = spec[i], spec[i + 1]
            i += 2
            os = 1.0
            if scaled:
                os = th[t]
                t += 1
            B[0, 0] += os
            for _f in range(nfac):
                kind, nu2, ard, nd = spec[i:i + 4]
                dims = spec[i + 4:i + 4 + nd]
                i += 4 + nd
                ls = [th[t + (j if ard else 0)] for j in range(nd)]
                t += nd if ard else 1
                for j, col in enumerate(dims):
                    if kind == 0:
                        w = 1 / ls[j] ** 2
                    elif kind == 1:
                        w = {1: float("inf"), 3: 3.0, 5: 5.0 / 3.0}[nu2] / ls[j] ** 2
                    else:
                        w = 4 * math.pi ** 2 / (th[t] ** 2 * ls[j])
                    B[1 + col, 1 + col] += os * w  # every other factor of the product is 1 at 0, its first derivative 0
                if kind == 2:
                    t += 1
        return B

    return prior


PRIORS = {"loadest": loadest_prior, "rating": rating_prior}


def autograd_prior_block(gram, theta, Xs, eps):
    """The block (1 + d, 1 + d, m) by autograd at x' = x + eps (one offset per column): k, d_x k, d_x' k and the mixed
    d_x d_x' k of the pairs (x_j, x'_j).  The distance clamp is inactive in every factor that sees a column with a nonzero
    offset -- and ACTIVE (second derivative zeroed) in a factor that sees none -- so an offset along one column e_c checks the
    entries over (value, c), and an offset in all columns the whole block; the closed forms hold up to O(eps / l)."""
    d, m = Xs.shape[1], Xs.shape[0]
    xa = Xs.clone().double().requires_grad_(True)
    xb = (Xs.clone().double() + torch.as_tensor(eps, dtype=torch.float64)).requires_grad_(True)
    k = torch.diagonal(gram(xa, xb, theta))
    B = torch.zeros(1 + d, 1 + d, m, dtype=torch.float64)
    B[0, 0] = k.detach()
    ga, gb = torch.autograd.grad(k.sum(), (xa, xb), create_graph=True)
    for a in range(d):
        B[1 + a, 0] = ga[:, a].detach()
        B[0, 1 + a] = gb[:, a].detach()
        mixed = torch.autograd.grad(ga[:, a].sum(), xb, retain_graph=True)[0]
        for b in range(d):
            B[1 + a, 1 + b] = mixed[:, b]
    return B


def slopes_reference(gram, prior_fn, X, r, noise, theta, Xs, cols):
    """-> (mean (P, m), cov (P, P, m), scales (P,)): the posterior of (value, slopes in ``cols``) at every test point and
    the plane scales sqrt(max_j prior_aa) the covariance bounds are taken against (pair (a, b): scales[a] scales[b])."""
    X, r, noise, theta, Xs = (torch.as_tensor(v, dtype=torch.float64) for v in (X, r, noise, theta, Xs))
    cols = [int(c) for c in cols]
    L = torch.linalg.cholesky(gram(X, X, theta) + torch.diag(noise))
    alpha = torch.cholesky_solve(r.unsqueeze(1), L).squeeze(1)
    Ks = cross_planes(gram, X, Xs, theta, cols)
    V = [torch.linalg.solve_triangular(L, K, upper=False) for K in Ks]
    sel = [0] + [1 + c for c in cols]
    prior = prior_fn(theta, Xs)[sel][:, sel]
    P, m = len(sel), Xs.shape[0]
    mean = torch.stack([K.T @ alpha for K in Ks])
    cov = torch.empty(P, P, m, dtype=torch.float64)
    for a in range(P):
        for b in range(P):
            cov[a, b] = prior[a, b] - (V[a] * V[b]).sum(0)
    scales = torch.sqrt(torch.stack([prior[a, a].max() for a in range(P)]))
    return mean, cov, scales


def errors(mean, cov, ref_mean, ref_cov, scales):
    """(worst plane-mean error / max(1, max |mean_plane|), worst packed-covariance error / (scales[a] scales[b]))."""
    mean, cov = mean.cpu().double(), unpack_cov(cov.cpu().double())
    P = ref_mean.shape[0]
    e_m = max(((mean[a] - ref_mean[a]).abs().max() / ref_mean[a].abs().max().clamp(min=1.0)).item() for a in range(P))
    e_c = max(((cov[a, b] - ref_cov[a, b]).abs().max() / (scales[a] * scales[b])).item() for a in range(P) for b in range(P))
    return e_m, e_c


def model_reference(model, Xnew, cols, gram=None, prior_fn=None):
    """(mean, cov, scales) in model space from a fitted engine model's own state, at model-space points ``Xnew``."""
    with torch.no_grad():
        if hasattr(model.model, "prepare_eval"):
            model.model.prepare_eval(model._train_x, Xnew.to(model._train_x.device, model._train_x.dtype))
        spec = model._prior()
        X = model._train_x.detach().cpu().double()
        y = model._train_y.detach().cpu().double()
        theta = torch.as_tensor(spec.theta).detach().cpu().double()
        prior = spec.mean.detach().cpu().double()
        noise = spec.noise.detach().cpu().double()
    name = model._plan.model
    return slopes_reference(gram or orc.GRAMS[name], prior_fn or PRIORS[name], X, y - prior, noise, theta,
                            Xnew.detach().cpu().double(), cols)


class SlopesOraclePlan(OraclePlan):
    """``OraclePlan`` with ``predict_slopes`` answered by ``slopes_reference`` (``GPPlan``'s surface, one site)."""

    def predict_slopes(self, theta, Xs, cols, chunk=None, return_cov=True):
        theta, r, noise = self._state
        mean, cov, _ = slopes_reference(orc.GRAMS[self.model], PRIORS[self.model], self.X, r, noise, theta, Xs.double(), cols)
        return mean.to(self.dtype), (pack_cov(cov).to(self.dtype) if return_cov else None)


def shifted(covariates, name, delta):
    """``covariates`` with covariate ``name`` moved by ``delta`` in its slope unit u (ln flow, years, stage), and the exact
    du that produced (timestamps move by whole nanoseconds, and a decimal year is not the same number of days every year)."""
    time = np.asarray(covariates.coords["time"].values)
    data = {k: ("time", np.asarray(covariates[k].values, dtype=np.float64).copy()) for k in covariates}
    if name == "time":
        moved = time + np.timedelta64(int(round(delta * 365.25 * 86400e9)), "ns")
        du = datetime_to_decimal_year(moved) - datetime_to_decimal_year(time)
        return Dataset(data, coords={"time": moved}), du
    values = data[name][1]
    data[name] = ("time", values * np.exp(delta) if name == "flow" else values + delta)
    return Dataset(data, coords={"time": time}), np.full(len(time), delta)
