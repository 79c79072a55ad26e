"""Dense CPU restatement of expectation propagation for censored fits, for the CPU and GPU suites (TEST INFRASTRUCTURE).

Rows of side 0 keep their exact Gaussian site (y~ = y, n~ = v).  A censored row (side -1 / +1: one-sided at the limit y; side 2:
the truth in [y, upper]) carries a Gaussian SITE with pseudo-target y~_i and pseudo-noise n~_i (natural parameters tau~ = 1 / n~,
nu~ = y~ / n~).  One PARALLEL sweep:
    factorise   a = (K + diag n~)^-1 (y~ - m),  k_i = [(K + diag n~)^-1]_ii,  mu = y~ - n~ o a  (the posterior mean at the samples)
    cavity      v_c = 1 / k - n~,   mu_c = y~ - a / k                        (the leave-one-out predictive of that regression)
    moments     log Z^, g = d log Z^ / d mu_c, W = -d2 log Z^ / d mu_c^2 by the pointwise functions of the Laplace fit at the
                standard deviation s = sqrt(v + v_c):  one-sided z = side (mu_c - y) / s;  bracket za = (y - mu_c) / s,
                Delta = (upper - y) / s;  g = (.) / s,  W = (.) / s^2
    proposal    tau' = W / (1 - W v_c),  y' = mu_c + g / W  (g / W := 0 when W is not positive),  nu' = y' tau'
    cap         tau' v < 1e-12:  tau' = 1e-12 / v, y' kept; the row is counted
    guard       v_c <= 0 or 1 - W v_c <= 0 (or either not a number): the row keeps its site for this sweep and is counted
    test        d_tau = max v |tau' - tau~| <= tol  and  d_mu <= tol, where d_mu = max_i |mu_i - mu_i^prev| over ALL rows from the
                second sweep on and, in the first sweep (no previous mean exists), max v |nu' - nu~| over the censored rows
    update      only when the test failed and the sweep is not the last: tau~ <- (1 - delta) tau~ + delta tau' and nu~ likewise
                (delta = 1: n~ = 1 / tau', y~ = y' exactly)
so the sites that were factorised last ARE the result, converged or not.  Sigma_ii = n~ - n~^2 k is never tested: for nearly
uninformative rows it is pure cancellation.  Value (R&W eq. 3.65; ``nll`` the short form with v_c + n~ = 1 / k and
mu_c - y~ = -a / k, ``nll_long`` the textbook form from Sigma = (K^-1 + diag tau~)^-1 and its own cavities):
    NLL_EP = NLL_engine(y~ - m, n~) - sum_censored [log Z^_i + 1/2 log 2 pi - 1/2 log k_i + a_i^2 / (2 k_i)]
and at the fixed point dNLL_EP / dtheta = the engine's explicit gradient, dNLL_EP / dr = a.
Cold start: the Laplace terms at f = m (``interval_helpers.terms``): n~ = 1 / W(m), y~ = m + g / W with the Laplace cap."""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import censored_helpers as ch
from tests import interval_helpers as ih

CAP = ch.CAP
LOG2PI = ch.LOG2PI


def tilted(mu_c, v_c, y, side, v, upper=None):
    """-> (log Z^, g, W) of the tilted distributions N(f | mu_c, v_c) p(y | f) of the censored rows (zeros on side 0)."""
    side = np.asarray(side)
    cens = side != 0
    br = side == 2
    with np.errstate(all="ignore"):
        s = np.sqrt(np.where(cens, v + v_c, 1.0))
        sd = np.where(br, 0, side).astype(np.float64)
        logphi, h, q, _c3 = ch.pointwise(np.where(cens & ~br, sd * (mu_c - y) / s, 0.0))
        logz, g, W = logphi, sd * h / s, q / (s * s)
        if br.any():
            up = np.asarray(upper, dtype=np.float64)
            za = np.where(br, (y - mu_c) / s, 0.0)
            dl = np.where(br, (up - y) / s, 1.0)
            logp, mu, wv, _d3 = ih.interval_pointwise(za, dl)
            logz, g, W = np.where(br, logp, logz), np.where(br, mu / s, g), np.where(br, wv / (s * s), W)
    zero = np.zeros_like(logz)
    return np.where(cens, logz, zero), np.where(cens, g, zero), np.where(cens, W, zero)


def cold_sites(y, side, v, m, upper=None):
    tm = ih.terms(m, y, side, v, m, upper)
    return m + tm["rt"], tm["nn"].copy(), int(tm["capped"])


def ep(K, y, side, v, m, upper=None, sites0=None, maxit=100, tol=1e-10, damping=1.0):
    """One EP fit on a dense K (numpy).  -> dict: yt, nt (the sites that were factorised last), mu, k, alpha, cav_mean, cav_var,
    logz, nll, nll_long, nll_engine, stat = (sweeps, d_mu, d_tau, capped, held, censored) and converged."""
    y, v, m = (np.asarray(t, dtype=np.float64) for t in (y, v, m))
    side = np.asarray(side)
    K = np.asarray(K, dtype=np.float64)
    n = len(y)
    cens = side != 0
    if not 0.0 < damping <= 1.0:
        raise ValueError("damping must be in (0, 1]")
    if sites0 is None:
        yt, nt, capped0 = cold_sites(y, side, v, m, upper)
    else:
        yt, nt = (np.asarray(t, dtype=np.float64).copy() for t in sites0)
        capped0 = 0
    yt[~cens], nt[~cens] = y[~cens], v[~cens]
    sweeps, d_mu, d_tau, capped, held = 0, 0.0, 0.0, capped0, 0
    converged = not cens.any()
    mu_prev = None
    while True:
        A = K + np.diag(nt)
        Ainv = np.linalg.inv(A)
        Ainv = 0.5 * (Ainv + Ainv.T)
        alpha = np.linalg.solve(A, yt - m)
        k = np.diag(Ainv).copy()
        mu = yt - nt * alpha
        v_c, mu_c = 1.0 / k - nt, yt - alpha / k
        logz, g, W = tilted(mu_c, v_c, y, side, v, upper)
        if converged:  # (no censored row: no sweep)
            break
        sweeps += 1
        with np.errstate(all="ignore"):
            om = 1.0 - W * v_c
            ok = cens & (v_c > 0.0) & (om > 0.0) & np.isfinite(g)
            tau_p = np.where(ok, W / np.where(ok, om, 1.0), 0.0)
            cap = ok & ~(tau_p * v >= CAP)
            tau_p = np.where(cap, CAP / v, tau_p)
            y_p = mu_c + np.where(W > 0.0, g / np.where(W > 0.0, W, 1.0), 0.0)
            nu_p = y_p * tau_p
            tau, nu = 1.0 / nt, yt / nt
            d_tau = float(np.max(np.where(ok, v * np.abs(tau_p - tau), 0.0)))
            if mu_prev is None:
                d_mu = float(np.max(np.where(ok, v * np.abs(nu_p - nu), 0.0)))
            else:
                d_mu = float(np.max(np.abs(mu - mu_prev)))
        capped, held = int(cap.sum()), int((cens & ~ok).sum())
        converged = d_mu <= tol and d_tau <= tol
        if converged or sweeps >= maxit:
            break
        if damping == 1.0:
            nt = np.where(ok, 1.0 / np.where(ok, tau_p, 1.0), nt)
            yt = np.where(ok, y_p, yt)
        else:
            tn = (1.0 - damping) * tau + damping * tau_p
            nn = (1.0 - damping) * nu + damping * nu_p
            nt = np.where(ok, 1.0 / tn, nt)
            yt = np.where(ok, nn / tn, yt)
        mu_prev = mu
    rt = yt - m
    _sign, logdet = np.linalg.slogdet(A)
    nll_engine = float(0.5 * rt @ alpha + 0.5 * logdet + 0.5 * n * LOG2PI)
    with np.errstate(all="ignore"):
        short = np.where(cens, logz + 0.5 * LOG2PI - 0.5 * np.log(k) + alpha * alpha / (2.0 * k), 0.0)
    # the textbook form: Sigma = (K^-1 + diag tau~)^-1 = K - K A^-1 K, posterior mean mu_full = m + K alpha, cavities from them
    Sigma = K - K @ Ainv @ K
    mu_full = m + K @ alpha
    with np.errstate(all="ignore"):
        sii = np.diag(Sigma)
        tc = 1.0 / sii - 1.0 / nt
        vc2 = 1.0 / tc
        mc2 = vc2 * (mu_full / sii - yt / nt)
        logz2, _g2, _w2 = tilted(mc2, vc2, y, side, v, upper)
        long_ = np.where(cens, logz2 + 0.5 * np.log(vc2 + nt) + (mc2 - yt) ** 2 / (2.0 * (vc2 + nt)), 0.0)
    _s2, logdetB = np.linalg.slogdet(A)
    nll_long = float(0.5 * logdetB + 0.5 * rt @ np.linalg.solve(A, rt) + 0.5 * (n - int(cens.sum())) * LOG2PI - long_.sum())
    return dict(yt=yt, nt=nt, mu=mu, k=k, alpha=alpha, cav_mean=mu_c, cav_var=v_c, logz=logz, nll=nll_engine - float(short.sum()),
                nll_long=nll_long, nll_engine=nll_engine, rt=rt, nn=nt, converged=bool(converged), K=K,
                stat=(float(sweeps), d_mu, d_tau, float(capped), float(held), float(cens.sum())))


def _np(t):
    return np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t)


def ep_fit(model, X, y, side, v, m, theta, upper=None, sites0=None, maxit=100, tol=1e-10, damping=1.0, with_grad=True):
    """Everything ``dgp_ep_fit_step`` returns, densely: ``ep`` on the oracle's Gram matrix plus dtheta and dr = alpha from the
    oracle's explicit gradient at the final sites."""
    from oracle import gp_oracle as orc

    X = torch.as_tensor(X, dtype=torch.float64)
    theta = torch.as_tensor(theta, dtype=torch.float64).detach()
    y, v, m = (_np(t).astype(np.float64) for t in (y, v, m))
    side = _np(side)
    upper = None if upper is None else _np(upper).astype(np.float64)
    res = ep(ch.gram(model, X, theta), y, side, v, m, upper, sites0, maxit, tol, damping)
    res["theta"] = theta
    if with_grad:
        with torch.enable_grad():
            val, g_theta, alpha, g_noise = orc.nll_data_and_grads(model, X, torch.tensor(res["rt"]), torch.tensor(res["nt"]), theta)
        res.update(dtheta=g_theta.numpy(), dr=alpha.numpy(), dnoise=g_noise.numpy(), nll_engine_oracle=float(val))
    return res


def nll_of(model, X, y, side, v, m, theta, upper=None, tol=1e-13, maxit=400):
    """The re-converged EP value alone (for central differences)."""
    res = ep_fit(model, X, y, side, v, m, theta, upper, tol=tol, maxit=maxit, with_grad=False)
    assert res["converged"], res["stat"]
    return res["nll"]


def posterior(model, X, res, Xs, full_cov=False):
    """The EP posterior of the latent f at Xs (without the prior mean): the GP posterior of the pseudo-data."""
    return ch.posterior(model, X, res, Xs, full_cov=full_cov)


class EPOraclePlan(ih.IntervalOraclePlan):
    """``IntervalOraclePlan`` with the EP entry points of ``backend.GPPlan``, answered by ``ep_fit`` above."""

    def _ep(self, with_grad, theta, y, mean, noise, side, sites, maxit, tol, damping, upper):
        from discontinuum_amd import _lib

        self.ep_calls = getattr(self, "ep_calls", 0) + 1
        theta = torch.as_tensor(theta, dtype=torch.float64).detach()
        out = torch.zeros(_lib.OUT_LEN, dtype=self.dtype)
        s0 = None if sites is None else tuple(_np(t) for t in sites)
        try:
            res = ep_fit(self.model, self.X, y.detach(), side, noise.detach(), mean.detach(), theta,
                         None if upper is None else upper.detach(), s0, maxit, tol, damping, with_grad=with_grad)
        except (torch.linalg.LinAlgError, np.linalg.LinAlgError):
            out[_lib.OUT_NLL], out[_lib.OUT_INFO] = float("nan"), 1
            zero = torch.zeros(self.n, dtype=self.dtype)
            keep = (y.detach().clone(), noise.detach().clone()) if sites is None else tuple(t.detach().clone() for t in sites)
            self.ep_stat = (0.0, float("inf"), float("inf"), 0.0, 0.0, 0.0)
            return (out, zero, keep, self.ep_stat) if with_grad else (out, keep, self.ep_stat)
        self._state = (theta, torch.tensor(res["rt"]), torch.tensor(res["nt"]))
        self.ep_stat = tuple(float(x) for x in res["stat"])
        self.ep_aux = {k: torch.tensor(res[k], dtype=self.dtype) for k in ("cav_mean", "cav_var", "logz")}
        new = (torch.tensor(res["yt"], dtype=self.dtype), torch.tensor(res["nt"], dtype=self.dtype))
        if not res["converged"]:
            raise _lib.DGPError(_lib.E_NOCONV, "dgp_ep_fit_step", "expectation propagation did not converge")
        out[_lib.OUT_NLL] = res["nll"]
        if not with_grad:
            return out, new, self.ep_stat
        dr = torch.tensor(res["dr"], dtype=self.dtype)
        out[_lib.OUT_DTHETA:_lib.OUT_DTHETA + self.ntheta] = torch.tensor(res["dtheta"])
        out[_lib.OUT_SUM_DR] = dr.sum()
        out[_lib.OUT_SUM_DNOISE] = float(res["dnoise"].sum())
        if getattr(self, "_dr_w", None) is not None:
            out[_lib.OUT_DR_W0] = (dr * self._dr_w[0]).sum()
            out[_lib.OUT_DR_W0 + 1] = (dr * self._dr_w[1]).sum()
        return out, dr, new, self.ep_stat

    def ep_fit_step(self, theta, y, mean, noise, side, sites=None, maxit=100, tol=1e-10, damping=1.0, upper=None):
        self.calls += 1
        return self._ep(True, theta, y, mean, noise, side, sites, maxit, tol, damping, upper)

    def ep_factorize(self, theta, y, mean, noise, side, sites=None, maxit=100, tol=1e-10, damping=1.0, upper=None):
        return self._ep(False, theta, y, mean, noise, side, sites, maxit, tol, damping, upper)
