"""The leave-one-out training objective restated densely (TEST INFRASTRUCTURE): torch fp64 on the oracle's Gram matrix, the value from
``torch.linalg.inv`` and every gradient from autograd -- not from the closed forms the engine uses -- plus the closed forms
themselves (for the CPU test that compares the two), a brute-force deletion of single rows, and a plan double that answers
``loo_fit_step`` / ``loo_value`` from the restatement."""
from __future__ import annotations

import math

import torch

from discontinuum_amd import _lib
from oracle import gp_oracle as orc

from tests.helpers import OraclePlan

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def khat(model, X, theta, noise):
    return orc.GRAMS[model](X, X, theta) + torch.diag(noise)


def loo_from_khat(Khat, r):
    """L_LOO = sum_i [1/2 log 2 pi - 1/2 log k_i + alpha_i^2 / (2 k_i)], k = diag Khat^-1, alpha = Khat^-1 r."""
    S = torch.linalg.inv(Khat)
    S = 0.5 * (S + S.T)
    k = torch.diagonal(S)
    alpha = S @ r
    return (HALF_LOG_2PI - 0.5 * torch.log(k) + 0.5 * alpha * alpha / k).sum()


def loo_value_and_grads(model, X, r, noise, theta):
    """-> (value, d/dtheta, d/dr, d/dnoise) of L_LOO, the gradients by autograd through the inverse."""
    th, rr, nz = (t.detach().double().clone().requires_grad_(True) for t in (theta, r, noise))
    with torch.enable_grad():
        val = loo_from_khat(khat(model, X.double(), th, nz), rr)
        g = torch.autograd.grad(val, (th, rr, nz))
    return val.detach(), g[0], g[1], g[2]


def closed_form(Khat, r):
    """The engine's formulas: (value, M, b, alpha, k) with dL/dK^ = M - 1/2 (b alpha^T + alpha b^T), dL/dr = b."""
    S = torch.linalg.inv(Khat)
    S = 0.5 * (S + S.T)
    k = torch.diagonal(S)
    alpha = S @ r
    w = (1.0 + alpha * alpha / k) / (2.0 * k)
    c = alpha / k
    M = S @ torch.diag(w) @ S
    b = S @ c
    val = (HALF_LOG_2PI - 0.5 * torch.log(k) + 0.5 * alpha * alpha / k).sum()
    return val, M, b, alpha, k


def brute_force_loo(Khat, r):
    """-sum_i log N(r_i | mu_-i, var_-i) with row / column i really deleted (own noise included in var)."""
    n = r.shape[0]
    total = torch.zeros((), dtype=torch.float64)
    for i in range(n):
        keep = [j for j in range(n) if j != i]
        Kr = Khat[keep][:, keep]
        ki = Khat[keep, i]
        sol = torch.linalg.solve(Kr, torch.stack([ki, r[keep]], dim=1))
        mu = ki @ sol[:, 1]
        var = Khat[i, i] - ki @ sol[:, 0]
        total = total + HALF_LOG_2PI + 0.5 * torch.log(var) + 0.5 * (r[i] - mu) ** 2 / var
    return total


class LooOraclePlan(OraclePlan):
    """``OraclePlan`` with the leave-one-out step answered from the dense restatement; counts its calls."""

    def __init__(self, model, n, d, dtype=torch.float64, device="cpu", lookahead=True, batch=1):
        super().__init__(model, n, d, dtype, device, lookahead, batch)
        self.loo_calls = 0
        if self.batch > 1:
            self._sites = [LooOraclePlan(model, n, d, dtype) for _ in range(self.batch)]

    def loo_fit_step(self, theta, r, noise):
        self.loo_calls += 1
        if self._sites:
            rows = [p.loo_fit_step(theta[b], r[b, : self._sizes[b]], noise[b, : self._sizes[b]]) for b, p in enumerate(self._sites)]
            pad = lambda v: torch.cat([v, torch.zeros(self.n - v.shape[0], dtype=v.dtype)])  # noqa: E731
            return (torch.stack([o for o, _, _ in rows]), torch.stack([pad(a) for _, a, _ in rows]),
                    torch.stack([pad(g) for _, _, g in rows]))
        theta = torch.as_tensor(theta, dtype=torch.float64).detach()
        out = torch.zeros(_lib.OUT_LEN, dtype=self.dtype)
        r64, nz64 = r.detach().double(), noise.detach().double()
        Kh = khat(self.model, self.X, theta, nz64)
        if int(torch.linalg.cholesky_ex(Kh)[1]) != 0:  # not positive definite: as fit_step reports it
            out[_lib.OUT_NLL] = float("nan")
            out[_lib.OUT_INFO] = 1
            return out, torch.zeros(self.n, dtype=self.dtype), torch.zeros(self.n, dtype=self.dtype)
        val, g_theta, g_r, g_noise = loo_value_and_grads(self.model, self.X, r64, nz64, theta)
        out[_lib.OUT_NLL] = val
        out[_lib.OUT_QUAD] = r64 @ torch.linalg.solve(Kh, r64)
        out[_lib.OUT_LOGDET] = torch.linalg.slogdet(Kh)[1]
        out[_lib.OUT_DTHETA:_lib.OUT_DTHETA + self.ntheta] = g_theta
        out[_lib.OUT_SUM_DR] = g_r.sum()
        out[_lib.OUT_SUM_DNOISE] = g_noise.sum()
        if getattr(self, "_dr_w", None) is not None:
            out[_lib.OUT_DR_W0] = (g_r * self._dr_w[0]).sum()
            out[_lib.OUT_DR_W0 + 1] = (g_r * self._dr_w[1]).sum()
        self._state = (theta, r64, nz64)
        return out, g_r.to(self.dtype), g_noise.to(self.dtype)

    def loo_value(self):
        theta, r, noise = self._state
        return torch.stack([loo_from_khat(khat(self.model, self.X, theta, noise), r), torch.zeros((), dtype=torch.float64)])
