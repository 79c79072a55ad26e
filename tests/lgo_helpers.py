"""The leave-group-out training objective restated densely (TEST INFRASTRUCTURE): torch fp64 on the oracle's Gram matrix, the value
from ``torch.linalg.inv`` and every gradient from autograd -- not from the closed forms the engine uses -- plus the closed forms
themselves (for the CPU test that compares the two), a brute-force deletion of whole folds, and a plan double that answers
``set_folds`` / ``lgo_fit_step`` / ``lgo_value`` from the restatement."""
from __future__ import annotations

import math

import torch

from discontinuum_amd import _lib

from tests.loo_helpers import LooOraclePlan, khat

LOG_2PI = math.log(2.0 * math.pi)


def fold_index(groups):
    """Fold ids (n,) (-1 = never held out) -> the list of index tensors of the non-empty folds, in fold order."""
    g = torch.as_tensor(groups).to(torch.int64).reshape(-1)
    return [idx for idx in (torch.nonzero(g == k).reshape(-1) for k in range(int(g.max()) + 1)) if idx.numel()]


def lgo_from_khat(Khat, r, groups):
    """L_LGO = sum_g [1/2 alpha_g^T G_g^-1 alpha_g - 1/2 log|G_g| + b_g / 2 log 2 pi], G_g = (Khat^-1)[B_g, B_g]."""
    S = torch.linalg.inv(Khat)
    S = 0.5 * (S + S.T)
    alpha = S @ r
    total = torch.zeros((), dtype=torch.float64)
    for idx in fold_index(groups):
        G = S[idx][:, idx]
        a = alpha[idx]
        total = total + 0.5 * a @ torch.linalg.solve(G, a) - 0.5 * torch.linalg.slogdet(G)[1] + 0.5 * idx.numel() * LOG_2PI
    return total


def lgo_value_and_grads(model, X, r, noise, theta, groups):
    """-> (value, d/dtheta, d/dr, d/dnoise) of L_LGO, the gradients by autograd through the inverse."""
    th, rr, nz = (t.detach().double().clone().requires_grad_(True) for t in (theta, r, noise))
    with torch.enable_grad():
        val = lgo_from_khat(khat(model, X.double(), th, nz), rr, groups)
        g = torch.autograd.grad(val, (th, rr, nz))
    return val.detach(), g[0], g[1], g[2]


def closed_form(Khat, r, groups):
    """The engine's formulas: (value, M2, b, alpha) with dL/dK^ = 1/2 (M2 - b alpha^T - alpha b^T), dL/dr = b,
    dL/dnoise_i = 1/2 (M2)_ii - b_i alpha_i."""
    n = r.shape[0]
    S = torch.linalg.inv(Khat)
    S = 0.5 * (S + S.T)
    alpha = S @ r
    c = torch.zeros(n, dtype=torch.float64)
    W = torch.zeros(n, n, dtype=torch.float64)
    val = torch.zeros((), dtype=torch.float64)
    for idx in fold_index(groups):
        G = S[idx][:, idx]
        Cg = torch.linalg.inv(G)
        Cg = 0.5 * (Cg + Cg.T)
        e = Cg @ alpha[idx]
        c[idx] = e
        W[idx[:, None], idx[None, :]] = Cg + torch.outer(e, e)
        val = val + 0.5 * alpha[idx] @ e - 0.5 * torch.linalg.slogdet(G)[1] + 0.5 * idx.numel() * LOG_2PI
    return val, S @ W @ S, S @ c, alpha


def brute_force_lgo(Khat, r, groups):
    """-sum_g log N(r_g | mu_-g, C_-g) with the rows / columns of fold g really deleted (own noise included in C)."""
    n = r.shape[0]
    total = torch.zeros((), dtype=torch.float64)
    for idx in fold_index(groups):
        held = set(idx.tolist())
        keep = torch.tensor([j for j in range(n) if j not in held], dtype=torch.int64)
        if keep.numel() == 0:
            mu, cov = torch.zeros(idx.numel(), dtype=torch.float64), Khat
        else:
            Kr = Khat[keep][:, keep]
            Kx = Khat[keep][:, idx]
            mu = Kx.T @ torch.linalg.solve(Kr, r[keep])
            cov = Khat[idx][:, idx] - Kx.T @ torch.linalg.solve(Kr, Kx)
        d = r[idx] - mu
        total = total + 0.5 * d @ torch.linalg.solve(cov, d) + 0.5 * torch.linalg.slogdet(cov)[1] + 0.5 * idx.numel() * LOG_2PI
    return total


class LgoOraclePlan(LooOraclePlan):
    """``LooOraclePlan`` with the leave-group-out step answered from the dense restatement; counts its calls."""

    def __init__(self, model, n, d, dtype=torch.float64, device="cpu", lookahead=True, batch=1):
        super().__init__(model, n, d, dtype, device, lookahead, batch)
        self.lgo_calls = 0
        self._folds = None
        if self.batch > 1:
            self._sites = [LgoOraclePlan(model, n, d, dtype) for _ in range(self.batch)]

    def set_folds(self, groups):
        if groups is None:
            self._folds = None
            return
        g = torch.as_tensor(groups).to(torch.int64)
        shape = (self.n,) if self.batch == 1 else (self.batch, self.n)
        if tuple(g.shape) != shape:
            raise ValueError(f"groups must have shape {shape}, got {tuple(g.shape)}")
        if int(g.min()) < -1:
            raise ValueError("fold ids must be >= 0, or -1 for observations that are never held out")
        self._folds = g.clone()

    def _need_folds(self, what):
        if self._folds is None:
            raise ValueError(f"{what}: no folds in the plan (call set_folds first)")
        return self._folds

    def lgo_fit_step(self, theta, r, noise):
        folds = self._need_folds("lgo_fit_step")
        self.lgo_calls += 1
        if self._sites:
            rows = []
            for b, p in enumerate(self._sites):
                p.set_folds(folds[b, : self._sizes[b]])
                rows.append(p.lgo_fit_step(theta[b], r[b, : self._sizes[b]], noise[b, : self._sizes[b]]))
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
        val, g_theta, g_r, g_noise = lgo_value_and_grads(self.model, self.X, r64, nz64, theta, folds)
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

    def lgo_value(self):
        theta, r, noise = self._state
        return torch.stack([lgo_from_khat(khat(self.model, self.X, theta, noise), r, self._need_folds("lgo_value")),
                            torch.zeros((), dtype=torch.float64)])
