"""Dense-deletion references shared by the cross-validation tests (tests/test_crossval_cpu.py, tests/test_gpu_crossval.py)."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import gp_oracle as orc
from tests.helpers import OraclePlan


def dense_deletion_cv(Khat, r, groups):
    """Cross-validation by DELETION on a dense fp64 K^ (n, n) and residual r (n,): for every fold id in ``groups`` (-1 =
    never held out) the fold's rows and columns are removed, the rest is Cholesky-solved and the fold conditioned on it.
    -> (resid, var, lpd): y_B - E[y_B | y_-B] and diag Cov[y_B | y_-B] at the observations' positions (0 where never held
    out), the joint log density per fold id (0 for an id nobody uses).  Independent of the partitioned-inverse identity the
    device code uses."""
    Khat = torch.as_tensor(Khat, dtype=torch.float64)
    r = torch.as_tensor(r, dtype=torch.float64)
    g = torch.as_tensor(np.asarray(groups), dtype=torch.int64)
    n = r.shape[0]
    ngroups = int(g.max()) + 1
    resid, var = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    lpd = torch.zeros(ngroups, dtype=torch.float64)
    for f in range(ngroups):
        B = (g == f).nonzero().reshape(-1)
        if B.numel() == 0:
            continue
        R = (g != f).nonzero().reshape(-1)
        mean = torch.zeros(B.numel(), dtype=torch.float64)
        cov = Khat[B][:, B].clone()
        if R.numel():
            L = torch.linalg.cholesky(Khat[R][:, R])
            V = torch.linalg.solve_triangular(L, Khat[R][:, B], upper=False)
            z = torch.linalg.solve_triangular(L, r[R, None], upper=False)
            mean = (V.T @ z).reshape(-1)
            cov = cov - V.T @ V
        e = r[B] - mean
        Lc = torch.linalg.cholesky(0.5 * (cov + cov.T))
        w = torch.linalg.solve_triangular(Lc, e[:, None], upper=False).reshape(-1)
        resid[B], var[B] = e, cov.diagonal()
        lpd[f] = -0.5 * (w @ w) - Lc.diagonal().log().sum() - 0.5 * B.numel() * math.log(2 * math.pi)
    return resid, var, lpd


class CVOraclePlan(OraclePlan):
    """``OraclePlan`` with ``cross_validate`` by dense deletion (``GPPlan.cross_validate``'s surface, single site)."""

    def cross_validate(self, groups):
        theta, r, noise = self._state
        Khat = orc.GRAMS[self.model](self.X, self.X, theta) + torch.diag(noise)
        g = torch.as_tensor(np.asarray(groups), dtype=torch.int64)
        resid, var, lpd = dense_deletion_cv(Khat, r, g)
        return resid, var, lpd, torch.zeros(lpd.shape[0], dtype=torch.int32)


def posterior_deletion_reference(model, groups):
    """The held-out (mu, var) in model space from the engine's own state through ``orc.posterior``: for every fold the
    oracle posterior of the rows outside it, evaluated at the rows inside it with the full covariance, plus the held-out
    rows' prior mean and noise.  -> numpy (mu, var, cov_by_fold)."""
    with torch.no_grad():
        if hasattr(model.model, "prepare_eval"):
            model.model.prepare_eval(model._train_x, model._train_x)
        spec = model._prior()
        X = model._train_x.detach().cpu().double()
        y = model._train_y.detach().cpu().double()
        theta = torch.as_tensor(spec.theta).detach().cpu().double()
        mean = spec.mean.detach().cpu().double()
        noise = spec.noise.detach().cpu().double()
    name = model._plan.model
    g = np.asarray(groups)
    mu, var, covs = np.full(len(g), np.nan), np.full(len(g), np.nan), {}
    for f in np.unique(g[g >= 0]):
        B, R = np.nonzero(g == f)[0], np.nonzero(g != f)[0]
        m, cov = orc.posterior(name, X[R], (y - mean)[R], noise[R], theta, X[B], full_cov=True)
        cov = cov + torch.diag(noise[B])
        mu[B], var[B] = (m + mean[B]).numpy(), cov.diagonal().numpy()
        covs[int(f)] = cov.numpy()
    return mu, var, covs
