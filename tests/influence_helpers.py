"""Dense references for the influence of folds of observations on the period sums, and a plan double that knows
``deletion_influence`` (TEST INFRASTRUCTURE).

``dense_deletion_influence`` DELETES: for every fold it removes the fold's rows, runs ``oracle.posterior`` on the rest with the
full covariance and takes the difference of the period sums (and of their variances for a linear target).  It shares nothing
with the partitioned-inverse identities the device implements.  ``formula_deletion_influence`` evaluates those identities
densely in double; the CPU suite holds the two against each other, which keeps the GPU bound honest."""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import gp_oracle as orc
from tests.flux_helpers import dense_period_moments
from tests.sensitivity_helpers import CASES, SensitivityOraclePlan, build_case  # noqa: F401  (the shared case grid)

MODE_LINEAR, MODE_LOG = 0, 1
SCALE, SHIFT = 0.7, 0.4  # s and t of the target transform the references use


def _onehot(periods, P):
    g = torch.as_tensor(np.asarray(periods), dtype=torch.int64)
    A = torch.zeros(g.shape[0], P, dtype=torch.float64)
    ok = g >= 0
    A[ok.nonzero().reshape(-1), g[ok]] = 1.0
    return A


def period_sums(mode, mu, cov, w, A, s, t):
    """(L (P,), Var (P,) for the linear mode else None, the per-point a) of f ~ N(mu, cov); ``cov`` full (m, m) or its diagonal."""
    diag = cov if cov.dim() == 1 else cov.diagonal()
    if mode == MODE_LOG:
        a = w * torch.exp(s * mu + t + 0.5 * s * s * diag)
        return A.T @ a, None, a
    a = s * w
    Wa = A * a[:, None]
    return A.T @ (w * (s * mu + t)), ((Wa.T @ cov @ Wa).diagonal() if cov.dim() == 2 else None), a


def _posterior_of_rows(Khat, Ks, Kss, r, keep):
    """``oracle.posterior(..., full_cov=True)`` of the training rows ``keep``, line by line, from Grams evaluated once: the rows
    and columns of K^ and the rows of K* that belong to deleted observations are dropped, nothing else is reused."""
    L = torch.linalg.cholesky(Khat[keep][:, keep])
    alpha = torch.cholesky_solve(r[keep].unsqueeze(1), L).squeeze(1)
    mu = Ks[keep].T @ alpha
    V = torch.linalg.solve_triangular(L, Ks[keep], upper=False)
    return mu, Kss - V.T @ V


def dense_deletion_both(model, X, r, noise, theta, Xs, folds, w, periods, P, s=SCALE, t=SHIFT):
    """``dense_deletion_influence`` for both modes from ONE pass of deletions -> {MODE_LINEAR: dict, MODE_LOG: dict}."""
    X, r, noise, theta, Xs, w = (torch.as_tensor(v).double() for v in (X, r, noise, theta, Xs, w))
    g = np.asarray(folds)
    F = int(g.max()) + 1
    A = _onehot(periods, P)
    gram = orc.GRAMS[model]
    Khat, Ks, Kss = gram(X, X, theta) + torch.diag(noise), gram(X, Xs, theta), gram(Xs, Xs, theta)
    mu, cov = orc.posterior(model, X, r, noise, theta, Xs, full_cov=True)
    sd = cov.diagonal().clamp(min=0.0).sqrt()
    out = {}
    for mode in (MODE_LINEAR, MODE_LOG):
        L, Var, a = period_sums(mode, mu, cov, w, A, s, t)
        scale = L.abs() if mode == MODE_LOG else A.T @ (a.abs() * (mu.abs() + sd))
        out[mode] = {"dload": torch.zeros(F, P, dtype=torch.float64), "dvar": torch.zeros(F, P, dtype=torch.float64) if mode == MODE_LINEAR else None,
                     "shift": torch.zeros(F, dtype=torch.float64), "load": L, "var": Var, "a": a, "inv_sd": 1.0 / sd, "scale": scale}
    for f in range(F):
        keep = torch.as_tensor(np.nonzero(g != f)[0])
        if keep.numel() == X.shape[0]:
            continue  # an empty fold changes nothing
        if keep.numel() == 0:  # everything deleted: the prior
            mu2, cov2 = torch.zeros_like(mu), Kss
        else:
            mu2, cov2 = _posterior_of_rows(Khat, Ks, Kss, r, keep)
        for mode in (MODE_LINEAR, MODE_LOG):
            L2, Var2, _ = period_sums(mode, mu2, cov2, w, A, s, t)
            out[mode]["dload"][f] = L2 - out[mode]["load"]
            if mode == MODE_LINEAR:
                out[mode]["dvar"][f] = Var2 - out[mode]["var"]
            out[mode]["shift"][f] = ((mu2 - mu).abs() / sd).max()
    return out


def dense_deletion_influence(model, X, r, noise, theta, Xs, folds, w, periods, P, mode, s=SCALE, t=SHIFT):
    """Brute-force deletion.  ``folds`` (n,) fold ids (-1: in no fold), ``w`` (m,) weights, ``periods`` (m,) ids (-1: excluded).
    -> dict: ``dload`` (F, P) = sums without the fold minus with it, ``dvar`` (F, P) (linear mode) or None, ``shift`` (F,) =
    max_j |mu'_j - mu_j| / sigma_j, ``load`` (P,), ``var`` (P,) or None, ``a`` (m,), ``inv_sd`` (m,), ``scale`` (P,): the
    denominators of the error measures -- L_g (log) or sum_{j in g} |a_j| (|mu_j| + sigma_j) (linear)."""
    return dense_deletion_both(model, X, r, noise, theta, Xs, folds, w, periods, P, s, t)[mode]


def formula_deletion_influence(model, X, r, noise, theta, Xs, folds, a, scale, periods, P, mode, inv_sd=None):
    """The identities of ``dgp_deletion_influence``, dense in double: -> (dload (F, P), dvar (F, P) or None, shift (F,) or None,
    info (F,) int32).  A fold whose block G_F is not positive definite gets NaN rows and info 1."""
    X, r, noise, theta, Xs, a = (torch.as_tensor(v).double() for v in (X, r, noise, theta, Xs, a))
    g = np.asarray(folds)
    F = int(g.max()) + 1
    A = _onehot(periods, P)
    Khat = orc.GRAMS[model](X, X, theta) + torch.diag(noise)
    S = torch.linalg.inv(Khat)
    S = 0.5 * (S + S.T)
    alpha = S @ r
    beta = S @ orc.GRAMS[model](X, Xs, theta)
    s = float(scale)
    dload = torch.zeros(F, P, dtype=torch.float64)
    dvar = torch.zeros(F, P, dtype=torch.float64) if mode == MODE_LINEAR else None
    shift = torch.zeros(F, dtype=torch.float64) if inv_sd is not None else None
    info = torch.zeros(F, dtype=torch.int32)
    for f in range(F):
        rows = torch.as_tensor(np.nonzero(g == f)[0])
        if rows.numel() == 0:
            continue
        M, bad = torch.linalg.cholesky_ex(S[rows][:, rows])
        if int(bad) != 0:
            dload[f] = float("nan")
            info[f] = int(bad)
            if dvar is not None:
                dvar[f] = float("nan")
            if shift is not None:
                shift[f] = float("nan")
            continue
        z = torch.linalg.solve_triangular(M, beta[rows], upper=False)            # (f, m)
        u = torch.linalg.solve_triangular(M, alpha[rows, None], upper=False)[:, 0]
        dmu, ds2 = -(z.T @ u), (z * z).sum(0)
        if mode == MODE_LOG:
            dload[f] = A.T @ (a * torch.expm1(s * dmu + 0.5 * s * s * ds2))
        else:
            dload[f] = A.T @ (a * dmu)
            dvar[f] = ((z * a[None, :]) @ A).pow(2).sum(0)
        if shift is not None:
            shift[f] = (dmu.abs() * torch.as_tensor(inv_sd).double()).max()
    return dload, dvar, shift, info


def errors(ref, dload, dvar=None, shift=None):
    """The issue's error measures against a ``dense_deletion_influence`` result: max |dL - dL_ref| / scale_g, max |dVar - dVar_ref|
    / Var_g and max |shift - shift_ref| / max(1, shift_ref) -> (e_load, e_var, e_shift), None where not given."""
    e_load = ((torch.as_tensor(dload).double().cpu() - ref["dload"]).abs() / ref["scale"][None, :]).max().item()
    e_var = e_shift = None
    if dvar is not None:
        e_var = ((torch.as_tensor(dvar).double().cpu() - ref["dvar"]).abs() / ref["var"][None, :]).max().item()
    if shift is not None:
        e_shift = ((torch.as_tensor(shift).double().cpu() - ref["shift"]).abs() / ref["shift"].clamp(min=1.0)).max().item()
    return e_load, e_var, e_shift


def record(m, nperiods=3, excluded=True):
    """(w (m,), periods (m,) int32): positive seeded weights; ``nperiods`` contiguous periods of nearly equal length, with -- when
    there is room -- one excluded point inside the first period and one at the end."""
    gen = torch.Generator().manual_seed(77 + m)
    w = 0.5 + torch.rand(m, dtype=torch.float64, generator=gen)
    P = min(nperiods, m)
    periods = (np.arange(m) * P // m).astype(np.int32)
    if excluded and m >= 8:
        periods[1] = -1
        periods[-1] = -1
    return w, periods, P


def fold_schemes(n):
    """name -> fold ids (n,) for the issue's schemes that fit n observations."""
    out = {"loo": np.arange(n, dtype=np.int64), "all": np.zeros(n, dtype=np.int64)}
    sizes = [1, 2, 63, 64]
    if n >= sum(sizes) + 2:  # the LDS route and its boundary; some observations in no fold, fold id 2 empty
        ids = np.full(n, -1, dtype=np.int64)
        perm = np.random.default_rng(5).permutation(n)
        pos = 0
        for fid, k in zip((0, 1, 3, 4), sizes):
            ids[perm[pos:pos + k]] = fid
            pos += k
        out["lds"] = ids
    if n >= 65 + 129 + 1:  # the block route at orders 128 and 256 (max fold <= 128 without the rest, 256 with it when large)
        ids = np.full(n, 2, dtype=np.int64)
        perm = np.random.default_rng(6).permutation(n)
        ids[perm[:65]] = 0
        ids[perm[65:65 + 129]] = 1
        out["block"] = ids
    elif n >= 66:
        ids = np.full(n, 1, dtype=np.int64)
        ids[np.random.default_rng(6).permutation(n)[:65]] = 0
        out["block"] = ids
    return out


@functools.lru_cache(maxsize=None)
def reference(model, d, n, m, scheme):
    """The deletion references {mode: dict} of a case of the shared grid, computed once per process and never modified by its users."""
    name, X, r, noise, theta, Xs = build_case(model, d, n, m)
    w, periods, P = record(m)
    return dense_deletion_both(name, X, r, noise, theta, Xs, fold_schemes(n)[scheme], w, periods, P)


# ---- the engine-level reference
def engine_reference(engine, kind, record, weights, folds, freq):
    """Deletion with every piece from the model oracle (constrained hyperparameters, prior mean, noise) at the engine's raw
    values: -> (reference dict of ``dense_deletion_influence``, fold ids, period ids of the sorted record, P, mode)."""
    from discontinuum_amd.loads import _kept, period_groups, target_transform
    from discontinuum_amd.validation import cv_folds
    from tests.fisher_helpers import oracle_view

    x_all = torch.tensor(engine.dm.Xnew(record), dtype=torch.float64)
    engine._eval_ready(x_all.to(engine.device, engine.dtype))
    o, raw, _perm, X, fixed = oracle_view(engine, kind)
    order, periods, labels, _np, _dr = _kept(*period_groups(record.coords["time"].values, np.asarray(weights), freq))
    x = x_all[torch.as_tensor(order)]
    n = X.shape[0]
    noise = (fixed + (o.second_noise(raw) if kind == "rating" else 0.0)).expand(n).detach()
    theta = o.constrained(raw).detach()
    y = engine._train_y.double().cpu()
    mode, s, t = target_transform(engine.dm)
    ids, _labels = cv_folds(np.asarray(engine.dm.data.target.coords["time"].values), folds)
    w = torch.as_tensor(np.asarray(weights, dtype=np.float64)[order])
    ref = dense_deletion_influence(kind, X, (y - o.mean(raw, X)).detach(), noise, theta, x, ids, w, periods, len(labels), mode, s=s,
                                      t=t + s * o.mean(raw, x).detach())
    return ref, ids, periods, len(labels), mode


class InfluenceOraclePlan(SensitivityOraclePlan):
    """The oracle plan + ``deletion_influence`` (the device's formulas, dense) and ``posterior_period_moments``: the CPU
    stand-in the host logic of ``discontinuum_amd.influence`` is exercised against."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        if self._sites:
            self._sites = [InfluenceOraclePlan(self.model, self.n, self.d, self.dtype) for _ in range(self.batch)]

    def posterior_period_moments(self, theta, Xs, mu, scale2, w, groups, ngroups, mode, extra_var=None):
        theta, r, noise = self._state
        _mu, cov = orc.posterior(self.model, self.X, r, noise, theta, Xs.double(), full_cov=True)
        return dense_period_moments(cov, mu, scale2, w, groups, ngroups, mode, extra_var)

    def deletion_influence(self, theta, Xs, groups, a, scale, periods, nperiods, mode, inv_sd=None, max_bytes=None, max_group=None):
        g = torch.as_tensor(groups)
        if g.dtype.is_floating_point or g.dtype == torch.bool:
            raise ValueError("fold ids must be integers")
        if tuple(g.shape) != (self.n,) or int(g.min()) < -1 or int(g.max()) < 0:
            raise ValueError("fold ids: one per observation, >= 0 or -1, at least one held out")
        need = 3 * 8 * (-(-self.n // 128) * 128) * (-(-Xs.shape[0] // 128) * 128)
        if max_bytes is not None and need > int(max_bytes):
            raise ValueError(f"the influence needs a work area of {need} bytes, which exceeds max_bytes = {int(max_bytes)}")
        theta, r, noise = self._state
        return formula_deletion_influence(self.model, self.X, r, noise, theta, Xs, g.numpy(), a, scale, periods, int(nperiods), mode, inv_sd)
