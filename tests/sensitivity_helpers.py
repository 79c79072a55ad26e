"""Dense references for the Jacobians of the posterior mean and variance with respect to the hyperparameter directions, and a
plan double that knows ``predict_sensitivity`` (TEST INFRASTRUCTURE).

``dense_sensitivity`` is forward-mode ``jvp`` through ``oracle.posterior`` (Cholesky + triangular solves), one pass per
direction: it shares nothing with the device's route (T = L^-1, beta = T^T T K*, derivative pair sums, tile GEMMs).
``formula_sensitivity`` evaluates the formulas the device implements, densely in double; the CPU suite holds the two against
each other, which keeps the GPU bound honest."""
from __future__ import annotations

import functools

import torch
import torch.autograd.forward_ad as fwAD

from oracle import gp_oracle as orc
from tests.fisher_helpers import FisherOraclePlan


def _rows(t):
    return [] if t is None else [row for row in t.double()]


def _jvp(fn, x, tangent):
    """Forward-mode derivative of ``fn`` (a tensor or a tuple of tensors) at ``x`` along ``tangent``: one dual-number pass."""
    with fwAD.dual_level():
        out = fn(fwAD.make_dual(x, tangent))
        many = isinstance(out, tuple)
        tans = [fwAD.unpack_dual(o).tangent for o in (out if many else (out,))]
        tans = [torch.zeros_like(o) if t is None else t.detach().clone() for t, o in zip(tans, out if many else (out,))]
    return tuple(tans) if many else tans[0]


def dense_sensitivity(model, X, r, noise, theta, Xs, diag=None, rhs=None):
    """-> (dmean (P + E + C, m), dvar (P + E, m)): kernel directions d/dtheta_p, then the rows of ``diag`` (E, n) as directions
    of the noise diagonal, then -- mean only -- the rows of ``rhs`` (C, n) as directions g_c of the prior mean at the training
    rows (the residual r = y - m(X) moves by -g_c)."""
    X, r, noise, theta, Xs = (t.double() for t in (X, r, noise, theta, Xs))
    zero, one = torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64)
    Jm, Jv = [], []
    for p in range(theta.numel()):
        e = torch.zeros_like(theta)
        e[p] = 1.0
        tm, tv = _jvp(lambda th: orc.posterior(model, X, r, noise, th, Xs), theta, e)
        Jm.append(tm)
        Jv.append(tv)
    for dvec in _rows(diag):
        tm, tv = _jvp(lambda s: orc.posterior(model, X, r, noise + s * dvec, theta, Xs), zero, one)
        Jm.append(tm)
        Jv.append(tv)
    for g in _rows(rhs):
        tm, _tv = _jvp(lambda s: orc.posterior(model, X, r - s * g, noise, theta, Xs), zero, one)
        Jm.append(tm)
    return torch.stack(Jm), torch.stack(Jv)


def formula_sensitivity(model, X, r, noise, theta, Xs, diag=None, rhs=None):
    """The same Jacobians from the formulas of ``dgp_predict_sensitivity``, dense in double: beta = K^^-1 K*, D_p = dK/dtheta_p,
    D*_p = dK*/dtheta_p by forward-mode jvp of the oracle's Gram."""
    X, r, noise, theta, Xs = (t.double() for t in (X, r, noise, theta, Xs))
    gram = orc.GRAMS[model]
    Khat = gram(X, X, theta) + torch.diag(noise)
    T = torch.linalg.inv(torch.linalg.cholesky(Khat))
    alpha = T.T @ (T @ r)
    beta = T.T @ (T @ gram(X, Xs, theta))
    Fm, Fv = [], []
    for p in range(theta.numel()):
        e = torch.zeros_like(theta)
        e[p] = 1.0
        D = _jvp(lambda th: gram(X, X, th), theta, e)
        Ds = _jvp(lambda th: gram(X, Xs, th), theta, e)
        dd = _jvp(lambda th: torch.diagonal(gram(Xs, Xs, th)), theta, e)
        Fm.append(Ds.T @ alpha - beta.T @ (D @ alpha))
        Fv.append(dd - 2 * (beta * Ds).sum(0) + (beta * (D @ beta)).sum(0))
    for dvec in _rows(diag):
        Fm.append(-beta.T @ (dvec * alpha))
        Fv.append((beta * beta * dvec[:, None]).sum(0))
    for g in _rows(rhs):
        Fm.append(-beta.T @ g)
    return torch.stack(Fm).detach(), torch.stack(Fv).detach()


def scaled_rows(J, J_ref):
    """Per direction max_j |J - J_ref| / max_j |J_ref| -> (rows,) tensor.  A direction whose reference is identically zero has
    no scale of its own (``fisher_helpers.scaled_error``'s rule): it is measured against the largest scale of the reference."""
    J, J_ref = J.double().cpu(), J_ref.double().cpu()
    sc = J_ref.abs().amax(dim=1)
    diff = (J - J_ref).abs().amax(dim=1)
    if float(sc.max()) == 0.0:
        return torch.where(diff == 0, torch.zeros_like(diff), torch.full_like(diff, float("inf")))
    sc = torch.where(sc > 0, sc, sc.max().expand_as(sc))
    return diff / sc


class SensitivityOraclePlan(FisherOraclePlan):
    """``FisherOraclePlan`` + ``predict_sensitivity``, by jvp through the oracle's posterior: the CPU stand-in the engine-level
    host algebra is exercised against."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        if self._sites:
            self._sites = [SensitivityOraclePlan(self.model, self.n, self.d, self.dtype) for _ in range(self.batch)]

    def predict_sensitivity(self, theta, Xs, diag=None, rhs=None, chunk=None, return_var=True):
        if self._sites:
            cut = lambda t, b: None if t is None else t[b][:, : self._sizes[b]]  # noqa: E731
            out = [p.predict_sensitivity(None, Xs[b], cut(diag, b), cut(rhs, b), return_var=return_var) for b, p in enumerate(self._sites)]
            return torch.stack([o[0] for o in out]), (torch.stack([o[1] for o in out]) if return_var else None)
        theta, r, noise = self._state
        Jm, Jv = dense_sensitivity(self.model, self.X, r, noise, theta, Xs, diag, rhs)
        return Jm, (Jv if return_var else None)


# ---- the cases of tests/test_gpu_sensitivity.py; tests/test_sensitivity_cpu.py holds the two references against each other on
# every one of them
TREND = "loadest+trend d=3"
NS = (1, 2, 127, 128, 129, 257, 300)  # pads in n, one and several row tiles
MS = (1, 130, 300)                    # m below one tile, pads in m, m > n
MODELS = (("loadest", 2), ("loadest", 3), ("loadest", 4), ("rating", 2), (TREND, 3))
CASES = [(model, d, n, m) for model, d in MODELS for n in NS for m in MS]
E_MAX, C_MAX = 2, 3


def columns(E, C, n, seed=0):
    """(diag (E, n) or None, rhs (C, n) or None): the first E / C rows of one fixed set, so that every (E, C) of a case is a
    subset of the rows of the reference at (E_MAX, C_MAX)."""
    g = torch.Generator().manual_seed(1000 + seed)
    diag = torch.stack([torch.ones(n, dtype=torch.float64), 0.2 + torch.rand(n, dtype=torch.float64, generator=g)])
    rhs = torch.stack([torch.ones(n, dtype=torch.float64), torch.randn(n, dtype=torch.float64, generator=g),
                       torch.randn(n, dtype=torch.float64, generator=g)])
    return (diag[:E] if E else None), (rhs[:C] if C else None)


def _near(X, m, seed):
    """m test points next to the rows of X.  One or two training points leave most of an independent record of test points
    many lengthscales away, where a kernel part and every derivative of it have decayed to 1e-37: such a direction is zero
    for every purpose, yet not identically, and has no scale to measure an error against."""
    g = torch.Generator().manual_seed(2000 + seed)
    Xs = X[torch.arange(m) % X.shape[0]].clone()
    Xs[:, 0] += 0.1 * torch.randn(m, dtype=torch.float64, generator=g)
    Xs[:, 1:] *= 1.0 + 0.03 * torch.randn(m, X.shape[1] - 1, dtype=torch.float64, generator=g)
    return Xs


def build_case(model, d, n, m, seed=3):
    """-> (plan model name, X (n, d), r, noise, theta, Xs (m, d)).  Test points: an independent record of m points, except
    for n <= 2 (``_near``)."""
    from tests.test_gpu_composite import _case as composite_case
    from tests.test_gpu_stages import make_case

    if model == TREND:
        name, _, X, r, noise, theta = composite_case(TREND, n, seed)
        Xs = composite_case(TREND, m, seed + 1)[2] if n > 2 else _near(X, m, seed)
        return name, X, r, noise, theta, Xs
    X, r, noise, theta = make_case(model, d, n, seed=seed, perturb=0.3)
    Xs = make_case(model, d, m, seed=seed + 1)[0] if n > 2 else _near(X, m, seed)
    return model, X, torch.nan_to_num(r, nan=0.3), noise, theta, Xs  # (y is standardised: undefined for one observation)


@functools.lru_cache(maxsize=None)
def reference(model, d, n, m):
    """The dense reference of a case at (E_MAX, C_MAX), computed once per process and never modified by its users."""
    name, X, r, noise, theta, Xs = build_case(model, d, n, m)
    diag, rhs = columns(E_MAX, C_MAX, n)
    return dense_sensitivity(name, X, r, noise, theta, Xs, diag, rhs)


def reference_rows(ref, P, E, C):
    """The rows of ``reference`` that a call with E diagonal directions and C right-hand sides returns."""
    Jm, Jv = ref
    keep = list(range(P + E)) + list(range(P + E_MAX, P + E_MAX + C))
    return Jm[keep], Jv[: P + E]
