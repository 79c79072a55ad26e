"""Dense references for the posterior of the covariance's additive parts (tests/test_terms_cpu.py, tests/test_gpu_terms.py).

The oracle's Gram functions are linear in the outputscales, so part c's Gram is the oracle's own Gram evaluated at the
hyperparameters with every OTHER outputscale set to 0 -- nothing of the oracle is changed.  From these the helper builds
mean_c = K_c^T alpha and the C x C point covariances with ``torch.linalg.solve_triangular``, as ``orc.posterior`` does."""
from __future__ import annotations

import numpy as np
import torch

from oracle import gp_oracle as orc
from tests.helpers import OraclePlan

NAMES = {"loadest": ("seasonal", "covariates", "residual"), "rating": ("shift_1", "shift_2", "bend", "base", "periodic")}


def outputscale_indices(model, d, spec=None):
    """Positions of the parts' outputscales in theta, in the parts' order."""
    if model == "loadest":
        return (0, 4, 4 + d)
    if model == "rating":
        return (1, 4, 7, 10, 12)
    spec = [int(v) for v in spec]
    idx, i, t = [], 2, 0
    for _term in range(spec[1]):
        scaled, nfac = spec[i], spec[i + 1]
        i += 2
        assert scaled, "the zeroed-outputscale construction needs every term scaled"
        idx.append(t)
        t += 1
        for _f in range(nfac):
            kind, _nu2, ard, nd = spec[i:i + 4]
            i += 4 + nd
            t += (nd if ard else 1) + (1 if kind == 2 else 0)
    return tuple(idx)


def term_grams(gram, os_idx):
    """One Gram function per part: ``gram`` with the other parts' outputscales zeroed."""
    def part(c):
        def fn(X1, X2, theta):
            th = theta.clone()
            for k, i in enumerate(os_idx):
                if k != c:
                    th[i] = 0.0
            return gram(X1, X2, th)
        return fn
    return [part(c) for c in range(len(os_idx))]


def terms_reference(gram, parts, X, r, noise, theta, Xs):
    """-> (mean (C, m), cov (C, C, m), scale): the parts' posterior means, their point covariances and the largest TOTAL
    prior variance max_j k(x*_j, x*_j), the scale every variance / covariance bound is taken against.  ``parts``: the
    positions of the parts' outputscales in theta (``outputscale_indices``; the zeroed-outputscale construction), or one
    Gram function (X1, X2, theta) per part -- a composite with an unscaled term has no outputscale to zero
    (tests/composite_helpers.py builds its parts from one-term descriptions)."""
    X, r, noise, theta, Xs = (torch.as_tensor(v, dtype=torch.float64) for v in (X, r, noise, theta, Xs))
    parts = list(parts)
    parts = parts if parts and callable(parts[0]) else term_grams(gram, parts)
    L = torch.linalg.cholesky(gram(X, X, theta) + torch.diag(noise))
    alpha = torch.cholesky_solve(r.unsqueeze(1), L).squeeze(1)
    Ks = [g(X, Xs, theta) for g in parts]
    V = [torch.linalg.solve_triangular(L, K, upper=False) for K in Ks]
    kss = [torch.diagonal(g(Xs, Xs, theta)) for g in parts]
    C, m = len(parts), Xs.shape[0]
    mean = torch.stack([K.T @ alpha for K in Ks])
    cov = torch.empty(C, C, m, dtype=torch.float64)
    for c in range(C):
        for e in range(C):
            cov[c, e] = (kss[c] if c == e else 0.0) - (V[c] * V[e]).sum(0)
    scale = float(torch.diagonal(gram(Xs, Xs, theta)).max())
    return mean, cov, scale


def pack_cov(cov):
    """(C, C, m) -> (C (C + 1) / 2, m), entry (c, c'), c' <= c, at c (c + 1) / 2 + c' (the device's layout)."""
    C = cov.shape[0]
    return torch.stack([cov[c, e] for c in range(C) for e in range(c + 1)])


def unpack_cov(packed):
    packed = torch.as_tensor(packed)
    P = packed.shape[-2]
    C = int(round((np.sqrt(8 * P + 1) - 1) / 2))
    full = torch.empty(packed.shape[:-2] + (C, C, packed.shape[-1]), dtype=packed.dtype)
    for c in range(C):
        for e in range(c + 1):
            full[..., c, e, :] = full[..., e, c, :] = packed[..., c * (c + 1) // 2 + e, :]
    return full


def model_reference(model, Xnew):
    """The parts' (mean (C, m), cov (C, C, m), scale) in model space from a fitted engine model's own state (the pattern of
    ``crossval_helpers.posterior_deletion_reference``), at model-space points ``Xnew``."""
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
    return terms_reference(orc.GRAMS[name], outputscale_indices(name, X.shape[1]), X, y - prior, noise, theta,
                           Xnew.detach().cpu().double())


class TermsOraclePlan(OraclePlan):
    """``OraclePlan`` with ``nterms`` / ``predict_terms`` answered by ``terms_reference`` (``GPPlan``'s surface, one site)."""

    @property
    def nterms(self):
        return len(NAMES[self.model])

    def predict_terms(self, theta, Xs, chunk=None, return_cov=True):
        theta, r, noise = self._state
        mean, cov, _ = terms_reference(orc.GRAMS[self.model], outputscale_indices(self.model, self.d), self.X, r, noise, theta,
                                       Xs.double())
        return mean.to(self.dtype), (pack_cov(cov).to(self.dtype) if return_cov else None)
