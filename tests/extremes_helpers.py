"""Host restatements for the period-extreme tests: the orthant estimator of ``csrc/dgp_orthant.hip`` in numpy / scipy, point
for point on the same generators and shifts, and the closed forms the estimator is held against."""
from __future__ import annotations

import numpy as np
from scipy.special import ndtr, ndtri

YMAX = 38.0  # the |y| clamp of the device code


def weights(gen, shifts, npoints):
    """w[s, n, i] = |2 frac(n g_i + D_{s,i}) - 1|, n = 1 .. npoints: product and sum rounded once each (numpy never fuses)."""
    n = np.arange(1, npoints + 1, dtype=np.float64)
    x = n[None, :, None] * gen[None, None, :] + shifts[:, None, :]
    x = x - np.floor(x)
    return np.abs(2.0 * x - 1.0)


def orthant_ref(L, lo, hi, gen, shifts, npoints, return_shifts=False, return_y=False):
    """Genz's separation of variables for P(lo <= f <= hi), f ~ N(0, L L^T), over ``shifts.shape[0]`` randomly shifted
    Richtmyer rules of ``npoints`` points with the tent transform; vectorised over shifts and points, sequential in the
    dimension.  Tail care as on the device: the pair (A, B) and the argument of Phi^-1 are formed in the upper tail when the
    interval's centre lies there, so 1 - tiny is never formed; d < 0 counts as 0; y is clamped to +-38.
    ``L``: (m, m) lower factor (only its lower triangle is read); ``lo`` / ``hi``: (m,) centred limits, +-inf allowed.
    -> (prob, se), with ``return_shifts`` also the per-shift estimates."""
    L = np.asarray(L, dtype=np.float64)
    m = L.shape[0]
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.float64), (m,)), np.broadcast_to(np.asarray(hi, dtype=np.float64), (m,))
    gen, shifts = np.asarray(gen, dtype=np.float64)[:m], np.asarray(shifts, dtype=np.float64)[:, :m]
    S = shifts.shape[0]
    w_all = weights(gen, shifts, npoints)
    w_all = np.ascontiguousarray(np.moveaxis(w_all, 2, 0))  # (m, S, npoints): a dimension's slice is contiguous
    y = np.zeros((m, S, npoints))
    p = np.ones((S, npoints))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        for i in range(m):
            c = np.tensordot(L[i, :i], y[:i], axes=1) if i else np.zeros((S, npoints))
            a, b = (lo[i] - c) / L[i, i], (hi[i] - c) / L[i, i]
            flip = a + b > 0.0
            A, B = ndtr(np.where(flip, -b, a)), ndtr(np.where(flip, -a, b))
            d = np.maximum(B - A, 0.0)
            w = np.where(flip, 1.0 - w_all[i], w_all[i])
            t = np.minimum(A + w * d, 1.0)
            z = np.clip(ndtri(t), -YMAX, YMAX)
            y[i] = np.where(flip, -z, z)
            p = p * d
    est = p.mean(axis=1)
    prob, se = est.mean(), est.std(ddof=1) / np.sqrt(S)
    if return_y:
        return prob, se, y, p
    return (prob, se, est) if return_shifts else (prob, se)


def equicorrelated_truth(m, rho, b, nodes=400):
    """P(max_i f_i <= b) for f ~ N(0, (1 - rho) I + rho 11^T): int phi(z) Phi((b - sqrt(rho) z) / sqrt(1 - rho))^m dz by
    Gauss-Legendre on [-9, 9] (the integrand is smooth and its tails are below 1e-18 there)."""
    x, wq = np.polynomial.legendre.leggauss(nodes)
    z = 9.0 * x
    f = np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi) * ndtr((b - np.sqrt(rho) * z) / np.sqrt(1.0 - rho)) ** m
    return float(9.0 * np.sum(wq * f))


def equicorrelated_factor(m, rho):
    return np.linalg.cholesky((1.0 - rho) * np.eye(m) + rho * np.ones((m, m)))


def factor_layout(Lm, poison=True):
    """An (m, m) lower factor in the layout ``psd_safe_factor`` leaves: (M, M), M = m rounded up to 128, zeros above the
    diagonal inside the diagonal 128-blocks, identity pad; ``poison``: NaN in every block above the block diagonal, which the
    device code must never read."""
    m = Lm.shape[0]
    M = -(-m // 128) * 128
    out = np.eye(M)
    out[:m, :m] = np.tril(Lm)
    if poison:
        for bi in range(M // 128):
            out[bi * 128:(bi + 1) * 128, (bi + 1) * 128:] = np.nan
    return out


def make_oracle_plan():
    """``WindowOraclePlan`` with the two entries the period extremes add, answered on the host: ``psd_safe_factor`` (torch's
    Cholesky with the same jitter ladder, padded layout) and ``orthant_probability`` (``orthant_ref`` on the product's own
    generators and shifts).  Built on demand: the window helpers import the oracle."""
    import torch

    from discontinuum_amd.backend import orthant_shifts, richtmyer_generators
    from tests.window_helpers import WindowOraclePlan

    class ExtremeOraclePlan(WindowOraclePlan):
        def psd_safe_factor(self, cov, m, ladder=None):
            eye = torch.eye(cov.shape[0], dtype=torch.float64)
            for jitter in ladder or (0.0, 1e-8, 1e-7, 1e-6):
                L, info = torch.linalg.cholesky_ex(cov.double() + jitter * eye)
                if int(info) == 0:
                    return L, jitter
            raise RuntimeError("not positive definite")

        def orthant_probability(self, L, m, lo, hi, npoints=4096, nshifts=16, seed=0, max_bytes=None):
            lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1, m), np.asarray(hi, dtype=np.float64).reshape(-1, m)
            gen, sh = richtmyer_generators(m), orthant_shifts(m, nshifts, seed).numpy()
            out = np.array([orthant_ref(L.numpy()[:m, :m], lo[l], hi[l], gen, sh, npoints) for l in range(lo.shape[0])])
            return torch.tensor(out[:, 0]), torch.tensor(out[:, 1])

    return ExtremeOraclePlan


def smooth_cov(m, ell=30.0, noise=0.05, amp=1.0):
    """A smooth GP plus short-range noise over m days: amp^2 exp(-d^2 / 2 ell^2) + noise^2 I."""
    t = np.arange(m, dtype=np.float64)
    return amp * amp * np.exp(-0.5 * ((t[:, None] - t[None, :]) / ell) ** 2) + noise * noise * np.eye(m)
