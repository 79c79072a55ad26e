"""Parity across the hyperparameter domain (tests/test_domain_cpu.py, tests/test_gpu_domain.py): the 40-digit fixtures of
tests/golden/make_domain_pairs.py, the bounds the device is held to, and plain numpy emulations of every model's pair formula
(TEST INFRASTRUCTURE; everything here runs on the CPU).

Bounds ("Parity across the hyperparameter domain"):
  values, per entry, of the sum of the outputscales          fp64 1e-13   float32 5e-6
      fp64: the bound of tests/test_gpu_stages.py, scaled.  An entry's error is (|arg| + a few) 2^-53 relative with
      |arg| e^-|arg| poly <= 1.5; float32: ~80 x 2^-24.
  derivative sweeps, per parameter, of the stored sum |term|   fp64 1e-12   float32 1e-4
      fp64: argument rounding up to (708 + 20) 2^-53 = 1.6e-13 per term at the exponent clamp, plus summation; float32:
      (87 + 20) 2^-24 = 6e-6, plus the phase features' 4 delta / l <= 2.4e-5 at l = 0.02, plus accumulation over 2628 pairs.
The emulations below -- the formulas alone, in numpy at the plan's precision -- must stay within a QUARTER of each bound at
every corner (tests/test_domain_cpu.py); the measured figures are in DESIGN.md.

The emulations are written from the formulas (closed-form derivatives with respect to the constrained hyperparameters), not
by calling the library.  They follow the device in the two places where the formula is a choice: the inverse hyperparameters
are formed in double and rounded to the working precision, and the fused models take sin / cos of pi t / p per POINT in
double and the angle-difference identities per pair.

The composite tree registers ONE more structure in the library's registry (39 of its 64 slots over the whole suite, see
tests/composite_helpers.py)."""
from __future__ import annotations

import functools
import importlib.util
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

VALUE_BOUND = {np.float64: 1e-13, np.float32: 5e-6}   # per entry, x sum of the outputscales
SWEEP_BOUND = {np.float64: 1e-12, np.float32: 1e-4}   # per parameter, x sum |term|
NOISE_FRACTION = 0.1                                  # products: noise = 0.1 sum_os on every row, cond(K^) <= 1 + 10 n


@functools.lru_cache(maxsize=None)
def generator():
    """tests/golden/make_domain_pairs.py as a module (the corner tables, the composite's description, the mpmath entries)."""
    spec = importlib.util.spec_from_file_location("make_domain_pairs", os.path.join(GOLDEN, "make_domain_pairs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case_ids():
    return [f"{model}_{corner}" for model, corner in generator().CASES]


def split_id(case):
    model, corner = case.split("_")
    return model, corner


def plan_model(model):
    """(GPPlan model family, d) of a fixture's model."""
    g = generator()
    return ("loadest" if model.startswith("loadest") else model), g.MODEL_D[model]


@functools.lru_cache(maxsize=None)
def load(case):
    """The fixture as a dict of read-only arrays, with K (n, n) and S (n, n) unpacked to full symmetric matrices."""
    with np.load(os.path.join(GOLDEN, f"domain_{case}.npz")) as z:
        fx = {k: z[k].astype(np.float64) if z[k].dtype == np.float32 else z[k] for k in z.files}
    n = fx["X"].shape[0]
    for packed, full in (("K_tril", "K"), ("S_tril", "S")):
        m = np.zeros((n, n))
        m[np.tril_indices(n)] = fx[packed]
        fx[full] = m + np.tril(m, -1).T
    fx["sum_os"] = float(fx["sum_os"])
    for v in fx.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return fx


@functools.lru_cache(maxsize=None)
def load_batch():
    """The extra sites of the batched sweep (``build_batch``): theta (5, 11), X (5, 24, 3), u, alpha (5, 24), g_bil and
    g_bil_scale (5, 11), read-only."""
    with np.load(os.path.join(GOLDEN, "domain_loadest3_batch.npz")) as z:
        fx = {k: z[k].astype(np.float64) for k in z.files}
    for v in fx.values():
        v.setflags(write=False)
    return fx


def within(got, ref, scale, bound):
    """(|got - ref| <= bound scale everywhere, the worst |got - ref| / scale where scale > 0).  A scale of exactly 0 -- a
    derivative every term of which underflows, a part that is switched off -- leaves no room: the entry must be exact."""
    err, scale = np.abs(np.asarray(got, dtype=np.float64) - ref), np.broadcast_to(scale, np.shape(ref))
    worst = float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0
    return bool((err <= bound * scale).all()), worst


def unpack_prior(prior):
    """(P (P + 1) / 2, m) -> (P, P, m)."""
    P = int(round((np.sqrt(8 * prior.shape[0] + 1) - 1) / 2))
    full = np.empty((P, P, prior.shape[1]))
    for a in range(P):
        for b in range(a + 1):
            full[a, b] = full[b, a] = prior[a * (a + 1) // 2 + b]
    return full


# ---- numpy emulations of the pair formulas ---------------------------------------------------------------------------------------
SQRT3, SQRT5 = 1.73205080756887729353, 2.23606797749978969641


def _exp(x, T):
    """e^x for x <= 0 at precision T; float32 as 2^(x log2 e), the two-instruction form the argument rounding of which the
    float32 bounds price."""
    if T is np.float32:
        return np.exp2(x * T(1.44269504088896340736))
    return np.exp(x)


def _m52(absd, inv_l, T):
    """Matern-5/2 of |delta| / l: (q, poly, dpoly) with value poly e^-q and d value / d l = dpoly e^-q / l."""
    q = T(SQRT5) * absd * inv_l
    return q, T(1) + q + q * q * T(1.0 / 3.0), (T(1) + q) * q * q * T(1.0 / 3.0)


def _m32(absd, inv_l, T):
    q = T(SQRT3) * absd * inv_l
    return q, T(1) + q, q * q


def _phase(t, inv_p_double, T):
    """sin and cos of pi t / p per point, in double, rounded to T."""
    a = np.pi * np.remainder(t.astype(np.float64) * inv_p_double, 2.0)
    return np.sin(a).astype(T), np.cos(a).astype(T)


def _periodic_time(t1, t2, th_l, th_p, th_lm, T):
    """Periodic x Matern-5/2 in time from per-point phase features: value / os, and its derivatives by l, p, l_matern."""
    inv_p = 1.0 / th_p
    s1, c1 = _phase(t1, inv_p, T)
    s2, c2 = _phase(t2, inv_p, T)
    s = s1[:, None] * c2[None, :] - c1[:, None] * s2[None, :]
    c = c1[:, None] * c2[None, :] + s1[:, None] * s2[None, :]
    dt = t1[:, None] - t2[None, :]
    inv_lp, inv_lm, inv_pT = T(1.0 / th_l), T(1.0 / th_lm), T(inv_p)
    q, poly, dpoly = _m52(np.abs(dt), inv_lm, T)
    e = _exp(T(-2) * s * s * inv_lp - q, T)
    base = e * poly
    return base, base * (T(2) * s * s * inv_lp * inv_lp), base * (T(4 * np.pi) * dt * s * c * inv_lp * inv_pT * inv_pT), e * dpoly * inv_lm


def emulate(model, X1, X2, theta, T, grad=False):
    """K(X1, X2) of a fixture's model in numpy at precision T, and with ``grad`` the planes d K / d theta_p (ntheta, n1, n2)."""
    theta = [float(v) for v in theta]
    X1, X2 = np.asarray(X1, dtype=T), np.asarray(X2, dtype=T)
    n1, n2 = X1.shape[0], X2.shape[0]
    dK = np.zeros((len(theta), n1, n2), dtype=T)
    diff = lambda c: X1[:, c][:, None] - X2[:, c][None, :]  # noqa: E731
    if model.startswith("loadest"):
        d = X1.shape[1]
        os1, os2, os3 = T(theta[0]), T(theta[4]), T(theta[4 + d])
        b1, d_lp, d_p, d_lm = _periodic_time(X1[:, 0], X2[:, 0], theta[1], theta[2], theta[3], T)
        dK[0], dK[1], dK[2], dK[3] = b1, os1 * d_lp, os1 * d_p, os1 * d_lm
        sq2, sq3 = np.zeros((n1, n2), dtype=T), np.zeros((n1, n2), dtype=T)
        z2, z3 = [], []
        for j in range(d):
            z3.append(diff(j) * T(1.0 / theta[5 + d + j]))
            sq3 += z3[-1] * z3[-1]
            if j:
                z2.append(diff(j) * T(1.0 / theta[4 + j]))
                sq2 += z2[-1] * z2[-1]
        b2 = _exp(T(-0.5) * sq2, T)
        q3 = T(SQRT3) * np.sqrt(sq3)
        e3 = _exp(-q3, T)
        b3 = (T(1) + q3) * e3
        dK[4], dK[4 + d] = b2, b3
        for j in range(d - 1):
            dK[5 + j] = os2 * b2 * z2[j] * z2[j] * T(1.0 / theta[5 + j])
        for j in range(d):
            dK[5 + d + j] = T(3) * os3 * e3 * z3[j] * z3[j] * T(1.0 / theta[5 + d + j])
        K = os1 * b1 + os2 * b2 + os3 * b3
    elif model == "rating":
        def gate(x):  # (g, 1 - g), each from its own exponential
            a = T(20) * (x[:, 1] - T(theta[0]))
            with np.errstate(over="ignore"):
                return T(1) / (T(1) + np.exp(a)), T(1) / (T(1) + np.exp(-a))
        g1, h1 = gate(X1)
        g2, h2 = gate(X2)
        gg, hh = g1[:, None] * g2[None, :], h1[:, None] * h2[None, :]
        w1, w2 = np.log(X1[:, 1] + T(1e-6)), np.log(X2[:, 1] + T(1e-6))
        adw, adt = np.abs(w1[:, None] - w2[None, :]), np.abs(diff(0))
        lower = np.zeros((n1, n2), dtype=T)
        for o in (1, 4):
            os, inv_ls, inv_lt = T(theta[o]), T(1.0 / theta[o + 1]), T(1.0 / theta[o + 2])
            qs, ps, ds = _m52(adw, inv_ls, T)
            qt, pt, dt_ = _m32(adt, inv_lt, T)
            e = _exp(-qs - qt, T)
            base = e * ps * pt
            lower += os * base
            dK[o], dK[o + 1], dK[o + 2] = gg * base, gg * os * e * ds * pt * inv_ls, gg * os * e * ps * dt_ * inv_lt
        os_u, inv_ls, inv_lt = T(theta[7]), T(1.0 / theta[8]), T(1.0 / theta[9])
        qs, ps, ds = _m52(adw, inv_ls, T)
        qt, pt, dt_ = _m52(adt, inv_lt, T)
        e = _exp(-qs - qt, T)
        upper = os_u * e * ps * pt
        dK[7], dK[8], dK[9] = hh * e * ps * pt, hh * os_u * e * ds * pt * inv_ls, hh * os_u * e * ps * dt_ * inv_lt
        os_b, inv_lb = T(theta[10]), T(1.0 / theta[11])
        qb, pb, db = _m52(adw, inv_lb, T)
        eb = _exp(-qb, T)
        dK[10], dK[11] = eb * pb, os_b * eb * db * inv_lb
        os_p = T(theta[12])
        bp, d_lp, d_p, d_lm = _periodic_time(X1[:, 0], X2[:, 0], theta[13], theta[14], theta[15], T)
        dK[12], dK[13], dK[14], dK[15] = bp, os_p * d_lp, os_p * d_p, os_p * d_lm
        gp1, gp2 = T(20) * g1 * h1, T(20) * g2 * h2  # d gate / d b; the inverted gate has the opposite sign
        dK[0] = (lower * (gp1[:, None] * g2[None, :] + g1[:, None] * gp2[None, :])
                 - upper * (gp1[:, None] * h2[None, :] + h1[:, None] * gp2[None, :]))
        K = gg * lower + hh * upper + os_b * eb * pb + os_p * bp
    else:
        K, t = np.zeros((n1, n2), dtype=T), 0
        for scaled, factors in generator().COMPOSITE_TERMS:
            os, os_at = T(1), None
            if scaled:
                os, os_at, t = T(theta[t]), t, t + 1
            vals, ders = [], []  # per factor: its value and [(theta index, d value / d theta)]
            for kind, nu2, ard, cols in factors:
                if kind == 2:
                    dt = diff(cols[0])
                    inv_l, inv_p = T(1.0 / theta[t]), T(1.0 / theta[t + 1])
                    # the phase in double: the exact difference of the coordinates times 1 / p rounded to double
                    exact = X1[:, cols[0]].astype(np.float64)[:, None] - X2[:, cols[0]].astype(np.float64)[None, :]
                    a = np.pi * np.remainder(exact * (1.0 / theta[t + 1]), 2.0)
                    s, c = np.sin(a).astype(T), np.cos(a).astype(T)
                    v = _exp(T(-2) * s * s * inv_l, T)
                    ders.append([(t, v * T(2) * s * s * inv_l * inv_l), (t + 1, v * T(4 * np.pi) * dt * s * c * inv_l * inv_p * inv_p)])
                    t += 2
                else:
                    inv = [T(1.0 / theta[t + (j if ard else 0)]) for j in range(len(cols))]
                    z = [diff(c) * inv[j] for j, c in enumerate(cols)]
                    sq = sum(zz * zz for zz in z)
                    if kind == 0:
                        v = aux = _exp(T(-0.5) * sq, T)
                    else:
                        r = np.sqrt(sq)
                        if nu2 == 1:
                            v = _exp(-r, T)
                            with np.errstate(divide="ignore", invalid="ignore"):
                                aux = np.where(sq > 0, v / r, T(0)).astype(T)
                        elif nu2 == 3:
                            e = _exp(-T(SQRT3) * r, T)
                            v, aux = (T(1) + T(SQRT3) * r) * e, T(3) * e
                        else:
                            q = T(SQRT5) * r
                            e = _exp(-q, T)
                            v, aux = (T(1) + q + q * q * T(1.0 / 3.0)) * e, T(5.0 / 3.0) * (T(1) + q) * e
                    dl = {}
                    for j in range(len(cols)):
                        at = t + (j if ard else 0)
                        dl[at] = dl.get(at, 0) + aux * z[j] * z[j] * inv[j]
                    ders.append(list(dl.items()))
                    t += len(cols) if ard else 1
                vals.append(v)
            prod = functools.reduce(lambda a, b: a * b, vals)
            K = K + os * prod
            if os_at is not None:
                dK[os_at] = prod
            for f, fd in enumerate(ders):
                others = functools.reduce(lambda a, b: a * b, [v for g, v in enumerate(vals) if g != f], os)
                for at, dv in fd:
                    dK[at] = dK[at] + others * dv
    return (K, dK) if grad else K


def sweeps(dK, u, alpha, S, T):
    """(g_bil, g_nll) of emulated derivative planes at precision T: sum_ij u_i dK_ij alpha_j and 1/2 sum_ij (S - alpha
    alpha^T)_ij dK_ij, summed as the device sums them -- lower triangle once, the diagonal with half weight."""
    u, alpha, S = np.asarray(u, dtype=T), np.asarray(alpha, dtype=T), np.asarray(S, dtype=T)
    n = len(u)
    low, dia = np.tril(np.ones((n, n), dtype=T), -1), np.eye(n, dtype=T)
    wb = (np.outer(u, alpha) + np.outer(alpha, u)) * (low + T(0.5) * dia)
    wn = (S - np.outer(alpha, alpha)) * (low + T(0.5) * dia)
    return (wb[None] * dK).sum(axis=(1, 2), dtype=T), (wn[None] * dK).sum(axis=(1, 2), dtype=T)
