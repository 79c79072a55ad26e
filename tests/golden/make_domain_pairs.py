"""Writes tests/golden/domain_<model>_<corner>.npz: the covariance functions of loadest-gp (d = 2, 3), rating-gp and one
composite tree at the CORNERS of their hyperparameter domain, evaluated with mpmath at 40 digits (tests/test_domain_cpu.py,
tests/test_gpu_domain.py).

Independent of oracle/gp_oracle.py and of csrc/dgp_models.h: the entries are the textbook forms of SURVEY.md Appendix A.2,
    RBF exp(-1/2 sum (dx_j / l_j)^2),   Matern r = sqrt(sum (dx_j / l_j)^2): 1/2 e^-r, 3/2 (1 + sqrt3 r) e^(-sqrt3 r),
    5/2 (1 + sqrt5 r + 5 r^2 / 3) e^(-sqrt5 r),   Periodic exp(-2 sin^2(pi dx / p) / l),
composed per model (``entry_parts``).  The derivatives with respect to the hyperparameters are ``mp.diff`` of those entries
(central differences at raised precision), not hand-derived closed forms.  The derivatives with respect to the test point are
closed forms (Matern-3/2 is only C^1 at 0, which rules ``mp.diff`` out there); ``main`` checks them against ``mp.diff`` on
pairs that do not coincide before anything is written.

Every file holds numbers only:
    theta, X (n, d), Xs (m, d)                        inputs, X / Xs exactly representable in float32 (drawn, rounded, THEN
                                                      evaluated: one file serves the float64 and the float32 plans) and
                                                      stored as float32, like u, alpha, r and S_tril
    K_tril (n (n + 1) / 2,), Ks (n, m), kss (m,)      K(X, X) lower triangle by rows, K(X, Xs), k(x*, x*)
    parts (C, n, m), parts_kss (C, m)                 the additive parts of K(X, Xs) in ``terms()`` order and their k(x*, x*)
    slope_cols (Q,), dKs (Q, n, m)                    d K(X, Xs) / d x*_c for every differentiable column c
    prior (P (P + 1) / 2, m), P = 1 + Q               D_a D'_b k at x = x' = x* over (value, slope_cols), packed lower triangle
    u, alpha (n,), S_tril (n (n + 1) / 2,), r (n,)    seeded weights (float32-representable), S symmetric
    g_bil, g_bil_scale (ntheta,)                      sum_ij u_i dK_ij/dtheta_p alpha_j and sum_ij |u_i dK_ij/dtheta_p alpha_j|
    g_nll, g_nll_scale (ntheta,)                      1/2 sum_ij (S - alpha alpha^T)_ij dK_ij/dtheta_p and 1/2 sum_ij |...|
    sum_os ()                                         the sum of the outputscales (an unscaled term counts 1)
The composite's description (the integer list of ``dgp_composite_define``) is ``COMPOSITE_SPEC`` below, not in the files.

n = 72 (one full 64-row tile, one padded one), m = 20.  Corners: every lengthscale in 0.01 .. 0.05 or 40 .. 300, every
outputscale in 1e-5 .. 25, the period within 3 % of 1; rating's gate switch b inside the stages (centre, mixed), below all
of them (short) and above all of them (long).  ``mixedp`` is ``mixed`` with the period 3 % off 1: only there does a period that
float32 cannot represent meet a short periodic lengthscale AND a long Matern one, so that pairs decades apart still count.
Its periodic lengthscale is 0.5, not 0.02: with p != 1 the phase t (1 / p) of a point -- in the composite (t - t') (1 / p) of a
pair -- carries |t| 2^-53 in double from the rounding of 1 / p and of the product, the entry 4 / l times that, and at l = 0.02
the fp64 emulation of the formula alone is at 9.4e-14 (loadest d = 3) and 4.4e-14 (composite) of the outputscales, not at a
quarter of the 1e-13 bound.
``deep`` (rating only) is the centre with b = 40, where 1 - g underflows to zero at every stage.  Two input-edge cases per model at the centre: ``edge`` (two coincident rows,
a test point equal to a train point, a run of 15-minute spacings, a stage at the pipeline's clip value 1e-6) and
``edge2000`` (the same with every time offset by +2000, an unshifted decimal year; float32 cannot tell 15 minutes apart
there, so the run collapses onto neighbouring float32 values -- the reference is evaluated at what the plan receives).

mpmath here runs on Python integers: one fixture takes 20 s (loadest d = 2) to 1 minute (rating), all 29 and the batch
file (``build_batch``) about 4 minutes on 8 processes.
Run:  python tests/golden/make_domain_pairs.py [name ...]"""
import os
import sys
from multiprocessing import Pool

import mpmath as mp
import numpy as np

DPS = 40
mp.mp.dps = DPS
N, M = 72, 20
HERE = os.path.dirname(os.path.abspath(__file__))

# the composite tree: every factor kind of the interpreter, a Periodic factor inside a three-factor product, one unscaled
# term, d = 4.  (scaled, [(kind 0 RBF / 1 Matern / 2 Periodic, 2 nu, ard, columns)]); column 3 sees a Matern-1/2 factor.
COMPOSITE_TERMS = [
    (True, [(2, 0, False, (0,)), (1, 5, False, (0,)), (0, 0, True, (1, 2))]),
    (True, [(1, 3, True, (0, 1, 2))]),
    (False, [(1, 1, False, (3,)), (0, 0, False, (1, 2))]),
    (True, [(1, 5, False, (0, 1))]),
]
COMPOSITE_D = 4


def composite_spec():
    spec = [COMPOSITE_D, len(COMPOSITE_TERMS)]
    for scaled, factors in COMPOSITE_TERMS:
        spec += [int(scaled), len(factors)]
        for kind, nu2, ard, cols in factors:
            spec += [kind, nu2, int(ard), len(cols), *cols]
    return spec


COMPOSITE_SPEC = composite_spec()

# theta in the order of oracle/gp_oracle.py::loadest_gram / rating_gram / composite_gram
CORNERS = {
    "loadest3": {
        "centre": [1, 1, 1, 1, 1, .7, .7, .2, .2, .2, .2],
        "short": [4, .02, .97, .05, 9, .03, .03, 1, .01, .02, .02],
        "long": [1e-4, 50, 1.03, 300, 1e-3, 40, 40, 1e-5, 100, 80, 80],
        "mixed": [25, .02, 1, 300, 1e-4, .03, 40, 4, 100, .02, 80],
        "mixedp": [25, .5, .97, 300, 1e-4, .03, 40, 4, 100, .02, 80],
    },
    "loadest2": {
        "centre": [1, 1, 1, 1, 1, .7, .2, .2, .2],
        "short": [4, .02, .97, .05, 9, .03, 1, .01, .02],
        "long": [1e-4, 50, 1.03, 300, 1e-3, 40, 1e-5, 100, 80],
        "mixed": [25, .02, 1, 300, 1e-4, .03, 4, 100, .02],
        "mixedp": [25, .5, 1.03, 300, 1e-4, .03, 4, 100, .02],
    },
    # b, shift 1 (os, l_stage, l_time), shift 2, bend (os, l_stage, l_time), base (os, l_stage), periodic (os, l, p, l_matern)
    "rating": {
        "centre": [1.3, 1, 1, 1, 1, .7, .7, 1, 1, 1, .2, 1, .2, 1, 1, 1],
        "short": [0.1, 4, .02, .05, 9, .03, .01, 2, .04, .02, 1, .03, .5, .02, .97, .05],
        "long": [2.9, 1e-4, 50, 300, 1e-3, 40, 100, 1e-5, 80, 60, 1e-2, 200, 1e-4, 50, 1.03, 300],
        "mixed": [1.4, 25, .02, 300, 1e-4, 40, .03, 4, 100, .02, 1e-5, .05, 9, .02, 1, 300],
        "mixedp": [1.4, 25, .02, 300, 1e-4, 40, .03, 4, 100, .02, 1e-5, .05, 9, .5, 1.03, 300],
        # centre with b = 40: 20 (b - stage) > 709, so 1 - g underflows to zero in float64 and float32 alike at every stage
        # in 1 .. 2; one train and one test row have stage 41.5, on the other side of the switch (g = e^-30, 1 - g = 1: further out
        # g^2 leaves float32's range and the sums of the b derivative with it, which no float32 plan can be held to)
        "deep": [40, 1, 1, 1, 1, .7, .7, 1, 1, 1, .2, 1, .2, 1, 1, 1],
    },
    # term 0 (os, l_periodic, p, l_matern52, l_rbf x 2), term 1 (os, l x 3), term 2 (l_matern12, l_rbf), term 3 (os, l)
    "composite": {
        "centre": [1, 1, 1, 1, .7, .7, .2, .2, .2, .2, 1, 1, .5, 1],
        "short": [4, .02, .97, .05, .03, .03, 1, .01, .02, .02, .04, .03, 9, .05],
        "long": [1e-4, 50, 1.03, 300, 40, 40, 1e-5, 100, 80, 80, 60, 200, 1e-3, 150],
        "mixed": [25, .02, 1, 300, .03, 40, 4, 100, .02, 80, .05, 40, 1e-4, .02],
        "mixedp": [25, .5, .97, 300, .03, 40, 4, 100, .02, 80, .05, 40, 1e-4, .02],
    },
}
EDGES = ("edge", "edge2000")
MODEL_D = {"loadest2": 2, "loadest3": 3, "rating": 2, "composite": COMPOSITE_D}
CASES = [(model, corner) for model in CORNERS for corner in (*CORNERS[model], *EDGES)]


def case_name(model, corner):
    return f"domain_{model}_{corner}"


def case_theta(model, corner):
    return np.asarray(CORNERS[model]["centre" if corner in EDGES else corner], dtype=np.float64)


# ---- inputs -------------------------------------------------------------------------------------------------------------
def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def s32(a):
    """A float32-representable array as float32, for storage (half the bytes, the same numbers)."""
    out = np.asarray(a, dtype=np.float32)
    assert np.array_equal(out.astype(np.float64), a)
    return out


def draw_inputs(model, corner):
    """X (n, d), Xs (m, d), float32-representable.  Times uniform in +-16, covariates standard normal, stages 1 + Beta(2, 5)
    (oracle.synth_loadest / synth_rating); the last 12 train rows and the last 6 test rows lie within ~0.02 per column of an
    earlier train row, so that the short lengthscales see pairs at distances of their own size."""
    d = MODEL_D[model]
    rng = np.random.default_rng(abs(hash_name(model + corner)))

    def block(k):
        t = rng.uniform(-16.0, 16.0, k)
        rest = 1.0 + rng.beta(2.0, 5.0, (k, 1)) if model == "rating" else rng.standard_normal((k, d - 1))
        return np.concatenate([t[:, None], rest], axis=1)

    X = block(N)
    Xs = block(M)
    X[N - 12:] = X[:12] + 0.02 * rng.standard_normal((12, d))
    Xs[M - 6:] = X[20:26] + 0.02 * rng.standard_normal((6, d))
    if corner == "deep":
        X[40, 1] = Xs[3, 1] = 41.5
    if corner in EDGES:
        X[7] = X[3]                                        # two coincident rows
        Xs[2] = X[5]                                       # a train point equal to a test point
        X[30:36, 0] = X[30, 0] + 2.85e-5 * np.arange(6)    # a run of 15-minute spacings ...
        X[30:36, 1:] = X[30, 1:]                           # ... at one gauge reading
        Xs[4] = X[31]
        Xs[4, 0] += 2.85e-5 / 2
        if model == "rating":
            X[40, 1] = 1e-6                                # the pipeline's clip value
            Xs[6, 1] = 1e-6
        if corner == "edge2000":
            X[:, 0] += 2000.0
            Xs[:, 0] += 2000.0
    X, Xs = f32(X), f32(Xs)
    if corner in EDGES:  # rounding must not separate what has to coincide
        X[7], Xs[2] = X[3], X[5]
    return X, Xs


def hash_name(s):
    h = 0
    for ch in s:
        h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
    return h


def draw_weights(model, corner):
    rng = np.random.default_rng(hash_name("w" + model + corner))
    u, alpha, r = (f32(rng.standard_normal(N)) for _ in range(3))
    S = rng.standard_normal((N, N))
    S = f32((S + S.T) / 2)
    return u, alpha, r, S


# ---- the textbook factors: value and closed-form d / d x2_c ------------------------------------------------------------------
SQRT3, SQRT5 = mp.sqrt(3), mp.sqrt(5)


def rbf(dx, ls):
    return mp.exp(-sum((a / l) ** 2 for a, l in zip(dx, ls)) / 2)


def matern(dx, ls, nu2):
    r = mp.sqrt(sum((a / l) ** 2 for a, l in zip(dx, ls)))
    if nu2 == 1:
        return mp.exp(-r)
    if nu2 == 3:
        return (1 + SQRT3 * r) * mp.exp(-SQRT3 * r)
    return (1 + SQRT5 * r + 5 * r * r / 3) * mp.exp(-SQRT5 * r)


def periodic(dx, l, p):
    return mp.exp(-2 * mp.sin(mp.pi * dx / p) ** 2 / l)


def d_rbf(dx, ls, j):
    """d rbf / d x2_j with dx = x1 - x2."""
    return rbf(dx, ls) * dx[j] / ls[j] ** 2


def d_matern(dx, ls, nu2, j):
    r = mp.sqrt(sum((a / l) ** 2 for a, l in zip(dx, ls)))
    if nu2 == 3:
        return 3 * mp.exp(-SQRT3 * r) * dx[j] / ls[j] ** 2
    assert nu2 == 5
    return mp.mpf(5) / 3 * (1 + SQRT5 * r) * mp.exp(-SQRT5 * r) * dx[j] / ls[j] ** 2


def d_periodic(dx, l, p):
    return periodic(dx, l, p) * (2 * mp.pi / (p * l)) * mp.sin(2 * mp.pi * dx / p)


GATE_A = 20
CLIP = mp.mpf("1e-6")


def gates(s, b):
    """(g, 1 - g) of rating-gp's sigmoid gate, each from its own exponential (no 1 - g at 40 digits when g -> 1)."""
    x = GATE_A * (s - b)
    return 1 / (1 + mp.exp(x)), 1 / (1 + mp.exp(-x))


# ---- the models: additive parts of one entry ----------------------------------------------------------------------------------
def entry_parts(model, x1, x2, th):
    """The additive parts of k(x1, x2) in ``terms()`` order (mp numbers); the entry is their sum."""
    if model.startswith("loadest"):
        d = len(x1)
        dt = x1[0] - x2[0]
        dx = [a - b for a, b in zip(x1, x2)]
        return [th[0] * periodic(dt, th[1], th[2]) * matern([dt], [th[3]], 5),
                th[4] * rbf(dx[1:], th[5:4 + d]),
                th[4 + d] * matern(dx, th[5 + d:5 + 2 * d], 3)]
    if model == "rating":
        dt = x1[0] - x2[0]
        dw = mp.log(x1[1] + CLIP) - mp.log(x2[1] + CLIP)
        g1, h1 = gates(x1[1], th[0])
        g2, h2 = gates(x2[1], th[0])
        shift = [g1 * g2 * th[o] * matern([dw], [th[o + 1]], 5) * matern([dt], [th[o + 2]], 3) for o in (1, 4)]
        bend = h1 * h2 * th[7] * matern([dw], [th[8]], 5) * matern([dt], [th[9]], 5)
        base = th[10] * matern([dw], [th[11]], 5)
        per = th[12] * periodic(dt, th[13], th[14]) * matern([dt], [th[15]], 5)
        return [shift[0], shift[1], bend, base, per]
    out, t = [], 0
    for scaled, factors in COMPOSITE_TERMS:
        v = mp.mpf(1)
        if scaled:
            v = th[t]
            t += 1
        for kind, nu2, ard, cols in factors:
            dx = [x1[c] - x2[c] for c in cols]
            ls = th[t:t + len(cols)] if ard else [th[t]] * len(cols)
            t += len(cols) if ard else 1
            if kind == 0:
                v = v * rbf(dx, ls)
            elif kind == 1:
                v = v * matern(dx, ls, nu2)
            else:
                v = v * periodic(dx[0], ls[0], th[t])
                t += 1
        out.append(v)
    return out


def entry(model, x1, x2, th):
    return mp.fsum(entry_parts(model, x1, x2, th))


def slope_cols(model):
    return [0, 1, 2] if model == "composite" else list(range(MODEL_D[model]))


def entry_slope(model, x1, x2, th, c):
    """d k(x1, x2) / d x2_c in closed form (product and chain rules over the closed-form factor derivatives)."""
    if model.startswith("loadest"):
        d = len(x1)
        dx = [a - b for a, b in zip(x1, x2)]
        dt = dx[0]
        out = th[4 + d] * d_matern(dx, th[5 + d:5 + 2 * d], 3, c)
        if c == 0:
            out += th[0] * (d_periodic(dt, th[1], th[2]) * matern([dt], [th[3]], 5)
                            + periodic(dt, th[1], th[2]) * d_matern([dt], [th[3]], 5, 0))
        else:
            out += th[4] * d_rbf(dx[1:], th[5:4 + d], c - 1)
        return out
    if model == "rating":
        dt = x1[0] - x2[0]
        dw = mp.log(x1[1] + CLIP) - mp.log(x2[1] + CLIP)
        g1, h1 = gates(x1[1], th[0])
        g2, h2 = gates(x2[1], th[0])
        if c == 0:
            out = th[12] * (d_periodic(dt, th[13], th[14]) * matern([dt], [th[15]], 5)
                            + periodic(dt, th[13], th[14]) * d_matern([dt], [th[15]], 5, 0))
            for o in (1, 4):
                out += g1 * g2 * th[o] * matern([dw], [th[o + 1]], 5) * d_matern([dt], [th[o + 2]], 3, 0)
            return out + h1 * h2 * th[7] * matern([dw], [th[8]], 5) * d_matern([dt], [th[9]], 5, 0)
        wp = 1 / (x2[1] + CLIP)            # d log(stage + 1e-6) / d stage
        dg2 = -GATE_A * g2 * h2            # d gate / d stage; the inverted gate has the opposite sign
        out = wp * th[10] * d_matern([dw], [th[11]], 5, 0)
        for o in (1, 4):
            mt = matern([dt], [th[o + 2]], 3)
            out += g1 * th[o] * mt * (dg2 * matern([dw], [th[o + 1]], 5) + g2 * wp * d_matern([dw], [th[o + 1]], 5, 0))
        mt = matern([dt], [th[9]], 5)
        return out + h1 * th[7] * mt * (-dg2 * matern([dw], [th[8]], 5) + h2 * wp * d_matern([dw], [th[8]], 5, 0))
    total, t = mp.mpf(0), 0
    for scaled, factors in COMPOSITE_TERMS:
        os = mp.mpf(1)
        if scaled:
            os = th[t]
            t += 1
        vals, ders = [], []
        for kind, nu2, ard, cols in factors:
            dx = [x1[q] - x2[q] for q in cols]
            ls = th[t:t + len(cols)] if ard else [th[t]] * len(cols)
            t += len(cols) if ard else 1
            j = cols.index(c) if c in cols else None
            if kind == 0:
                vals.append(rbf(dx, ls))
                ders.append(d_rbf(dx, ls, j) if j is not None else 0)
            elif kind == 1:
                vals.append(matern(dx, ls, nu2))
                ders.append(d_matern(dx, ls, nu2, j) if j is not None else 0)
            else:
                vals.append(periodic(dx[0], ls[0], th[t]))
                ders.append(d_periodic(dx[0], ls[0], th[t]) if j is not None else 0)
                t += 1
        for f in range(len(vals)):
            prod = os * ders[f]
            for g in range(len(vals)):
                if g != f:
                    prod = prod * vals[g]
            total += prod
    return total


def prior_block(model, xs, th):
    """D_a D'_b k(x, x') at x = x' = xs over (value, slope_cols), as a full symmetric list of lists.  Mixed second derivatives
    at 0 of the stationary factors: RBF 1 / l^2, Matern-3/2 3 / l^2, Matern-5/2 5 / (3 l^2), Periodic 4 pi^2 / (p^2 l); every
    factor is 1 and has a vanishing first derivative at 0, so a product contributes the sum over its factors."""
    cols = slope_cols(model)
    P = 1 + len(cols)
    B = [[mp.mpf(0)] * P for _ in range(P)]
    per2 = lambda l, p: 4 * mp.pi ** 2 / (p ** 2 * l)  # noqa: E731
    m52 = lambda l: mp.mpf(5) / (3 * l ** 2)  # noqa: E731
    if model.startswith("loadest"):
        d = len(xs)
        B[0][0] = th[0] + th[4] + th[4 + d]
        B[1][1] = th[0] * (per2(th[1], th[2]) + m52(th[3])) + 3 * th[4 + d] / th[5 + d] ** 2
        for j in range(1, d):
            B[1 + j][1 + j] = th[4] / th[4 + j] ** 2 + 3 * th[4 + d] / th[5 + d + j] ** 2
        return B
    if model == "rating":
        g, h = gates(xs[1], th[0])
        dg = -GATE_A * g * h
        wp = 1 / (xs[1] + CLIP)
        lo0 = th[1] + th[4]
        lo_tt = 3 * th[1] / th[3] ** 2 + 3 * th[4] / th[6] ** 2
        lo_ww = th[1] * m52(th[2]) + th[4] * m52(th[5])
        B[0][0] = g * g * lo0 + h * h * th[7] + th[10] + th[12]
        B[1][1] = g * g * lo_tt + h * h * th[7] * m52(th[9]) + th[12] * (per2(th[13], th[14]) + m52(th[15]))
        B[2][0] = B[0][2] = g * dg * lo0 - h * dg * th[7]
        B[2][2] = dg * dg * (lo0 + th[7]) + wp * wp * (g * g * lo_ww + h * h * th[7] * m52(th[8]) + th[10] * m52(th[11]))
        return B
    t = 0
    for scaled, factors in COMPOSITE_TERMS:
        os = mp.mpf(1)
        if scaled:
            os = th[t]
            t += 1
        B[0][0] += os
        for kind, nu2, ard, fcols in factors:
            ls = th[t:t + len(fcols)] if ard else [th[t]] * len(fcols)
            t += len(fcols) if ard else 1
            for j, c in enumerate(fcols):
                if c not in cols:
                    continue
                w = 1 / ls[j] ** 2 if kind == 0 else per2(ls[j], th[t]) if kind == 2 else {3: 3 / ls[j] ** 2, 5: m52(ls[j])}[nu2]
                B[1 + cols.index(c)][1 + cols.index(c)] += os * w
            if kind == 2:
                t += 1
    return B


def sum_os(model, theta):
    if model.startswith("loadest"):
        d = MODEL_D[model]
        return float(theta[0] + theta[4] + theta[4 + d])
    if model == "rating":
        return float(theta[1] + theta[4] + theta[7] + theta[10] + theta[12])
    return float(theta[0] + theta[6] + 1.0 + theta[12])


# ---- one fixture ----------------------------------------------------------------------------------------------------------------
def mpv(a):
    return [mp.mpf(float(v)) for v in a]


def dtheta(model, x1, x2, th, p):
    """d k(x1, x2) / d theta_p by mp.diff of the entry."""
    def f(v):
        t = list(th)
        t[p] = v
        return entry(model, x1, x2, t)
    return mp.diff(f, th[p])


def tril_index(i, j):
    return i * (i + 1) // 2 + j


def build(model, corner):
    mp.mp.dps = DPS
    theta = case_theta(model, corner)
    X, Xs = draw_inputs(model, corner)
    u, alpha, r, S = draw_weights(model, corner)
    th, Xm, Xsm = mpv(theta), [mpv(row) for row in X], [mpv(row) for row in Xs]
    um, am = mpv(u), mpv(alpha)
    P = len(theta)
    cols = slope_cols(model)
    K_tril = np.empty(N * (N + 1) // 2)
    g_bil, s_bil, g_nll, s_nll = ([mp.mpf(0)] * P for _ in range(4))
    for i in range(N):
        for j in range(i + 1):
            K_tril[tril_index(i, j)] = float(entry(model, Xm[i], Xm[j], th))
            wb = um[i] * am[j] + um[j] * am[i] if i != j else um[i] * am[i]
            wn = (mp.mpf(float(S[i, j])) - am[i] * am[j]) * (1 if i != j else mp.mpf(1) / 2)
            for p in range(P):
                dk = dtheta(model, Xm[i], Xm[j], th, p)
                g_bil[p] += wb * dk
                s_bil[p] += (abs(um[i] * am[j]) + abs(um[j] * am[i]) if i != j else abs(wb)) * abs(dk)
                g_nll[p] += wn * dk
                s_nll[p] += abs(wn * dk)
    C = len(entry_parts(model, Xm[0], Xm[0], th))
    Ks, parts, dKs = np.empty((N, M)), np.empty((C, N, M)), np.empty((len(cols), N, M))
    for i in range(N):
        for j in range(M):
            ps = entry_parts(model, Xm[i], Xsm[j], th)
            Ks[i, j] = float(mp.fsum(ps))
            parts[:, i, j] = [float(v) for v in ps]
            dKs[:, i, j] = [float(entry_slope(model, Xm[i], Xsm[j], th, c)) for c in cols]
    kss, parts_kss, prior = np.empty(M), np.empty((C, M)), np.empty(((1 + len(cols)) * (2 + len(cols)) // 2, M))
    for j in range(M):
        ps = entry_parts(model, Xsm[j], Xsm[j], th)
        kss[j], parts_kss[:, j] = float(mp.fsum(ps)), [float(v) for v in ps]
        B = prior_block(model, Xsm[j], th)
        for a in range(1 + len(cols)):
            for b in range(a + 1):
                prior[tril_index(a, b), j] = float(B[a][b])
    np.savez_compressed(
        os.path.join(HERE, case_name(model, corner) + ".npz"), theta=theta, X=s32(X), Xs=s32(Xs), K_tril=K_tril, Ks=Ks, kss=kss,
        parts=parts, parts_kss=parts_kss, slope_cols=np.asarray(cols, dtype=np.int64), dKs=dKs, prior=prior, u=s32(u),
        alpha=s32(alpha), r=s32(r), S_tril=s32(S[np.tril_indices(N)]), g_bil=np.asarray([float(v) for v in g_bil]), g_bil_scale=np.asarray([float(v) for v in s_bil]),
        g_nll=np.asarray([float(v) for v in g_nll]), g_nll_scale=np.asarray([float(v) for v in s_nll]),
        sum_os=np.asarray(sum_os(model, theta)))
    return case_name(model, corner)


# ---- the batched sweep: ten loadest d = 3 sites, no two with the same hyperparameters -------------------------------------------
BATCH_N = 24
BATCH_EXTRA = [  # sites 5 .. 9 of tests/test_gpu_domain.py's batched plan; sites 0 .. 4 are the five corner fixtures
    [1e-4, 300, .99, .02, 25, 40, .03, 1e-5, .02, 100, .05],
    [9, .05, 1.02, 40, 4, .01, 300, 25, 80, 80, .02],
    [1, .03, 1.01, .02, 1e-3, .05, .01, 9, .04, .03, .01],
    [25, 300, .98, 40, 4, 100, 60, 1, 50, 200, 150],
    [1e-5, .01, 1, 100, 1, 300, .02, 1e-4, .03, .05, 40],
]


def build_batch(_=None):
    """domain_loadest3_batch.npz: per extra site theta, X (24, 3), u, alpha and the bilinear sums -- small sites of a ragged
    batch, only what ``GPPlan.bilinear`` is checked against."""
    mp.mp.dps = DPS
    model, B, P = "loadest3", len(BATCH_EXTRA), len(BATCH_EXTRA[0])
    X, u, alpha = np.empty((B, BATCH_N, 3)), np.empty((B, BATCH_N)), np.empty((B, BATCH_N))
    g_bil, s_bil = np.empty((B, P)), np.empty((B, P))
    for b in range(B):
        full = draw_inputs(model, f"batch{b}")[0]
        X[b] = np.concatenate([full[:BATCH_N // 2], full[N - BATCH_N // 2:]])  # twelve rows and their near copies
        u[b], alpha[b] = (v[:BATCH_N] for v in draw_weights(model, f"batch{b}")[:2])
        th, Xm, um, am = mpv(BATCH_EXTRA[b]), [mpv(row) for row in X[b]], mpv(u[b]), mpv(alpha[b])
        g, sc = [mp.mpf(0)] * P, [mp.mpf(0)] * P
        for i in range(BATCH_N):
            for j in range(BATCH_N):
                for p in range(P):
                    term = um[i] * dtheta(model, Xm[i], Xm[j], th, p) * am[j]
                    g[p] += term
                    sc[p] += abs(term)
        g_bil[b], s_bil[b] = [float(v) for v in g], [float(v) for v in sc]
    np.savez_compressed(os.path.join(HERE, "domain_loadest3_batch.npz"), theta=np.asarray(BATCH_EXTRA, dtype=np.float64), X=s32(X),
                        u=s32(u), alpha=s32(alpha), g_bil=g_bil, g_bil_scale=s_bil)
    return "domain_loadest3_batch"


def check_closed_forms():
    """The closed-form test-point derivatives against mp.diff of the entry, on pairs that do not coincide."""
    for model in CORNERS:
        for corner in ("centre", "mixed"):
            th = mpv(case_theta(model, corner))
            X, Xs = draw_inputs(model, corner)
            for i, j in ((0, 0), (5, 3), (N - 1, M - 1)):
                x1, x2 = mpv(X[i]), mpv(Xs[j])
                for c in slope_cols(model):
                    def f(v):
                        x = list(x2)
                        x[c] = v
                        return entry(model, x1, x, th)
                    ref, got = mp.diff(f, x2[c]), entry_slope(model, x1, x2, th, c)
                    # mp.diff differences the whole entry: its error is relative to the entry, not to the derivative
                    tol = mp.mpf(10) ** -25 * (abs(ref) + entry(model, x1, x2, th))
                    assert abs(ref - got) <= tol, (model, corner, i, j, c, ref, got)


def _build(args):
    return build(*args)


def main():
    want = set(sys.argv[1:])
    cases = [c for c in CASES if not want or case_name(*c) in want or case_name(*c)[len("domain_"):] in want]
    check_closed_forms()
    jobs = [(_build, c) for c in cases] + ([(build_batch, None)] if not want or "loadest3_batch" in want else [])
    with Pool(min(8, len(jobs))) as pool:
        for name in [r.get() for r in [pool.apply_async(f, (a,)) for f, a in jobs]]:
            print(name, os.path.getsize(os.path.join(HERE, name + ".npz")), flush=True)


if __name__ == "__main__":
    main()
