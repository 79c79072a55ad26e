"""Writes tests/golden/excess_pairs.npy: Cov(e_i, e_j) of the excesses e = (c - tau)^+ (column ``above`` = 1) or deficits
(tau - c)^+ (0) of two jointly lognormal values over their thresholds, by 30-digit quadrature with mpmath -- independent of
the four-term form the library and tests/excess_helpers.py use.

With X = ln c_i ~ N(m_i, v_i) and Y | X = x ~ N(m_j + (c_ij / v_i)(x - m_i), v_j - c_ij^2 / v_i), the inner expectation is
the conditional Black-Scholes mean B(x) = E[(e^Y - tau_j)^+ | x] (closed form), and
    E e_i e_j = int_{x >= a_i} (e^x - tau_i) B(x) N(x; m_i, v_i) dx       (x <= a_i and the put for the deficit),
    Cov = E e_i e_j - E e_i E e_j,   E e = the marginal Black-Scholes mean.
The integrand has a kink of width ~ sqrt(1 - rho^2) where the conditional mean crosses a_j: the interval is split there.

Rows: m_i, v_i, a_i, m_j, v_j, a_j, c_ij, above, cov.  rho in +-{1e-8, 0.3, 0.75, 0.9249, 0.9251, 0.99, 0.9999}; v from
0.02 to 1; thresholds within +-3 sigma of the mean, plus |z| = 8.  Run:  python tests/golden/make_excess_pairs.py"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 30
RHOS = (1e-8, 0.3, 0.75, 0.9249, 0.9251, 0.99, 0.9999)
PER = 10  # pairs per (rho, sign, above)


def ncdf(x):
    return mp.erfc(-x / mp.sqrt(2)) / 2


def bs_mean(mean, var, a, above):
    """E (e^Y - e^a)^+ (above) or E (e^a - e^Y)^+ for Y ~ N(mean, var)."""
    s = mp.sqrt(var)
    d1, d0 = (mean + var - a) / s, (mean - a) / s
    if above:
        return mp.exp(mean + var / 2) * ncdf(d1) - mp.exp(a) * ncdf(d0)
    return mp.exp(a) * ncdf(-d0) - mp.exp(mean + var / 2) * ncdf(-d1)


def pair_cov(mi, vi, ai, mj, vj, aj, c, above):
    mi, vi, ai, mj, vj, aj, c = (mp.mpf(float(x)) for x in (mi, vi, ai, mj, vj, aj, c))
    si = mp.sqrt(vi)
    beta, cvar = c / vi, vj - c * c / vi
    csd = mp.sqrt(cvar)

    def f(x):
        pay = (mp.exp(x) - mp.exp(ai)) if above else (mp.exp(ai) - mp.exp(x))
        return pay * bs_mean(mj + beta * (x - mi), cvar, aj, above) * mp.exp(-(x - mi) ** 2 / (2 * vi)) / (si * mp.sqrt(2 * mp.pi))

    lo, hi = (ai, mi + vi + 14 * si) if above else (mi - 14 * si, ai)
    pts = {lo, hi}
    for q in (mi, mi + vi, mi + 2 * vi):
        for d in (-6, -3, -1, 0, 1, 3, 6):
            pts.add(q + d * si)
    if abs(beta) > 0:
        kink, width = mi + (aj - mj) / beta, csd / abs(beta)
        for d in (-40, -12, -6, -3, -1, 0, 1, 3, 6, 12, 40):
            pts.add(kink + d * width)
            pts.add(kink - cvar / beta + d * width)
    pts = sorted(p for p in pts if lo <= p <= hi)
    second = mp.quad(f, pts, maxdegree=10)
    return second - bs_mean(mi, vi, ai, above) * bs_mean(mj, vj, aj, above)


def main():
    rng = np.random.default_rng(20240917)
    rows = []
    for r0 in RHOS:
        for sign in (1.0, -1.0):
            for above in (1, 0):
                for q in range(PER):
                    vi, vj = np.exp(rng.uniform(np.log(0.02), np.log(1.0), 2))
                    mi, mj = rng.uniform(-0.5, 0.5, 2)
                    zi, zj = rng.uniform(-3, 3, 2)
                    if q == PER - 2:
                        zi = 8.0 * rng.choice([-1.0, 1.0])
                    if q == PER - 1:
                        zi, zj = 8.0 * rng.choice([-1.0, 1.0], 2)
                    if q == 0:
                        vi, vj = 1.0, 0.02
                    if q == 1:
                        vi, vj = 0.02, 0.02
                    ai, aj = mi + zi * np.sqrt(vi), mj + zj * np.sqrt(vj)
                    c = sign * r0 * np.sqrt(vi * vj)
                    rows.append([mi, vi, ai, mj, vj, aj, c, above, float(pair_cov(mi, vi, ai, mj, vj, aj, c, bool(above)))])
    out = np.asarray(rows, dtype=np.float64)
    np.save(os.path.join(os.path.dirname(os.path.abspath(__file__)), "excess_pairs.npy"), out)
    print(out.shape, out.nbytes)


if __name__ == "__main__":
    main()
