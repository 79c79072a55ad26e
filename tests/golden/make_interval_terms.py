#!/usr/bin/env python3
"""Generate tests/golden/interval_terms.npy (rows: za, Delta, then the four functions; a plain .npy like censored_terms.npy):
the pointwise functions of the interval-censored likelihood of a row whose truth lies in [za, zb] (standardised, zb = za + Delta),
    P = Phi(zb) - Phi(za),  ra = phi(za) / P,  rb = phi(zb) / P,
    log P,   sigma g = ra - rb,   W v = zb rb - za ra + (ra - rb)^2,
    sigma^3 d3 = ra (za^2 - 1) - rb (zb^2 - 1) - (ra - rb)(za ra - zb rb) + 2 (ra - rb) W v,
on za = -40, -39.5 .. 38 and a few values off that grid, Delta in {1e-6, 1e-4, 1e-3, 1e-2, 0.1, 1, 5, 30} with zb <= 40, plus the
far points za = -100, -300, -1000 (every Delta) at the end.  za and Delta are taken AS ROUNDED TO DOUBLE and zb = za + Delta is
formed exactly; mpmath at 600 digits (P is a difference of two tails that agree to ~ Delta |z| and underflow any fixed format; at 60
digits z = 30 already fails), rounded to float64.

    python tests/golden/make_interval_terms.py
"""
import os

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DELTAS = (1e-6, 1e-4, 1e-3, 1e-2, 0.1, 1.0, 5.0, 30.0)
OFF_GRID = (-7.3, -2.6, -0.75, -0.05, -1e-3, 0.05, 0.31, 1.7, 6.9)
FAR = (-100.0, -300.0, -1000.0)


def exact(za, delta):
    """The four functions of (za, Delta) given as Python floats, in the working precision of mpmath."""
    a = mp.mpf(float(za))
    b = a + mp.mpf(float(delta))
    r2 = mp.sqrt(2)
    # the smaller tails of both ends: no precision is spent on a leading 1
    P = (mp.erfc(-b / r2) - mp.erfc(-a / r2)) / 2 if a + b < 0 else (mp.erfc(a / r2) - mp.erfc(b / r2)) / 2
    phi = lambda x: mp.exp(-x * x / 2) / mp.sqrt(2 * mp.pi)  # noqa: E731
    ra, rb = phi(a) / P, phi(b) / P
    mu = ra - rb
    wv = b * rb - a * ra + mu * mu
    d3 = ra * (a * a - 1) - rb * (b * b - 1) - mu * (a * ra - b * rb) + 2 * mu * wv
    return mp.log(P), mu, wv, d3


def grid():
    za = np.concatenate([np.arange(-80, 77) * 0.5, OFF_GRID])
    near = [(a, d) for a in za for d in DELTAS if a + d <= 40.0]
    far = [(a, d) for a in FAR for d in DELTAS]
    return np.array(near + far), len(far)


def main():
    mp.mp.dps = 600
    pts, _nfar = grid()
    vals = np.array([[float(v) for v in exact(a, d)] for a, d in pts])
    np.save(os.path.join(HERE, "interval_terms.npy"), np.vstack([pts.T, vals.T]))
    print("wrote", len(pts), "points")


if __name__ == "__main__":
    main()
