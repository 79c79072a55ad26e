#!/usr/bin/env python3
"""Generate tests/golden/censored_terms.npy (rows: z, then the four functions; a plain .npy because the oracle suites take
every *.npz of this directory for a fit-step fixture): the four pointwise functions of the censored (Tobit) likelihood,
    log Phi(z),  h = phi(z) / Phi(z),  h (z + h),  h [1 - (z + h)(z + 2 h)],
on z = -40, -39.95 .. 8 plus the far points -100, -300, -1000, with mpmath at 500 digits (the positive side cancels to
nothing at lower precision), rounded to float64.

    python tests/golden/make_censored_terms.py
"""
import os

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    mp.mp.dps = 500
    z = np.concatenate([np.round(np.arange(-800, 161) * 0.05, 2), [-100.0, -300.0, -1000.0]])
    rows = []
    for zi in z:
        x = mp.mpf(float(zi))
        Phi = mp.erfc(-x / mp.sqrt(2)) / 2
        h = mp.exp(-x * x / 2) / mp.sqrt(2 * mp.pi) / Phi
        rows.append([float(mp.log(Phi)), float(h), float(h * (x + h)), float(h * (1 - (x + h) * (x + 2 * h)))])
    np.save(os.path.join(HERE, "censored_terms.npy"), np.vstack([z[None, :], np.array(rows).T]))
    print("wrote", len(z), "points")


if __name__ == "__main__":
    main()
