#!/usr/bin/env python
"""Timings of the orthant sweep and of ``extreme_probability`` for EXPERIMENTS.md ("Orthant sweep"):

  * one ``orthant_probability`` call at m = 366 with 16 levels x 16 shifts x 4096 points, and at m = 8760 with 1 level x 16 x 4096
    (HIP events, the second of two calls), beside the numpy restatement of tests/extremes_helpers.py on the same box (timed on a
    slice of the problem and scaled: the restatement is linear in levels and points) and the time m^2 N shifts levels flop take
    at the fp64 matrix peak;
  * the share of the diagonal-block steps: a call at m = 64 runs ONE diagonal block and no product at all, and every block of
    a longer sweep runs the same 64 steps, so the share is blocks x T(m = 64) / T(m);
  * ``extreme_probability`` for a 30-year daily record at 16 levels, split into covariance, factorisations and sweeps.

    python scripts/extremes_time.py [--quick]        one JSON line per measurement
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from discontinuum_amd import backend as B  # noqa: E402
from tests.extremes_helpers import factor_layout, orthant_ref, smooth_cov  # noqa: E402

PEAK_FP64_MATRIX = 157.3e12  # MI355X, flop / s


def event_ms(fn):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def sweep_case(dev, m, nlev, nshifts, npoints, ell, ref_levels, ref_shifts, ref_points):
    Lm = np.linalg.cholesky(smooth_cov(m, ell=ell))
    sd = np.sqrt(np.sum(Lm * Lm, axis=1))
    hi = np.linspace(1.0, 3.0, nlev)[:, None] * sd[None, :]
    lo = np.full_like(hi, -np.inf)
    Ld = torch.tensor(factor_layout(Lm, poison=False), dtype=torch.float64, device=dev)
    ms, (prob, se) = event_ms(lambda: B.orthant_probability(Ld, m, lo, hi, npoints=npoints, nshifts=nshifts, seed=0))
    L64 = torch.tensor(factor_layout(Lm[:64, :64], poison=False), dtype=torch.float64, device=dev)
    ms64, _ = event_ms(lambda: B.orthant_probability(L64, 64, lo[:, :64], hi[:, :64], npoints=npoints, nshifts=nshifts, seed=0))
    gen, sh = B.richtmyer_generators(m), B.orthant_shifts(m, nshifts, 0).numpy()
    t0 = time.perf_counter()
    for l in range(ref_levels):
        rp, rs = orthant_ref(Lm, lo[l], hi[l], gen, sh[:ref_shifts], ref_points)
    cpu_s = (time.perf_counter() - t0) * (nlev / ref_levels) * (nshifts / ref_shifts) * (npoints / ref_points)
    flop = float(m) ** 2 * npoints * nshifts * nlev
    blocks = m / 64.0
    return dict(what="orthant_probability", m=m, levels=nlev, shifts=nshifts, points=npoints, gpu_ms=round(ms, 3),
                cpu_restatement_s=round(cpu_s, 1), cpu_scaled_from=[ref_levels, ref_shifts, ref_points], peak_ms=round(1e3 * flop / PEAK_FP64_MATRIX, 3),
                one_block_ms=round(ms64, 3), diagonal_share=round(blocks * ms64 / ms, 3), prob=[float(prob[0]), float(prob[-1])],
                se=[float(se[0]), float(se[-1])], work_bytes=B.orthant_level_chunks(m, nlev, nshifts, npoints, 1 << 60)[1] * nlev)


def end_to_end(dev, years, nlev):
    from discontinuum_amd.loadest_gp import LoadestGP
    from tests.flux_helpers import daily_loadest

    cov_obs, target, daily = daily_loadest(n_obs=500, start="1990-01-01", end=f"{1990 + years}-01-01", seed=1)
    model = LoadestGP()
    model.fit(cov_obs, target, iterations=5)
    levels = np.quantile(np.asarray(target.values), np.linspace(0.5, 0.99, nlev))
    model.extreme_probability(cov_obs, threshold=levels[:2], npoints=256, nshifts=2)  # (warm-up on the sampling days: small blocks)
    spent = {}

    def timed(obj, name, key):
        fn = getattr(obj, name)

        def wrapper(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            spent[key] = spent.get(key, 0.0) + time.perf_counter() - t0
            return out

        setattr(obj, name, wrapper)

    plan = model._plan
    timed(plan, "posterior_cov", "covariance_s")
    timed(plan, "psd_safe_factor", "factorisations_s")
    timed(plan, "orthant_probability", "sweeps_s")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ds = model.extreme_probability(daily, threshold=levels)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    err = ds["error"].values
    return dict(what="extreme_probability", years=years, days=int(ds["n_points"].values.sum()), levels=nlev, total_s=round(total, 3),
                **{k: round(v, 3) for k, v in spent.items()}, other_s=round(total - sum(spent.values()), 3),
                max_error=float(np.nanmax(err)), jitter=ds.attrs["jitter"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small shapes (a check that the script runs)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.quick:
        print(json.dumps(sweep_case(dev, 130, 2, 2, 256, 10.0, 1, 2, 256)), flush=True)
        print(json.dumps(end_to_end(dev, 2, 2)), flush=True)
        return
    print(json.dumps(sweep_case(dev, 366, 16, 16, 4096, 30.0, 1, 16, 4096)), flush=True)
    print(json.dumps(sweep_case(dev, 8760, 1, 16, 4096, 720.0, 1, 2, 128)), flush=True)
    print(json.dumps(end_to_end(dev, 30, 16)), flush=True)


if __name__ == "__main__":
    main()
