#!/usr/bin/env python
"""Timings of the path-count sweep and of ``exceedance_distribution`` for EXPERIMENTS.md ("Path-count sweep"), each beside the
orthant sweep at the same sizes IN THE SAME SESSION and beside joint draws counted in torch:

  * one ``path_counts`` call at m = 366 with 16 levels x 16 shifts x 4096 points, and at m = 8760 with 1 level x 16 x 4096 (HIP
    events: two warm-up calls, then the median of ``REPEATS``), the same for ``orthant_probability``, the time m^2 N shifts flop
    per level chunk take at the fp64 matrix peak, and the torch alternative at the same number of paths: f = L z with z ~ N(0, I)
    (m x n doubles held whole), a comparison per level and a sum -- the counts only, no spells;
  * ``exceedance_distribution`` for a 30-year daily record at 16 levels, split into covariance, factorisations, sweeps and the
    host's statistics, beside ``extreme_probability`` at the same sizes and ``sample(n)`` plus counting in numpy.

    python scripts/counts_time.py [--quick]        one JSON line per measurement
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
from tests.extremes_helpers import factor_layout, smooth_cov  # noqa: E402

PEAK_FP64_MATRIX = 157.3e12  # MI355X, flop / s
REPEATS = 5


def event_ms(fn, repeats=REPEATS):
    """Median of ``repeats`` event-timed calls after two warm-up calls (the first allocates the work area)."""
    fn()
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), [round(t, 3) for t in times], out


def torch_counts(Ld, m, thr_d, paths, above=True):
    """The alternative a user has today, at plan level: joint draws held whole, compared and summed per level."""
    z = torch.randn(m, paths, dtype=torch.float64, device=Ld.device)
    f = torch.tril(Ld[:m, :m]) @ z
    out = []
    for l in range(thr_d.shape[0]):
        e = f > thr_d[l][:, None] if above else f < thr_d[l][:, None]
        out.append(torch.bincount(e.sum(dim=0), minlength=m + 1))
    return torch.stack(out)


def sweep_case(dev, m, nlev, nshifts, npoints, ell):
    Lm = np.linalg.cholesky(smooth_cov(m, ell=ell))
    sd = np.sqrt(np.sum(Lm * Lm, axis=1))
    thr = np.linspace(1.0, 3.0, nlev)[:, None] * sd[None, :]
    Ld = torch.tensor(factor_layout(Lm, poison=False), dtype=torch.float64, device=dev)
    link = np.ones(m, dtype=np.int32)
    ms, all_ms, (ch, sh) = event_ms(lambda: B.path_counts(Ld, m, thr, above=True, link=link, npoints=npoints, nshifts=nshifts, seed=0))
    lo = np.full_like(thr, -np.inf)
    oms, oall, (prob, se) = event_ms(lambda: B.orthant_probability(Ld, m, lo, thr, npoints=npoints, nshifts=nshifts, seed=0))
    thr_d = torch.tensor(thr, device=dev)
    tms, tall, _ = event_ms(lambda: torch_counts(Ld, m, thr_d, npoints * nshifts))
    chunks = -(-nlev // B.PATH_COUNT_LEVEL_GROUP)
    flop = float(m) ** 2 * npoints * nshifts * chunks
    p0 = ch[:, :, 0].double().mean(dim=1) / npoints  # P(N = 0) per level, beside the orthant estimate of the same number
    return dict(what="path_counts", m=m, levels=nlev, shifts=nshifts, points=npoints, gpu_ms=round(ms, 3), gpu_ms_all=all_ms,
                orthant_ms=round(oms, 3), orthant_ms_all=oall, torch_draws_ms=round(tms, 3), torch_draws_ms_all=tall,
                peak_ms=round(1e3 * flop / PEAK_FP64_MATRIX, 3), share_of_peak=round(1e3 * flop / PEAK_FP64_MATRIX / ms, 3),
                p_none=[float(p0[0]), float(p0[-1])], orthant_prob=[float(prob[0]), float(prob[-1])],
                work_bytes=B.path_count_level_chunks(m, nlev, nshifts, npoints, 1 << 60)[1] * chunks,
                draws_bytes=8 * m * npoints * nshifts)


def end_to_end(dev, years, nlev, draws):
    from discontinuum_amd.loadest_gp import LoadestGP
    from tests.flux_helpers import daily_loadest

    cov_obs, target, daily = daily_loadest(n_obs=500, start="1990-01-01", end=f"{1990 + years}-01-01", seed=1)
    model = LoadestGP()
    model.fit(cov_obs, target, iterations=5)
    levels = np.quantile(np.asarray(target.values), np.linspace(0.5, 0.99, nlev))
    model.exceedance_distribution(cov_obs, threshold=levels[:2], npoints=256, nshifts=2)  # (warm-up on the sampling days)
    model.extreme_probability(cov_obs, threshold=levels[:2], npoints=256, nshifts=2)
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
    timed(plan, "path_counts", "sweeps_s")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    wall(lambda: model.exceedance_distribution(daily, threshold=levels))  # warm: the work areas are allocated
    spent.clear()
    total, ds = wall(lambda: model.exceedance_distribution(daily, threshold=levels))
    parts = dict(spent)
    ext_s, _ = wall(lambda: model.extreme_probability(daily, threshold=levels))
    ext_s, _ = wall(lambda: model.extreme_probability(daily, threshold=levels))

    def sample_and_count():
        sim = np.asarray(model.sample(daily, n=draws).values)  # (draws, m) in data space
        year = daily.coords["time"].values.astype("datetime64[Y]").astype(int)
        return [[(sim[:, year == y] > lv).sum(axis=1) for y in np.unique(year)] for lv in levels]

    sample_s, _ = wall(sample_and_count)
    return dict(what="exceedance_distribution", years=years, days=int(ds["n_points"].values.sum()), levels=nlev, total_s=round(total, 3),
                **{k: round(v, 3) for k, v in parts.items()}, other_s=round(total - sum(parts.values()), 3),
                extreme_probability_s=round(ext_s, 3), sample_and_count_s=round(sample_s, 3), sample_draws=draws,
                paths=int(ds.attrs["npoints"] * ds.attrs["nshifts"]), max_cdf_error=float(np.nanmax(ds["cdf_error"].values)),
                max_mean_error=float(np.nanmax(ds["mean_error"].values)), jitter=ds.attrs["jitter"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small shapes (a check that the script runs)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.quick:
        print(json.dumps(sweep_case(dev, 130, 2, 2, 256, 10.0)), flush=True)
        print(json.dumps(end_to_end(dev, 2, 2, 256)), flush=True)
        return
    print(json.dumps(sweep_case(dev, 366, 16, 16, 4096, 30.0)), flush=True)
    print(json.dumps(sweep_case(dev, 8760, 1, 16, 4096, 720.0)), flush=True)
    print(json.dumps(end_to_end(dev, 30, 16, 16384)), flush=True)


if __name__ == "__main__":
    main()
