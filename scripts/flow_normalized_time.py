"""Flow-normalized loads through the streamed period moments (``dgp_posterior_period_moments``) at record lengths of
Y = 10, 20, 34 years of daily points (m ~ 365 Y^2 FN points, P = Y years) and fits of n = 300, 1000, 4000 observations.
One JSON line per (Y, n): m, P, N, the streamed call's device time (warm, median of 3), the peak device bytes of the call,
its MFMA flops (2 N 128 x 64 per visited 128 x 64 tile pair, counted on the host from the group layout), the entries visited
and an ESTIMATE of their vector-ALU operations (no counters: entries x a per-entry figure), the fraction of the 78.6 TFLOP/s fp64 matrix peak, and at Y = 10 the
dense path's time (``dgp_posterior_cov`` + ``dgp_period_moments``) on the same points."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
os.environ["TQDM_DISABLE"] = "1"
from discontinuum_amd import loads  # noqa: E402
from discontinuum_amd.loadest_gp import LoadestGP  # noqa: E402
from discontinuum_amd.xr_compat import DataArray, Dataset  # noqa: E402

PEAK = 78.6e12
VALU_PER_ENTRY = 109 + 28  # an estimate: bench.py's per-entry gram_sym figure (loadest d = 3) + expm1; not a measurement


def record(years, n, seed=0):
    rng = np.random.default_rng(seed)
    days = years * 365 + years // 4
    t = (np.datetime64("1990-01-01", "D") + np.arange(days)).astype("datetime64[ns]")
    season = np.sin(2 * np.pi * np.arange(days) / 365.25)
    flow = np.exp(1.0 + 0.6 * season + 0.4 * rng.standard_normal(days)) * 10
    pick = np.sort(rng.choice(days, n, replace=n > days))  # (several samples a day when n exceeds the days)
    conc = np.exp(0.3 * np.log(flow[pick]) + 0.2 * rng.standard_normal(n))
    units = {"units": "cubic meters per second"}
    obs = Dataset({"flow": ("time", flow[pick], units)}, coords={"time": t[pick]})
    target = DataArray(conc, dims=("time",), coords={"time": t[pick]}, name="concentration", attrs={"units": "mg/l"})
    return obs, target, Dataset({"flow": ("time", flow, units)}, coords={"time": t})


def device_ms(fn, reps=3):
    fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        out.append(start.elapsed_time(stop))
    return float(np.median(out))


def visited(groups, m, P):
    """(tile pairs, entries) of ppm_rows_kernel: row block I (128 rows) visits every 64-column tile of every group h >= its
    lowest."""
    M = -(-m // 128) * 128
    lo = np.full(M // 128, P)
    np.minimum.at(lo, np.arange(m) // 128, groups)
    first = np.searchsorted(groups, np.arange(P), side="left")
    last = np.searchsorted(groups, np.arange(P), side="right")
    tiles_h = np.where(last > first, (last - 1) // 64 - first // 64 + 1, 0)
    suffix = np.concatenate([np.cumsum(tiles_h[::-1])[::-1], [0]])
    pairs = int(suffix[np.minimum(lo, P)].sum())
    return pairs, pairs * 128 * 64


def one(years, n):
    obs, target, daily = record(years, n)
    model = LoadestGP()
    model.fit(obs, target, iterations=2)
    pts = loads.flow_normalized_points(daily)
    m, P = len(pts["flow"]), len(pts["labels"])
    mode, s, t = loads.target_transform(model.dm)
    Xnew = torch.tensor(model.dm.Xnew(Dataset({"flow": ("time", pts["flow"])}, coords={"time": pts["time"]})),
                        dtype=torch.float64).cuda().contiguous()
    model._ensure_factor()
    plan, theta = model._plan, model._factor_theta
    with torch.no_grad():
        mu = (s * (plan.predict_mean(theta, Xnew) + model.model.prior_mean(Xnew)) + t).contiguous()
    w = torch.tensor(pts["weight"], device="cuda")
    g = torch.tensor(pts["group"], device="cuda")
    run = lambda: plan.posterior_period_moments(theta, Xnew, mu, s * s, w, g, P, mode)  # noqa: E731
    run()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    ms = device_ms(run)
    pairs, entries = visited(pts["group"], m, P)
    flops = 2.0 * plan.N * 128 * 64 * pairs
    row = {"years": years, "n": n, "m": m, "P": P, "N": plan.N, "streamed_ms": ms,
           "peak_bytes": int(torch.cuda.max_memory_allocated() - base + plan._ppm_ws.numel()), "tile_pairs": pairs,
           "mfma_flops": flops, "entries": entries, "valu_ops_estimate": entries * VALU_PER_ENTRY,
           "frac_fp64_matrix_peak": flops / (ms * 1e-3) / PEAK}
    if years == 10:
        def dense():
            _k, cov = plan.posterior_cov(theta, Xnew)
            return plan.period_moments(cov, m, mu, s * s, w, g, P, mode)
        row["dense_ms"] = device_ms(dense)
    del plan, model
    torch.cuda.empty_cache()
    return row


if __name__ == "__main__":
    assert torch.cuda.is_available(), "flow_normalized_time.py measures on the GPU"
    for years in (10, 20, 34):
        for n in (300, 1000, 4000):
            print(json.dumps({"script": "flow_normalized_time", **one(years, n)}), flush=True)
