"""Streamed against dense rolling means on the same fit, in one process: (a) a loadest-gp fit at n = 300 over a daily record of
40 years (m = 14 610) with "30D" (reach 30), (b) a rating-gp fit at n = 300 over a 15-minute stage record of the same length
with "7D" (reach 672) -- ``rolling_mean`` (``posterior_cov`` + ``window_moments``) against ``rolling_mean(streamed=True)``
under the default budget, wall milliseconds around whole calls (each ends in a device synchronise), both warmed, alternating,
median of the repeats, with the peak device bytes of one call of each and the largest relative difference of the Datasets --,
then (c) one 15-minute stage record the dense path cannot hold (``--long`` points, rating-gp at n = 500) through
``rolling_mean(streamed=True)`` with "7D" and "30D": wall time, the panel height picked, the peak device bytes.  Prints one JSON
line.  ``--m 0`` skips (a) and (b), ``--long 0`` skips (c), ``--windows 7D`` restricts (c) (for a profiler run), ``--rows 1024,4096``
adds to (c) a sweep of ``posterior_window_variances`` alone over these panel heights and the one the budget picks."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
os.environ["TQDM_DISABLE"] = "1"
from discontinuum_amd.loadest_gp import LoadestGP  # noqa: E402
from discontinuum_amd.rating_gp import RatingGP  # noqa: E402
from discontinuum_amd.rolling import record_windows  # noqa: E402
from discontinuum_amd.xr_compat import DataArray, Dataset  # noqa: E402
from scripts.exceedance_time import record  # noqa: E402


def stage_record(m, n, seed=0):
    """A 15-minute stage record of m points and n rated samples of it -> (model, record)."""
    rng = np.random.default_rng(seed)
    t = (np.datetime64("2015-01-01T00:00", "m") + 15 * np.arange(m)).astype("datetime64[ns]")
    stage_all = 1.0 + 3.0 * rng.beta(2, 5, m)
    pick = np.sort(rng.choice(m, n, replace=False))
    q = np.exp(1.6 * np.log(stage_all[pick]) + 0.05 * rng.standard_normal(n))
    obs = Dataset({"stage": ("time", stage_all[pick])}, coords={"time": t[pick]})
    target = DataArray(q, dims=("time",), coords={"time": t[pick]}, name="discharge", attrs={"units": "cfs"})
    unc = DataArray(np.full(n, 1.05), dims=("time",), coords={"time": t[pick]}, name="discharge_unc")
    model = RatingGP()
    model.fit(obs, target, target_unc=unc, iterations=3)
    return model, Dataset({"stage": ("time", stage_all)}, coords={"time": t})


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def peak(fn, plan):
    """Peak device bytes of one call, the plan's cached work areas of earlier calls released first (its own workspace stays)."""
    for k in [k for k in vars(plan) if k.endswith("_ws") and k != "_ws"]:
        setattr(plan, k, None)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated())


def geometry(model, rec, window):
    Xnew, _t, lo, hi, out = record_windows(model, rec, window)
    m, q, reach = int(Xnew.shape[0]), len(out), int((hi - lo).max())
    model._eval_ready(Xnew.to(model.device).contiguous())
    return m, q, reach, int(model._plan.window_panel_rows(m, q, reach))


def compare(model, rec, window, reps):
    m, q, reach, R = geometry(model, rec, window)
    fns = {"dense": lambda: model.rolling_mean(rec, window), "streamed": lambda: model.rolling_mean(rec, window, streamed=True)}
    ref, got = fns["dense"](), fns["streamed"]()  # warm
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(timed(fn)[1])
    row = {"window": window, "m": m, "q": q, "reach": reach, "panel_rows": R, "reps": reps}
    for k in fns:
        row[f"{k}_wall_ms"] = float(np.median(ms[k]))
        row[f"{k}_spread_ms"] = float(np.max(ms[k]) - np.min(ms[k]))
    for k, fn in fns.items():
        row[f"{k}_peak_bytes"] = peak(fn, model._plan)
    row["streamed_over_dense"] = row["streamed_wall_ms"] / row["dense_wall_ms"]
    row["max_rel_diff"] = {k: float(np.max(np.abs(got[k].values - ref[k].values) / np.abs(ref[k].values))) for k in ("mean", "se", "lower", "upper")}
    return row


def panel_sweep(model, rec, window, heights, reps=3):
    """Device milliseconds (HIP events, warmed, median) and work-area bytes of ``posterior_window_variances`` alone at the given
    panel heights -- the band's GEMM work per row is R / 2 + reach columns, the launches' parallelism grows with R."""
    Xnew, _t, lo, hi, _out = record_windows(model, rec, window)
    Xd = Xnew.to(model.device).contiguous()
    model._eval_ready(Xd)
    plan, theta = model._plan, model._factor_theta
    m, q, reach = int(Xd.shape[0]), len(lo), int((hi - lo).max())
    with torch.no_grad():
        mu = (plan.predict_mean(theta, Xd) + model.model.prior_mean(Xd)).contiguous()
    lo_t, hi_t = torch.from_numpy(lo), torch.from_numpy(hi)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rows = {}
    for R in heights:
        plan._pwv_ws = None
        ms = []
        for k in range(reps + 1):
            start.record()
            plan.posterior_window_variances(theta, Xd, mu, lo_t, hi_t, panel_rows=R)
            stop.record()
            stop.synchronize()
            if k:
                ms.append(start.elapsed_time(stop))
        rows[str(R)] = {"device_ms": float(np.median(ms)),
                        "work_bytes": int(plan.lib.dgp_posterior_window_variances_workspace_bytes(plan._h, m, q, reach, R))}
    plan._pwv_ws = None
    return rows


def long_case(m, n, windows, heights=()):
    model, rec = stage_record(m, n)
    row = {"n": n, "m": m, "dense_bytes_would_be": 8 * (-(-m // 128) * 128) ** 2}
    try:
        model.rolling_mean(rec, "7D")
        row["dense"] = "completed"
    except (ValueError, RuntimeError) as e:
        row["dense"] = f"refused: {str(e)[:200]}"
    for window in windows:
        _m, q, reach, R = geometry(model, rec, window)
        model.rolling_mean(rec, window, streamed=True)  # warm
        ds, ms = timed(lambda: model.rolling_mean(rec, window, streamed=True))
        row[window] = {"q": q, "reach": reach, "panel_rows": R, "streamed_wall_s": ms / 1e3,
                       "peak_device_bytes": peak(lambda: model.rolling_mean(rec, window, streamed=True), model._plan),
                       "mean_head": [float(v) for v in ds["mean"].values[:3]], "se_head": [float(v) for v in ds["se"].values[:3]]}
        if heights:
            row[window]["panel_sweep"] = panel_sweep(model, rec, window, list(heights) + [R])
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=14610)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--long", type=int, default=140000)
    ap.add_argument("--windows", default="7D,30D")
    ap.add_argument("--rows", default="", help="panel heights of a sweep on the long record, e.g. 1024,4096")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "window_stream_time.py measures on the GPU"
    out = {"script": "window_stream_time"}
    if a.m > 0:
        obs, target, daily = record(a.n, a.m)
        loadest = LoadestGP()
        loadest.fit(obs, target, iterations=3)
        out["daily_30D"] = compare(loadest, daily, "30D", a.reps)
        del loadest
        torch.cuda.empty_cache()
        rating, rec = stage_record(a.m, a.n)
        out["quarter_hour_7D"] = compare(rating, rec, "7D", a.reps)
        del rating
        torch.cuda.empty_cache()
    if a.long > 0:
        out["long"] = long_case(a.long, 500, [w for w in a.windows.split(",") if w], [int(r) for r in a.rows.split(",") if r])
    print(json.dumps(out))
