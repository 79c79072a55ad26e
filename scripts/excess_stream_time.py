"""Streamed against dense excess moments on the same fit, in one process: a loadest-gp fit at n = 300 over a daily record of 40
years (m = 14 610, P = 40) at L = 1 and L = 8 threshold levels -- ``posterior_cov`` + ``excess_moments`` against
``posterior_excess_moments`` at panels of M, 2048 and 512 rows; HIP events around each call, every shape warmed first, the
entries alternating, median of the repeats --, then one 15-minute stage record the dense path cannot hold (``--long`` points,
rating-gp at n = 500, yearly groups) through ``RatingGP.excess(streamed=True, weights=seconds)`` at one and at three levels, with
the wall time, the panel height picked and the peak device memory.  Prints one JSON line.  ``--long 0`` skips the long record,
``--rows 512`` restricts the panel heights (for a profiler run)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
os.environ["TQDM_DISABLE"] = "1"
from discontinuum_amd.excess import log_threshold  # noqa: E402
from discontinuum_amd.loadest_gp import LoadestGP  # noqa: E402
from discontinuum_amd.loads import period_groups, target_transform  # noqa: E402
from discontinuum_amd.rating_gp import RatingGP  # noqa: E402
from discontinuum_amd.xr_compat import DataArray, Dataset  # noqa: E402
from scripts.exceedance_time import record  # noqa: E402
from scripts.excess_time import alternate  # noqa: E402


def daily_case(m, n, rows, reps):
    obs, target, daily = record(n, m)
    model = LoadestGP()
    model.fit(obs, target, iterations=3)
    _order, groups, labels, _n, _d = period_groups(daily.coords["time"].values, np.ones(m), "YE")
    P = len(labels)
    Xnew = torch.tensor(model.dm.Xnew(daily), dtype=model.dtype).cuda().contiguous()
    model._ensure_factor()
    theta, plan = model._factor_theta, model._plan
    kmean, cov = plan.posterior_cov(theta, Xnew)
    mu = (kmean + model.model.prior_mean(Xnew)).detach().contiguous()
    _mode, s, t = target_transform(model.dm)
    mapped = (s * mu + t).contiguous()
    conc_mean = np.asarray(model.dm.y_t(mu.cpu().numpy()).values).reshape(-1)
    levels = np.quantile(conc_mean, np.linspace(0.2, 0.8, 8))
    w = torch.ones(m, dtype=torch.float64, device="cuda")
    g = torch.tensor(groups, device="cuda")
    M = -(-m // 128) * 128
    heights = rows or (M, 2048, 512)
    row = {"n": n, "m": m, "P": P, "pairs": m * (m - 1) // 2, "reps": reps}
    del cov  # (the dense entry below forms it again, as a dense call does)

    def dense(a):
        return plan.excess_moments(plan.posterior_cov(theta, Xnew)[1], m, mapped, s * s, a, w, g, P)

    for L in (1, 8):
        lv = levels[4:5] if L == 1 else levels
        a = torch.tensor(np.broadcast_to(log_threshold(lv)[:, None], (L, m)).copy(), device="cuda")
        fns = [lambda: dense(a), lambda: plan.posterior_cov(theta, Xnew)]
        fns += [lambda R=R: plan.posterior_excess_moments(theta, Xnew, mapped, s * s, a, w, g, P, panel_rows=R) for R in heights]
        ms, spread = alternate(fns, reps)
        row[f"dense_total_L{L}_ms"], row[f"posterior_cov_L{L}_ms"] = ms[0], ms[1]
        row[f"spread_L{L}_ms"] = spread
        ref = dense(a)
        for R, v in zip(heights, ms[2:]):
            row[f"streamed_R{R}_L{L}_ms"] = v
            row[f"streamed_R{R}_L{L}_over_dense"] = v / ms[0]
            got = plan.posterior_excess_moments(theta, Xnew, mapped, s * s, a, w, g, P, panel_rows=R)
            scale = ref[2].abs().max()  # the largest period total: the scale of a mean, its square of a covariance
            row[f"streamed_R{R}_L{L}_vs_dense"] = [float((got[0] - ref[0]).abs().max() / scale),
                                                   float((got[1] - ref[1]).abs().max() / scale ** 2)]
    return row


def long_case(m, n, seed=0):
    rng = np.random.default_rng(seed)
    t = (np.datetime64("2015-01-01T00:00", "m") + 15 * np.arange(m)).astype("datetime64[ns]")
    stage_all = 1.0 + 3.0 * rng.beta(2, 5, m)
    pick = np.sort(rng.choice(m, n, replace=False))
    stage = stage_all[pick]
    q = np.exp(1.6 * np.log(stage) + 0.05 * rng.standard_normal(n))
    obs = Dataset({"stage": ("time", stage)}, coords={"time": t[pick]})
    target = DataArray(q, dims=("time",), coords={"time": t[pick]}, name="discharge", attrs={"units": "cfs"})
    unc = DataArray(np.full(n, 1.05), dims=("time",), coords={"time": t[pick]}, name="discharge_unc")
    record_ = Dataset({"stage": ("time", stage_all)}, coords={"time": t})
    model = RatingGP()
    model.fit(obs, target, target_unc=unc, iterations=3)
    seconds = np.full(m, 900.0)
    kw = dict(weights=seconds)  # yearly flood volumes
    levels = np.quantile(q, [0.9, 0.5, 0.7])
    row = {"n": n, "m": m, "dense_bytes_would_be": 8 * (-(-m // 128) * 128) ** 2}
    try:
        model.excess(record_, threshold=float(levels[0]), **kw)
        row["dense"] = "completed"
    except (NotImplementedError, RuntimeError) as e:
        row["dense"] = f"refused: {str(e)[:160]}"
    for L in (1, 3):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        ds = model.excess(record_, threshold=levels[:L], streamed=True, **kw)
        torch.cuda.synchronize()
        P = ds["mean"].values.shape[1]
        row[f"L{L}"] = {"streamed_wall_s": time.perf_counter() - t0, "peak_device_bytes": int(torch.cuda.max_memory_allocated()),
                        "groups": P, "panel_rows": int(model._plan.excess_panel_rows(m, P, L)),
                        "mean": [float(v) for v in ds["mean"].values[:, 0]], "se": [float(v) for v in ds["se"].values[:, 0]],
                        "share": [float(v) for v in ds["share"].values[:, 0]]}
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=14610)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--long", type=int, default=140000)
    ap.add_argument("--rows", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "excess_stream_time.py measures on the GPU"
    out = {"script": "excess_stream_time", "daily": daily_case(a.m, a.n, [int(r) for r in a.rows.split(",") if r], a.reps)}
    if a.long > 0:
        out["long"] = long_case(a.long, 500)
    print(json.dumps(out))
