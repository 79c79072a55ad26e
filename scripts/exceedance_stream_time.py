"""Streamed against dense exceedance moments on the same fit, in one process: a loadest-gp fit at n = 300 over a daily record
of 40 years (m = 14 610, P = 40) at L = 1 and L = 16 levels -- ``posterior_cov`` + ``exceedance_moments`` against
``posterior_exceedance_moments`` at several panel heights --, then one rating-gp stage record the dense path cannot hold
(``--long`` points, n = 500, one group: a flow-duration curve) through ``RatingGP.duration_curve(streamed=True)`` with its
peak device memory.  Prints one JSON line.  ``--long 0`` skips the long record, ``--rows 512`` restricts the panel heights (for a
profiler run)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
os.environ["TQDM_DISABLE"] = "1"
from discontinuum_amd.exceedance import model_space_threshold  # noqa: E402
from discontinuum_amd.loadest_gp import LoadestGP  # noqa: E402
from discontinuum_amd.loads import period_groups  # noqa: E402
from discontinuum_amd.rating_gp import RatingGP  # noqa: E402
from discontinuum_amd.xr_compat import DataArray, Dataset  # noqa: E402
from exceedance_time import device_ms, record  # noqa: E402


def daily_case(m, n, rows):
    obs, target, daily = record(n, m)
    model = LoadestGP()
    model.fit(obs, target, iterations=3)
    order, groups, labels, _n, _d = period_groups(daily.coords["time"].values, np.ones(m), "YE")
    P = len(labels)
    Xnew = torch.tensor(model.dm.Xnew(daily), dtype=model.dtype).cuda().contiguous()
    model._ensure_factor()
    theta, plan = model._factor_theta, model._plan
    kmean, cov = plan.posterior_cov(theta, Xnew)
    mu = (kmean + model.model.prior_mean(Xnew)).detach().contiguous()
    conc_mean = np.asarray(model.dm.y_t(mu.cpu().numpy()).values).reshape(-1)
    levels = np.quantile(conc_mean, np.linspace(0.2, 0.8, 16))
    w = torch.ones(m, dtype=torch.float64, device="cuda")
    g = torch.tensor(groups, device="cuda")
    M = -(-m // 128) * 128
    row = {"n": n, "m": m, "P": P, "posterior_cov_ms": device_ms(lambda: plan.posterior_cov(theta, Xnew), 3)}
    for L in (1, 16):
        u = torch.tensor(np.broadcast_to(model_space_threshold(model.dm, levels[8:9] if L == 1 else levels)[:, None], (L, m)).copy(),
                         device="cuda")
        dense = plan.exceedance_moments(cov, m, mu, u, w, g, P)
        row[f"dense_moments_L{L}_ms"] = device_ms(lambda: plan.exceedance_moments(cov, m, mu, u, w, g, P), 5)
        row[f"dense_total_L{L}_ms"] = row[f"dense_moments_L{L}_ms"] + row["posterior_cov_ms"]
        row["predict_ms"] = device_ms(lambda: plan.predict(theta, Xnew), 3)
        for R in rows or (512, 2048, M):
            got = plan.posterior_exceedance_moments(theta, Xnew, mu, u, w, g, P, panel_rows=R)
            row[f"streamed_R{R}_L{L}_ms"] = device_ms(lambda: plan.posterior_exceedance_moments(theta, Xnew, mu, u, w, g, P, panel_rows=R), 3)
            W = m / P
            row[f"streamed_R{R}_L{L}_vs_dense"] = [float((got[0] - dense[0]).abs().max() / W), float((got[1] - dense[1]).abs().max() / W ** 2)]
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
    levels = np.quantile(q, [0.1, 0.5, 0.9])
    row = {"n": n, "m": m, "levels": len(levels), "dense_bytes_would_be": 8 * (-(-m // 128) * 128) ** 2}
    try:
        model.duration_curve(record_, levels=levels)
        row["dense"] = "completed"
    except (ValueError, RuntimeError) as e:
        row["dense"] = f"refused: {str(e)[:120]}"
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    dc = model.duration_curve(record_, levels=levels, streamed=True)
    torch.cuda.synchronize()
    row["streamed_wall_s"] = time.perf_counter() - t0
    row["peak_device_bytes"] = int(torch.cuda.max_memory_allocated())
    row["panel_rows"] = int(model._plan.exceedance_panel_rows(m, 1, len(levels)))
    row["fraction"] = [float(v) for v in dc["mean"].values]
    row["se"] = [float(v) for v in dc["se"].values]
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=14610)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--long", type=int, default=140000)
    ap.add_argument("--rows", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "exceedance_stream_time.py measures on the GPU"
    out = {"script": "exceedance_stream_time", "daily": daily_case(a.m, a.n, [int(r) for r in a.rows.split(",") if r])}
    if a.long > 0:
        out["long"] = long_case(a.long, 500)
    print(json.dumps(out))
