"""The streamed value of additional samples against the dense path on the same fit, in one process.  (a) a rating-gp fit at
n = 300 over a stage record of m = 14 610 points in four years (P = 4, runoff-volume weights, the rule's K):
``posterior_cov`` + ``sample_value`` against ``posterior_sample_value`` with the panel the default budget picks and with 512-row
panels; (c) ``lowrank_period_moments`` at 12 and 64 rows against ``period_moments`` on the dense R = B^T B (formed outside the
timed region) -- HIP events around each call, every shape warmed first, the entries alternating, median of the repeats.  (b) one
15-minute stage record the dense path cannot hold (``--long`` points, rating-gp at n = 500, yearly groups):
``sample_value(streamed=True)`` and ``design(k = 12, streamed=True)`` as a whole, wall time and peak device bytes against
``max_bytes``.  Prints one JSON line.  ``--long 0`` skips the long record."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
os.environ["TQDM_DISABLE"] = "1"
from discontinuum_amd import design as dsn  # noqa: E402
from discontinuum_amd.backend import lowrank_period_moments, period_moments  # noqa: E402
from discontinuum_amd.loads import DEFAULT_MAX_BYTES  # noqa: E402
from discontinuum_amd.rating_gp import RatingGP  # noqa: E402
from discontinuum_amd.xr_compat import DataArray, Dataset  # noqa: E402
from scripts.excess_time import alternate  # noqa: E402


def stage_record(m, n, minutes, seed=0):
    rng = np.random.default_rng(seed)
    t = (np.datetime64("2015-01-01T00:00", "m") + minutes * np.arange(m)).astype("datetime64[ns]")
    stage_all = 1.0 + 3.0 * rng.beta(2, 5, m)
    pick = np.sort(rng.choice(m, n, replace=False))
    stage = stage_all[pick]
    q = np.exp(1.6 * np.log(stage) + 0.05 * rng.standard_normal(n))
    obs = Dataset({"stage": ("time", stage)}, coords={"time": t[pick]})
    target = DataArray(q, dims=("time",), coords={"time": t[pick]}, name="discharge", attrs={"units": "cfs"})
    unc = DataArray(np.full(n, 1.05), dims=("time",), coords={"time": t[pick]}, name="discharge_unc")
    model = RatingGP()
    model.fit(obs, target, target_unc=unc, iterations=3)
    return model, Dataset({"stage": ("time", stage_all)}, coords={"time": t}), np.full(m, 60.0 * minutes)


def short_case(m, n, reps):
    model, record, seconds = stage_record(m, n, 144)  # 144-minute steps: 14 610 points are four years
    fit = dsn._prepare(model, record, seconds, "YE", None, DEFAULT_MAX_BYTES)
    plan, theta, P, K = model._plan, model._factor_theta, fit.P, fit.nterms
    Xnew = torch.tensor(model.dm.Xnew(record), dtype=model.dtype)[torch.as_tensor(fit.order)].cuda().contiguous()
    M = fit.cov.shape[-1]
    picked = plan.sample_value_panel_rows(m, P, 64, K)
    row = {"n": n, "m": m, "M": M, "P": P, "nterms": K, "reps": reps, "default_panel_rows": picked}
    a, s2, g, ov, mapped, w = fit.a, fit.s2, fit.groups, fit.obs_var, fit.mapped, fit.w
    rows12 = dsn.conditioning_rows(fit, np.linspace(100, m - 100, 12).astype(np.int64))
    ref = plan.sample_value(fit.cov, m, a, s2, g, P, obs_var=ov, nterms=K)
    del fit
    torch.cuda.empty_cache()

    def dense(r=None):
        return plan.sample_value(plan.posterior_cov(theta, Xnew)[1], m, a, s2, g, P, obs_var=ov, rows=r, nterms=K)

    heights = sorted({picked, 512}, reverse=True)
    fns = [dense, lambda: plan.posterior_cov(theta, Xnew)]
    fns += [lambda R=R: plan.posterior_sample_value(theta, Xnew, a, s2, g, P, obs_var=ov, nterms=K, panel_rows=R) for R in heights]
    fns += [lambda: dense(rows12), lambda: plan.posterior_sample_value(theta, Xnew, a, s2, g, P, obs_var=ov, rows=rows12, nterms=K,
                                                                        panel_rows=picked)]
    ms, spread = alternate(fns, reps)
    row["dense_total_ms"], row["posterior_cov_ms"], row["spread_ms"] = ms[0], ms[1], spread
    for R, v in zip(heights, ms[2:]):
        got = plan.posterior_sample_value(theta, Xnew, a, s2, g, P, obs_var=ov, nterms=K, panel_rows=R)
        row[f"streamed_R{R}_ms"], row[f"streamed_R{R}_over_dense"] = v, v / ms[0]
        row[f"streamed_R{R}_vs_dense"] = float((got[0] - ref[0]).abs().max() / ref[0].abs().max())
    row["dense_rows12_ms"], row["streamed_rows12_ms"] = ms[-2], ms[-1]
    # (c) the value of a design from its rows against period_moments on the dense R
    shifted = mapped.double().contiguous()
    for nrows in (12, 64):
        B = (torch.randn(nrows, m, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(nrows))
             * (0.3 / np.sqrt(nrows) / np.sqrt(s2)))
        R = torch.zeros(M, M, dtype=torch.float64, device="cuda")
        R[:m, :m] = B.T @ B
        lms, _ = alternate([lambda: period_moments(R, m, shifted, s2, w, g, P, 1), lambda: lowrank_period_moments(B, m, shifted, s2, w, g, P, 1)],
                           reps)
        x, y = period_moments(R, m, shifted, s2, w, g, P, 1)[1], lowrank_period_moments(B, m, shifted, s2, w, g, P, 1)[1]
        row[f"period_moments_dense_R_nrows{nrows}_ms"], row[f"lowrank_nrows{nrows}_ms"] = lms
        row[f"lowrank_nrows{nrows}_vs_dense"] = float((x - y).abs().max() / x.abs().max())
        del R
    return row


def long_case(m, n):
    model, record, seconds = stage_record(m, n, 15)
    row = {"n": n, "m": m, "max_bytes": DEFAULT_MAX_BYTES, "dense_bytes_would_be": 8 * (-(-m // 128) * 128) ** 2}
    try:
        model.sample_value(record, seconds)
        row["dense"] = "completed"
    except ValueError as e:
        row["dense"] = f"refused: {str(e)[:160]}"
    for name, call in (("sample_value", lambda: model.sample_value(record, seconds, streamed=True)),
                       ("design_k12", lambda: model.design(record, seconds, 12, streamed=True))):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        ds = call()
        torch.cuda.synchronize()
        row[name] = {"wall_s": time.perf_counter() - t0, "peak_device_bytes": int(torch.cuda.max_memory_allocated()),
                     "nterms": int(ds.attrs["nterms"]), "periods": int(len(ds.coords["period"].values))}
        if name == "sample_value":
            row[name]["panel_rows"] = int(model._plan.sample_value_panel_rows(m, row[name]["periods"], 64, row[name]["nterms"]))
        else:
            row[name]["index"] = [int(i) for i in ds["index"].values]
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=14610)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--long", type=int, default=140000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "design_stream_time.py measures on the GPU"
    out = {"script": "design_stream_time"}
    if a.m > 0:
        out["short"] = short_case(a.m, a.n, a.reps)
    if a.long > 0:
        out["long"] = long_case(a.long, 500)
    print(json.dumps(out))
