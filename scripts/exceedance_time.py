"""Exceedance days per year on a daily record of 10 and of 40 years (m = 3653 and m = 14 610 points, P = 10 / 40 years)
for a loadest-gp fit at n = 300: ``dgp_exceedance_moments`` alone at L = 1 and L = 16 levels, ``LoadestGP.exceedance`` as a
whole, and the sampling route that answers the same question without it -- ``sample(1000)``, compare every draw with the
threshold, count per year.  One process, one order; prints one JSON line.  ``--sizes 3653`` restricts the sizes (for a
profiler run), ``--kernel-only`` skips the model-level timings."""
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
from discontinuum_amd.xr_compat import DataArray, Dataset  # noqa: E402

START = "1980-01-01"
PEAK_FP64_VECTOR_FMA = 78.6e12 / 2  # lane-FMAs per second


def record(n, m, seed=0):
    rng = np.random.default_rng(seed)
    t = (np.datetime64(START, "D") + np.arange(m)).astype("datetime64[ns]")
    season = np.sin(2 * np.pi * np.arange(m) / 365.25)
    flow = np.exp(1.0 + 0.6 * season + 0.4 * rng.standard_normal(m)) * 10
    pick = np.sort(rng.choice(m, n, replace=False))
    conc = np.exp(0.3 * np.log(flow[pick]) + 0.2 * rng.standard_normal(n))
    units = {"units": "cubic meters per second"}
    obs = Dataset({"flow": ("time", flow[pick], units)}, coords={"time": t[pick]})
    target = DataArray(conc, dims=("time",), coords={"time": t[pick]}, name="concentration", attrs={"units": "mg/l"})
    daily = Dataset({"flow": ("time", flow, units)}, coords={"time": t})
    return obs, target, daily


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def device_ms(fn, reps):
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


def one_size(m, n, kernel_only):
    obs, target, daily = record(n, m)
    model = LoadestGP()
    model.fit(obs, target, iterations=3)
    time_ = daily.coords["time"].values
    order, groups, labels, _n, _d = period_groups(time_, np.ones(m), "YE")
    P = len(labels)
    assert np.array_equal(order, np.arange(m))
    Xnew = torch.tensor(model.dm.Xnew(daily), dtype=model.dtype).cuda().contiguous()
    model._ensure_factor()
    theta, plan = model._factor_theta, model._plan
    kmean, cov = plan.posterior_cov(theta, Xnew)
    mu = (kmean + model.model.prior_mean(Xnew)).detach().contiguous()
    conc_mean = np.asarray(model.dm.y_t(mu.cpu().numpy()).values).reshape(-1)
    levels = np.quantile(conc_mean, np.linspace(0.2, 0.8, 16))
    w = torch.ones(m, dtype=torch.float64, device="cuda")
    g = torch.tensor(groups, device="cuda")
    sd = torch.diagonal(cov)[:m].double().clamp_min(1e-300).sqrt()
    low = torch.tril(cov[:m, :m].double(), -1) / (sd[:, None] * sd[None, :])
    npairs = m * (m - 1) // 2
    row = {"n": n, "m": m, "P": P, "pairs": npairs,
           "rho_share_above_0.925": float((low.abs() >= 0.925).sum()) / npairs,
           "rho_share_below_0.3": (float((low.abs() < 0.3).sum()) - (m * m - npairs)) / npairs}
    del low
    for L in (1, 16):
        u = torch.tensor(np.broadcast_to(model_space_threshold(model.dm, levels[8:9] if L == 1 else levels)[:, None], (L, m)).copy(),
                         device="cuda")
        ms = device_ms(lambda: plan.exceedance_moments(cov, m, mu, u, w, g, P), 5)
        row[f"exceedance_moments_L{L}_ms"] = ms
        row[f"pair_levels_per_s_L{L}"] = npairs * L / ms * 1e3
    row["posterior_cov_ms"] = device_ms(lambda: plan.posterior_cov(theta, Xnew), 3)
    del cov
    torch.cuda.empty_cache()
    if kernel_only:
        return row
    tau = float(levels[8])
    for L in (1, 16):
        thr = tau if L == 1 else levels
        row[f"exceedance_L{L}_ms"] = wall(lambda: model.exceedance(daily, threshold=thr), 3)
    onehot = np.zeros((m, P))
    onehot[np.arange(m), groups] = 1.0

    def monte_carlo():
        sim = model.sample(daily, n=1000)
        return (np.asarray(sim.values) > tau).astype(np.float64) @ onehot

    row["sample1000_count_ms"] = wall(monte_carlo, 3)
    exact = model.exceedance(daily, threshold=tau)
    mc = monte_carlo()
    se_mc = mc.std(axis=0, ddof=1) / np.sqrt(mc.shape[0])
    row["mc_vs_exact_mean_max_z"] = float(np.max(np.abs(mc.mean(0) - exact["mean"].values[0]) / np.where(se_mc > 0, se_mc, np.inf)))
    row["mc_vs_exact_se_max_rel"] = float(np.max(np.abs(mc.std(axis=0, ddof=1) / np.where(exact["se"].values[0] > 0, exact["se"].values[0], np.nan) - 1)))
    row["speedup_vs_sample1000"] = row["sample1000_count_ms"] / row["exceedance_L1_ms"]
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3653,14610")
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "exceedance_time.py measures on the GPU"
    rows = [one_size(int(m), a.n, a.kernel_only) for m in a.sizes.split(",")]
    print(json.dumps({"script": "exceedance_time", "peak_fp64_vector_lane_fma_per_s": PEAK_FP64_VECTOR_FMA, "sizes": rows}))
