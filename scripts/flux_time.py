"""Annual loads at the reference workflow's size (a daily grid over a 31-year record: m = 11 323 points, P = 31 years),
for a loadest-gp fit at n = 300 (the reference's record size) and at n = 8192 (the bench's inference factorisation):
the exact path (``dgp_posterior_cov`` + ``dgp_period_moments``, and ``LoadestGP.annual_flux`` as a whole) against the
Monte Carlo path of the reference (``sample(1000)`` + ``concentration_to_flux`` + annual sums).  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
os.environ["TQDM_DISABLE"] = "1"
from discontinuum_amd.backend import MODE_LOG  # noqa: E402
from discontinuum_amd.loadest_gp import LoadestGP, concentration_to_flux  # noqa: E402
from discontinuum_amd.loads import period_groups, target_transform  # noqa: E402
from discontinuum_amd.xr_compat import DataArray, Dataset  # noqa: E402

M_DAYS, START = 11323, "1990-01-01"


def record(n, seed=0):
    rng = np.random.default_rng(seed)
    t = (np.datetime64(START, "D") + np.arange(M_DAYS)).astype("datetime64[ns]")
    season = np.sin(2 * np.pi * np.arange(M_DAYS) / 365.25)
    flow = np.exp(1.0 + 0.6 * season + 0.4 * rng.standard_normal(M_DAYS)) * 10
    pick = np.sort(rng.choice(M_DAYS, n, replace=False))
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


def one_fit(n):
    obs, target, daily = record(n)
    model = LoadestGP()
    model.fit(obs, target, iterations=3)
    flow = np.asarray(daily["flow"].values)
    order, groups, labels, _n, _d = period_groups(daily.coords["time"].values, flow, "YE")
    P = len(labels)
    assert P == 31 and np.array_equal(order, np.arange(M_DAYS))
    _mode, s, t = target_transform(model.dm)
    Xnew = torch.tensor(model.dm.Xnew(daily), dtype=model.dtype).cuda().contiguous()
    model._ensure_factor()
    theta = model._factor_theta
    plan = model._plan
    w = torch.tensor(flow * 86400 * 1e-3, device="cuda")
    g = torch.tensor(groups, device="cuda")
    kmean, cov = plan.posterior_cov(theta, Xnew)
    mu = (s * (kmean + model.model.prior_mean(Xnew)) + t).contiguous()
    row = {"n": n, "m": M_DAYS, "P": P}
    row["posterior_cov_ms"] = device_ms(lambda: plan.posterior_cov(theta, Xnew), 5)
    row["period_moments_ms"] = device_ms(lambda: plan.period_moments(cov, M_DAYS, mu, s * s, w, g, P, MODE_LOG), 10)
    nbytes = M_DAYS * M_DAYS * cov.element_size()  # every (i, j) read once: each off-diagonal element of the triangle twice
    row["period_moments_bytes"] = nbytes
    row["period_moments_GBps"] = nbytes / row["period_moments_ms"] / 1e6
    del cov
    torch.cuda.empty_cache()
    row["annual_flux_ms"] = wall(lambda: model.annual_flux(daily), 3)
    onehot = np.zeros((M_DAYS, P))
    onehot[np.arange(M_DAYS), groups] = 1.0

    def monte_carlo():
        sim = model.sample(daily, n=1000)
        flux = concentration_to_flux(sim, daily["flow"])
        return flux.values @ onehot

    row["sample1000_flux_annual_ms"] = wall(monte_carlo, 3)
    exact = model.annual_flux(daily)
    mc = monte_carlo()
    row["mc_vs_exact_mean_max_rel"] = float(np.max(np.abs(mc.mean(0) / exact["mean"].values - 1)))
    row["speedup_vs_sample1000"] = row["sample1000_flux_annual_ms"] / row["annual_flux_ms"]
    return row


if __name__ == "__main__":
    assert torch.cuda.is_available(), "flux_time.py measures on the GPU"
    rows = [one_fit(n) for n in (300, 8192)]
    print(json.dumps({"script": "flux_time", "fits": rows}))
