"""``dgp_excess_moments`` beside ``dgp_exceedance_moments`` on the same posterior covariance: a daily record of 31 years
(m = 11 323 points, P = 31 yearly groups) of a loadest-gp fit at n = 300, at L = 1 and L = 8 threshold levels, excess and
deficit.  HIP events around each call, every shape warmed first, the two entries alternating, median of the repeats.  Four
orthant probabilities per pair and level in place of one make about 4x the expectation for the ratio.  One process; prints
one JSON line.  ``--m`` / ``--reps`` change the size and the repeats."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
os.environ["TQDM_DISABLE"] = "1"
from discontinuum_amd.exceedance import model_space_threshold  # noqa: E402
from discontinuum_amd.excess import log_threshold  # noqa: E402
from discontinuum_amd.loadest_gp import LoadestGP  # noqa: E402
from discontinuum_amd.loads import period_groups, target_transform  # noqa: E402
from scripts.exceedance_time import record  # noqa: E402


def alternate(fns, reps):
    """Median device milliseconds of each of ``fns``, warmed, called in turn ``reps`` times."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            out[k].append(start.elapsed_time(stop))
    return [float(np.median(o)) for o in out], [float(np.max(o) - np.min(o)) for o in out]


def main(m, n, reps):
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
    npairs = m * (m - 1) // 2
    row = {"script": "excess_time", "n": n, "m": m, "P": P, "pairs": npairs, "reps": reps}
    for L in (1, 8):
        lv = levels[4:5] if L == 1 else levels
        u = torch.tensor(np.broadcast_to(model_space_threshold(model.dm, lv)[:, None], (L, m)).copy(), device="cuda")
        a = torch.tensor(np.broadcast_to(log_threshold(lv)[:, None], (L, m)).copy(), device="cuda")
        (count, above, below), spread = alternate([
            lambda: plan.exceedance_moments(cov, m, mu, u, w, g, P),
            lambda: plan.excess_moments(cov, m, mapped, s * s, a, w, g, P, above=True),
            lambda: plan.excess_moments(cov, m, mapped, s * s, a, w, g, P, above=False)], reps)
        row[f"exceedance_moments_L{L}_ms"], row[f"excess_moments_L{L}_ms"], row[f"deficit_moments_L{L}_ms"] = count, above, below
        row[f"spread_L{L}_ms"] = spread
        row[f"ratio_L{L}"] = above / count
        row[f"orthants_per_s_L{L}"] = 4 * npairs * L / above * 1e3
    print(json.dumps(row))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=11323)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "excess_time.py measures on the GPU"
    main(a.m, a.n, a.reps)
