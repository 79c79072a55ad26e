#!/usr/bin/env python
"""Measurements of the censored (Laplace) fit step for EXPERIMENTS.md, loadest d = 3, fp64, one GPU:

  * Newton iterations per training iteration over a short plan-level fit (Adam, lr 0.05, on softplus-constrained kernel
    hyperparameters and a constant mean; warm start from the previous mode) with a fraction of non-detects;
  * wall time per training iteration (host clock around work that ends in a device synchronise) against the uncensored
    ``fit_step`` on the same plan and the value-only ``factorize``;
  * the bilinear derivative sweep (``dgp_debug_bilinear``: two small copies, the pair sweep, its reduction) against the
    gradient contraction ``gram_grad`` (``dgp_stage_grad``), HIP events, median of ``--reps``.

    python scripts/censored_time.py --n 8192 --fractions 0.1 0.5 --iterations 50

One JSON line per fraction and one for the sweep."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.1, 0.5])
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch

    from discontinuum_amd import _lib
    from discontinuum_amd.backend import GPPlan

    dev = torch.device("cuda:0")
    n, d = args.n, args.d
    rng = np.random.default_rng(0)
    t = np.sort(rng.uniform(-16.0, 16.0, n))
    X = np.concatenate([t[:, None], rng.standard_normal((n, d - 1))], axis=1)
    truth = 0.15 * np.tanh(X[:, -1]) + 0.05 * np.sin(X[:, 0] / 4.0) + 0.1 * rng.standard_normal(n)
    plan = GPPlan("loadest", n, d, dtype=torch.float64, device=dev)
    plan.set_inputs(torch.tensor(X, device=dev).contiguous())
    nt = plan.ntheta
    noise = torch.full((n,), 0.01, dtype=torch.float64, device=dev)

    def clock():
        try:
            return torch.cuda.clock_rate()
        except Exception:  # noqa: BLE001
            return None

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize(dev)
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            out.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(out), min(out), max(out)

    theta0 = torch.full((nt,), 0.6931471805599453, dtype=torch.float64)
    r = torch.tensor(truth, device=dev)
    plain = timed(lambda: plan.fit_step(theta0, r, noise), args.reps)
    value = timed(lambda: plan.factorize(theta0, r, noise), args.reps)
    for frac in args.fractions:
        limit = float(np.quantile(truth, frac))  # one detection limit: everything below it is reported as "< limit"
        side = np.where(truth < limit, -1, 0).astype(np.int32)
        y = torch.tensor(np.where(side != 0, limit, truth), device=dev)
        sd = torch.tensor(side, device=dev)
        raw = torch.zeros(nt + 1, dtype=torch.float64, requires_grad=True)  # softplus(0) = ln 2; the last entry is the mean
        opt = torch.optim.Adam([raw], lr=0.05)
        f, newton, halvings, capped, ms, nll = None, [], [], [], [], []
        for _ in range(args.iterations):
            theta = torch.nn.functional.softplus(raw[:nt]).detach()
            mean = torch.full((n,), float(raw[nt].detach()), dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out, _dr, f, stat = plan.laplace_fit_step(theta, y, mean, noise, sd, f=f, maxit=50, tol=args.tol)
            host = out.cpu()
            ms.append(1e3 * (time.perf_counter() - t0))
            assert int(host[_lib.OUT_INFO]) == 0
            grad = torch.cat([host[_lib.OUT_DTHETA:_lib.OUT_DTHETA + nt] * torch.sigmoid(raw[:nt].detach()), -host[_lib.OUT_SUM_DR].reshape(1)])
            opt.zero_grad()
            raw.grad = grad / n
            opt.step()
            newton.append(stat[0])
            halvings.append(stat[2])
            capped.append(stat[3])
            nll.append(float(host[_lib.OUT_NLL]))
        print(json.dumps({"what": "fit", "n": n, "d": d, "non_detects": frac, "censored_rows": int((side != 0).sum()),
                          "newton_per_iteration": newton, "newton_mean_after_5": statistics.mean(newton[5:]) if len(newton) > 5 else None,
                          "halvings_total": sum(halvings), "capped_max": max(capped), "nll_first": nll[0], "nll_last": nll[-1],
                          "ms_per_iteration_median": statistics.median(ms), "ms_per_iteration_median_after_5": statistics.median(ms[5:]) if len(ms) > 5 else None,
                          "ms_first": ms[0], "ms_plain_fit_step_median_min_max": plain, "ms_factorize_median_min_max": value,
                          "sm_clock_mhz": clock(), "device": torch.cuda.get_device_name(dev)}))
    # the bilinear sweep against gram_grad: both read the plan left by a fit step
    plan.fit_step(theta0, r, noise)
    u = torch.tensor(rng.standard_normal(n), device=dev)
    a = torch.tensor(rng.standard_normal(n), device=dev)

    def events(fn):
        fn()
        torch.cuda.synchronize(dev)
        out = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize(dev)
            out.append(e0.elapsed_time(e1))
        return statistics.median(out), min(out), max(out)

    print(json.dumps({"what": "sweep", "n": n, "d": d, "ms_bilinear_median_min_max": events(lambda: plan.bilinear(theta0, u, a)),
                      "ms_gram_grad_median_min_max": events(lambda: plan.stage_grad(theta0)), "sm_clock_mhz": clock()}))


if __name__ == "__main__":
    main()
