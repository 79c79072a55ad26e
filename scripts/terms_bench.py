#!/usr/bin/env python
"""Times ``dgp_predict_terms`` (all additive parts of the covariance and their cross-covariances in one pass) against what
the ABI offered before it: C calls of ``dgp_predict`` with the other parts' outputscales zeroed (C pair evaluations per matrix
entry, no cross-covariances).  HIP events around whole ``GPPlan.predict_terms`` / ``GPPlan.predict`` calls, after a warm-up.

    python scripts/terms_bench.py --mode terms    --model loadest --n 8192 --m 11323
    python scripts/terms_bench.py --mode baseline --model loadest --n 8192 --m 11323 --root /path/to/another/checkout

``--root``: the checkout whose ``discontinuum_amd`` (and built ``libdgp_hip.so``) is imported -- the baseline only needs
``GPPlan.predict``, so it runs from a build of the commit before this entry point existed.  One JSON line per run; run the two
modes in alternating processes and take the spread from the repetitions (EXPERIMENTS.md)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

OUTPUTSCALES = {"loadest": lambda d: (0, 4, 4 + d), "rating": lambda d: (1, 4, 7, 10, 12)}
THETA = {
    "loadest": [0.9, 0.7, 1.0, 1.5, 0.6, 0.8, 1.2, 0.3, 0.9, 0.7, 1.1],
    "rating": [2.0, 0.5, 0.8, 1.5, 0.3, 1.2, 0.7, 0.6, 0.9, 1.4, 1.0, 1.1, 0.4, 0.8, 1.0, 1.3],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("terms", "baseline"), required=True)
    ap.add_argument("--model", choices=("loadest", "rating"), default="loadest")
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=11323)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtype", choices=("f64", "f32"), default="f64")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch

    from discontinuum_amd.backend import GPPlan

    dev = torch.device("cuda:0")
    dtype = torch.float64 if args.dtype == "f64" else torch.float32
    d = 3 if args.model == "loadest" else 2
    rng = np.random.default_rng(0)

    def points(k):
        t = np.sort(rng.uniform(0.0, 10.0, k))
        if args.model == "rating":
            return np.stack([t, 1.0 + 3.0 * rng.beta(2, 5, k)], axis=1)
        return np.concatenate([t[:, None], rng.standard_normal((k, d - 1))], axis=1)

    X = torch.tensor(points(args.n), dtype=dtype, device=dev).contiguous()
    Xs = torch.tensor(points(args.m), dtype=dtype, device=dev).contiguous()
    r = torch.tensor(rng.standard_normal(args.n), dtype=dtype, device=dev)
    noise = torch.full((args.n,), 0.01, dtype=dtype, device=dev)
    theta = torch.tensor(THETA[args.model], dtype=torch.float64)
    plan = GPPlan(args.model, args.n, d, dtype=dtype, device=dev)
    plan.set_inputs(X)
    out = plan.factorize(theta, r, noise)
    assert int(out[3].item()) == 0, "factorisation failed"
    os_idx = OUTPUTSCALES[args.model](d)
    thetas = []
    for c in range(len(os_idx)):
        th = theta.clone()
        for k, i in enumerate(os_idx):
            if k != c:
                th[i] = 0.0
        thetas.append(th)

    def once():
        if args.mode == "terms":
            return plan.predict_terms(theta, Xs)
        return [plan.predict(th, Xs) for th in thetas]

    for _ in range(args.warmup):
        once()
    torch.cuda.synchronize(dev)
    times = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = once()
        e1.record()
        torch.cuda.synchronize(dev)
        times.append(e0.elapsed_time(e1))
    if args.mode == "terms":
        check = float(res[0].sum(0).abs().max())
    else:
        check = float(sum(mu for mu, _ in res).abs().max())
    try:
        clock_mhz = torch.cuda.clock_rate()
    except Exception:  # noqa: BLE001
        clock_mhz = None
    print(json.dumps({"mode": args.mode, "model": args.model, "n": args.n, "m": args.m, "dtype": args.dtype, "parts": len(os_idx),
                      "ms_median": statistics.median(times), "ms_min": min(times), "ms_max": max(times), "reps": args.reps,
                      "max_abs_total_mean": check, "sm_clock_mhz": clock_mhz, "device": torch.cuda.get_device_name(dev)}))


if __name__ == "__main__":
    main()
