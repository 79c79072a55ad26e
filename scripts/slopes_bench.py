#!/usr/bin/env python
"""Times ``dgp_predict_slopes`` (value and input derivatives, P = 1 + ncols planes) against ``dgp_predict_terms`` (C additive
parts) at the same n, m and plane count -- loadest d = 3: P = 3 (two requested columns) against C = 3.  Both run the same GEMM
width and the same reduction; the difference is the pair evaluator.  HIP events around whole ``GPPlan.predict_slopes`` /
``GPPlan.predict_terms`` calls, after a warm-up.

    python scripts/slopes_bench.py --mode slopes --n 8192 --m 8192
    python scripts/slopes_bench.py --mode terms  --n 8192 --m 8192

One JSON line per run; run the two modes in alternating processes and take the spread from the repetitions.  The per-kernel
split comes from a kernel trace of one process per mode, in a run of its own (EXPERIMENTS.md)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

THETA = [0.9, 0.7, 1.0, 1.5, 0.6, 0.8, 1.2, 0.3, 0.9, 0.7, 1.1]  # loadest d = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("slopes", "terms"), required=True)
    ap.add_argument("--cols", default="0,1", help="requested columns of the slopes mode (two of them: P = 3 = loadest's C)")
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=8192)
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
    d = 3
    rng = np.random.default_rng(0)

    def points(k):
        t = np.sort(rng.uniform(0.0, 10.0, k))
        return np.concatenate([t[:, None], rng.standard_normal((k, d - 1))], axis=1)

    X = torch.tensor(points(args.n), dtype=dtype, device=dev).contiguous()
    Xs = torch.tensor(points(args.m), dtype=dtype, device=dev).contiguous()
    r = torch.tensor(rng.standard_normal(args.n), dtype=dtype, device=dev)
    noise = torch.full((args.n,), 0.01, dtype=dtype, device=dev)
    theta = torch.tensor(THETA, dtype=torch.float64)
    plan = GPPlan("loadest", args.n, d, dtype=dtype, device=dev)
    plan.set_inputs(X)
    out = plan.factorize(theta, r, noise)
    assert int(out[3].item()) == 0, "factorisation failed"
    cols = [int(c) for c in args.cols.split(",")]

    def once():
        if args.mode == "slopes":
            return plan.predict_slopes(theta, Xs, cols)
        return plan.predict_terms(theta, Xs)

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
    planes = int(res[0].shape[0])
    check = float(res[0].abs().max())
    try:
        clock_mhz = torch.cuda.clock_rate()
    except Exception:  # noqa: BLE001
        clock_mhz = None
    print(json.dumps({"mode": args.mode, "model": "loadest", "n": args.n, "m": args.m, "dtype": args.dtype, "planes": planes,
                      "ms_median": statistics.median(times), "ms_min": min(times), "ms_max": max(times), "reps": args.reps,
                      "max_abs_mean": check, "sm_clock_mhz": clock_mhz, "device": torch.cuda.get_device_name(dev)}))


if __name__ == "__main__":
    main()
