"""The windowing pass (``dgp_window_moments``, mode 0 and mode 1) beside the ``posterior_cov`` that feeds it, for a loadest
plan at n = 300, d = 3 in float64: m = 1096 (a three-year daily record) and m = 11 323 (the bench's inference size), trailing
windows of w = 30 and w = 365 points on every point (q = m).  Device events around the whole call (four launches); the bytes
the pass must move, M^2 esz + 2 * 8 M Q + 8 Q^2, over that time as a share of the 6.3 TB/s the memory system sustains.  The
split between the two passes comes from a ``rocprofv3 --kernel-trace --stats`` run of this script with ``--reps 3``.  One
process, one order; prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from discontinuum_amd.backend import MODE_LINEAR, MODE_LOG, GPPlan, window_moments  # noqa: E402
from oracle import gp_oracle as orc  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes per second


def device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        out.append(start.elapsed_time(stop))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1096,11323")
    ap.add_argument("--windows", default="30,365")
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "window_time.py measures on the GPU"
    dev, d, n = torch.device("cuda:0"), 3, a.n
    X, y = orc.synth_loadest(n, d, seed=0)
    X, y = torch.tensor(X), torch.tensor(y)
    theta = torch.full((orc.loadest_ntheta(d),), 0.6931471805599453, dtype=torch.float64)
    plan = GPPlan("loadest", n, d, dtype=torch.float64, device=dev)
    plan.set_inputs(X.to(dev).contiguous())
    plan.factorize(theta, (y - y.mean()).to(dev).contiguous(), torch.full((n,), 0.05, dtype=torch.float64, device=dev))
    rows = []
    for m in (int(v) for v in a.sizes.split(",")):
        g = torch.Generator().manual_seed(m)
        Xs = torch.rand(m, d, generator=g, dtype=torch.float64) * 4 - 2
        Xs[:, 0] = torch.sort(Xs[:, 0]).values
        Xs = Xs.to(dev).contiguous()
        row = {"n": n, "m": m}
        row["posterior_cov_ms"] = device_ms(lambda: plan.posterior_cov(theta, Xs), a.reps)
        mu, cov = plan.posterior_cov(theta, Xs)
        M = cov.shape[-1]
        i = np.arange(m)
        for w in (int(v) for v in a.windows.split(",")):
            lo, hi = torch.tensor(np.maximum(i + 1 - w, 0).astype(np.int32)), torch.tensor((i + 1).astype(np.int32))  # checked on the host
            Q = M
            nbytes = M * M * 8 + 2 * 8 * M * Q + 8 * Q * Q
            for mode, name in ((MODE_LINEAR, "linear"), (MODE_LOG, "log")):
                ms = device_ms(lambda: window_moments(cov, m, mu, lo, hi, mode=mode, scale2=0.7), a.reps)
                row[f"window_w{w}_{name}_ms"] = ms
                row[f"window_w{w}_{name}_share_of_6.3TBps"] = nbytes / (ms[0] * 1e-3) / HBM_ACHIEVABLE
            row[f"window_w{w}_bytes"] = nbytes
        rows.append(row)
        del cov
        torch.cuda.empty_cache()
    print(json.dumps({"script": "window_time", "times": "median, min, max ms over --reps", "device": torch.cuda.get_device_name(dev),
                      "sizes": rows}))


if __name__ == "__main__":
    main()
