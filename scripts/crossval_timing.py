"""Times of exact cross-validation (``dgp_cross_validate``) against one ``factorize`` on the same plan, in one process.

    python scripts/crossval_timing.py [--n 8192 300] [--reps 25] [--dtype f64]

Per size (loadest, d = 3): leave-one-out, 16 contiguous blocks and 5 random folds, each after a bare ``factorize`` (the
packed-panel route) and after a ``fit_step`` (the gather of K^^-1), and one ``factorize`` -- the cost of ONE refitted fold,
the yardstick: refitting k folds costs k of them.  Every figure is the median of ``--reps`` HIP-event timings after three
warm-up calls; the leave-one-out pass also reports its bytes/s against the lower triangle of T.  The chip's shader clock
during the run comes from ``dgp_debug_clock_probe``.  One JSON line per size.
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from discontinuum_amd import _lib  # noqa: E402
from discontinuum_amd.backend import GPPlan  # noqa: E402
from oracle import gp_oracle as orc  # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def clock_mhz(lib, load, load_s, seconds=0.2):
    """Shader clock while `load` runs back to back (bench.py::clock_probe): d s_memtime / d s_memrealtime x 100 MHz."""
    out = torch.zeros(2 * 16, dtype=torch.int64, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    load()
    if lib.dgp_debug_clock_probe(C.c_void_p(out.data_ptr()), 16, float(seconds), s) != 0:
        return None
    for _ in range(max(2, int(math.ceil(1.3 * seconds / max(load_s, 1e-4))))):
        load()
    torch.cuda.synchronize()
    o = out.cpu().numpy().reshape(-1, 2).astype(np.float64)
    ok = o[:, 1] > 0
    return float(np.median(o[ok, 0] / o[ok, 1]) * 100.0) if ok.any() else None


def run(n, reps, dtype):
    d = 3
    X, y = orc.synth_loadest(n, d, seed=0)
    Xd = torch.tensor(X, device="cuda", dtype=dtype).contiguous()
    yd = torch.tensor(y, device="cuda", dtype=dtype).contiguous()
    noise = torch.full((n,), 0.01, dtype=dtype, device="cuda")
    theta = torch.tensor([0.9, 0.7, 1.0, 1.5, 0.6, 0.8, 1.2, 0.3, 0.9, 0.7, 1.1], dtype=torch.float64)
    p = GPPlan("loadest", n, d, dtype=dtype, device="cuda")
    p.set_inputs(Xd)
    schemes = {"loo": np.arange(n), "16-block": np.arange(n) * 16 // n, "5-fold": np.random.default_rng(0).permutation(n) % 5}
    row = {"n": n, "d": d, "dtype": str(dtype).replace("torch.", ""), "reps": reps}
    med, lo, hi = timed(lambda: p.factorize(theta, yd, noise), reps)
    row["factorize_ms"] = {"median": med, "min": lo, "max": hi}
    for state in ("factorize", "fit_step"):
        (p.factorize if state == "factorize" else p.fit_step)(theta, yd, noise)
        for name, groups in schemes.items():
            g = torch.as_tensor(groups)
            med, lo, hi = timed(lambda: p.cross_validate(g), reps)  # (includes the host-side sort of the fold ids)
            row[f"{name}_after_{state}_ms"] = {"median": med, "min": lo, "max": hi}
    esz = 8 if dtype == torch.float64 else 4
    tri_bytes = esz * p.N * (p.N + 1) / 2
    row["loo_bytes_per_s_vs_lower_T"] = tri_bytes / (row["loo_after_factorize_ms"]["median"] * 1e-3)
    row["cv16_over_factorize"] = row["16-block_after_factorize_ms"]["median"] / row["factorize_ms"]["median"]
    row["clock_mhz"] = clock_mhz(p.lib, lambda: p.factorize(theta, yd, noise), row["factorize_ms"]["median"] * 1e-3)
    print(json.dumps(row))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[8192, 300])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    a = ap.parse_args()
    for n in a.n:
        run(n, max(20, a.reps), torch.float64 if a.dtype == "f64" else torch.float32)
