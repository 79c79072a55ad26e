#!/usr/bin/env python
"""Times ``dgp_predict_sensitivity`` -- the Jacobians of the posterior mean and variance with respect to every hyperparameter
direction -- at loadest d = 3 (P = 11 kernel directions, E = 1 diagonal direction, C = 1 right-hand side), HIP events around
whole ``GPPlan.predict_sensitivity`` calls in ONE chunk, after a warm-up, medians of the repetitions:

  * the whole call, and the means-only call (``return_var=False``: no quadratic forms, no beta^2 d sums); their difference is
    the quadratic-form pass, 2 P N^2 M flop, reported as a share and in TFLOP/s beside ``lauum_kernel``'s in-situ figure (N^3 / 3
    flop, the plan's own stage timing of a fit step) from the same process;
  * the alternative to the epilogue contraction, STORE-THEN-DOT: per direction the same product on the same direct-to-LDS core with
    its tile stored (``dgp_debug_tile_gemm``, N x N by N x M, operands of the same layouts) and the column dot with beta as a
    pass of its own -- P times -- on matrices of the call's shapes;
  * for comparison only, what the Jacobians replace: one ``factorize`` + ``predict`` at the same shape times 2 R, central
    differences over the R raw parameters.

    python scripts/sensitivity_bench.py --n 8192 --m 4096
    python scripts/sensitivity_bench.py --n 8192 --m 11323

One JSON line per run.  The quadratic-form pass is timed with E = 0 (no beta^2 d sums beside it)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

THETA = [0.9, 0.7, 1.0, 1.5, 0.6, 0.8, 1.2, 0.3, 0.9, 0.7, 1.1]  # loadest d = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtype", choices=("f64", "f32"), default="f64")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch

    from discontinuum_amd import _lib
    from discontinuum_amd.backend import GPPlan

    dev = torch.device("cuda:0")
    dtype = torch.float64 if args.dtype == "f64" else torch.float32
    d, n, m = 3, args.n, args.m
    rng = np.random.default_rng(0)

    def points(k):
        t = np.sort(rng.uniform(0.0, 10.0, k))
        return np.concatenate([t[:, None], rng.standard_normal((k, d - 1))], axis=1)

    X = torch.tensor(points(n), dtype=dtype, device=dev).contiguous()
    Xs = torch.tensor(points(m), dtype=dtype, device=dev).contiguous()
    r = torch.tensor(rng.standard_normal(n), dtype=dtype, device=dev)
    noise = torch.full((n,), 0.01, dtype=dtype, device=dev)
    diag = torch.ones(1, n, dtype=dtype, device=dev)
    rhs = torch.ones(1, n, dtype=dtype, device=dev)
    theta = torch.tensor(THETA, dtype=torch.float64)
    plan = GPPlan("loadest", n, d, dtype=dtype, device=dev)
    plan.set_inputs(X)
    plan.set_timing(True)
    out, _dr, _dn = plan.fit_step(theta, r, noise)
    assert int(out[_lib.OUT_INFO].item()) == 0, "factorisation failed"
    torch.cuda.synchronize(dev)
    lauum_ms = plan.get_timing()[_lib.TIME_LAUUM]
    plan.set_timing(False)
    chunk = -(-m // 128) * 128

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize(dev)
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = fn()
            e1.record()
            torch.cuda.synchronize(dev)
            times.append(e0.elapsed_time(e1))
        return statistics.median(times), min(times), max(times), res

    full = timed(lambda: plan.predict_sensitivity(theta, Xs, diag, rhs, chunk=chunk))
    # the quadratic-form pass alone: E = 0, so that the two calls differ by that launch (and P rows of the last pass)
    with_var = timed(lambda: plan.predict_sensitivity(theta, Xs, None, rhs, chunk=chunk))
    mean_only = timed(lambda: plan.predict_sensitivity(theta, Xs, None, rhs, chunk=chunk, return_var=False))

    # store-then-dot on the same core: W = D beta stored, then q = sum_i beta_ij W_ij, once per direction
    N, M = plan.N, chunk
    Dm = torch.randn(N, N, dtype=dtype, device=dev)
    Bm = torch.randn(N, M, dtype=dtype, device=dev)
    Wm = torch.empty(N, M, dtype=dtype, device=dev)
    code = _lib.F64 if dtype == torch.float64 else _lib.F32
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def store_then_dot():
        q = None
        for _p in range(plan.ntheta):
            rc = plan.lib.dgp_debug_tile_gemm(code, 1, 1, 0, ptr(Dm), N, ptr(Bm), M, N, ptr(Wm), M, N // 128, M // 128, 0, 0,
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0
            q = (Bm.double() * Wm.double()).sum(0) if dtype != torch.float64 else (Bm * Wm).sum(0)
        return q

    std = timed(store_then_dot)

    def refit():
        plan.factorize(theta, r, noise)
        return plan.predict(theta, Xs, chunk=chunk)

    fd = timed(refit)
    P = plan.ntheta
    quad_ms = with_var[0] - mean_only[0]
    R = 1 + P  # raw parameters of the loadest model: the mean constant and the kernel values
    try:
        clock_mhz = torch.cuda.clock_rate()
    except Exception:  # noqa: BLE001
        clock_mhz = None
    print(json.dumps({
        "model": "loadest", "d": d, "n": n, "m": m, "dtype": args.dtype, "P": P, "E": 1, "C": 1, "reps": args.reps,
        "sensitivity_ms_median": full[0], "sensitivity_ms_min": full[1], "sensitivity_ms_max": full[2],
        "means_only_ms_median": mean_only[0], "quadratic_pass_ms": quad_ms, "quadratic_pass_share": quad_ms / with_var[0],
        "store_then_dot_ms_median": std[0], "store_then_dot_ms_min": std[1], "store_then_dot_ms_max": std[2],
        "quadratic_pass_tflops": 2.0 * P * N * N * M / (quad_ms * 1e-3) / 1e12,
        "lauum_ms": lauum_ms, "lauum_tflops": N ** 3 / 3.0 / (lauum_ms * 1e-3) / 1e12,
        "factorize_predict_ms_median": fd[0], "central_differences_ms": 2 * R * fd[0], "raw_parameters": R,
        "max_abs_dmean": float(full[3][0].abs().max()), "max_abs_dvar": float(full[3][1].abs().max()),
        "sm_clock_mhz": clock_mhz, "device": torch.cuda.get_device_name(dev)}))


if __name__ == "__main__":
    main()
