"""Device time of the influence of the held samples on the period sums (``dgp_deletion_influence``): fp64 loadest d = 3,
n = 8192, m = 4096 and m = 11 323 test points in 32 periods.  Leave-one-out (8192 folds) and one fold per year of sampling (32
folds of about 256: the block route), in both modes, beside a means-only ``predict_sensitivity`` (E = C = 0,
``return_var=False``) on the same inputs in the same process -- it runs the same K*, V = T K*, beta = T^T V products -- and
beside n x (one ``factorize`` + one ``predict``), the refits the call replaces (one refit is measured, not n).  HIP events
after a warm-up call, median of the repetitions; the reduce pass alone and the products before it from torch's profiler in the
same process (``kernel_ms``).  Prints one JSON line per m.

``--kernels``: no timing, three calls per variant only -- the run to put under ``rocprofv3 --kernel-trace --stats`` for the
time of the sweep kernels alone (inf_sweep_kernel, inf_finish_kernel)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, ".."), HERE]
from discontinuum_amd.backend import MODE_LINEAR, MODE_LOG, GPPlan  # noqa: E402
from flux_time import device_ms  # noqa: E402
from oracle import gp_oracle as orc  # noqa: E402

N_OBS, D, SCALE = 8192, 3, 0.7


def kernel_ms(fn, tag, reps=3):
    """Device time per call of the kernels of one variant, by torch's profiler in this process: the reduce pass alone
    (inf_sweep_kernel + inf_finish_kernel) and the three products before it (gram_cross, predict_v, sens_beta).  Null when the
    profiler records no device activity on the box."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        rows = [(e.key, getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)) for e in prof.key_averages()]
    except Exception:  # noqa: BLE001
        rows = []

    def total(*names):
        hit = [t for k, t in rows if any(nm in k for nm in names)]
        return sum(hit) / reps / 1e3 if hit else None

    return {f"{tag}_reduce_pass_ms": total("inf_sweep_kernel", "inf_finish_kernel"),
            f"{tag}_products_ms": total("gram_cross_kernel", "predict_v_kernel", "sens_beta")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--n", type=int, default=N_OBS)
    ap.add_argument("--m", type=int, nargs="*", default=[4096, 11323])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "influence_time.py measures on the GPU"
    dev, n = torch.device("cuda:0"), args.n
    X, y = orc.synth_loadest(n, D, seed=0)
    theta = torch.tensor([0.9, 0.7, 1.0, 1.5, 0.6, 0.8, 1.2, 0.3, 0.9, 0.7, 1.1], dtype=torch.float64)
    noise = torch.full((n,), 0.01, dtype=torch.float64, device=dev)
    Xd, yd = torch.tensor(X).to(dev).contiguous(), torch.tensor(y).to(dev).contiguous()
    p = GPPlan("loadest", n, D, device=dev)
    p.set_inputs(Xd)
    assert int(p.factorize(theta, yd, noise)[3]) == 0
    years = np.floor(X[:, 0]).astype(np.int64)
    folds = {"loo": torch.arange(n), "year": torch.as_tensor(years - years.min())}
    for m in args.m:
        Xs = np.asarray(orc.synth_loadest(m, D, seed=1)[0])
        Xs = Xs[np.argsort(Xs[:, 0], kind="stable")]
        per = np.floor(Xs[:, 0]).astype(np.int32)
        per -= per.min()
        P = int(per.max()) + 1
        xs = torch.tensor(Xs).to(dev).contiguous()
        mu, var = p.predict(theta, xs)
        a = {MODE_LOG: torch.exp(SCALE * mu + 0.5 * SCALE * SCALE * var), MODE_LINEAR: torch.full_like(mu, SCALE)}
        isd = torch.rsqrt(var.clamp(min=1e-300))
        calls = {f"{name}_{'log' if mode == MODE_LOG else 'linear'}": (lambda ids=ids, mode=mode: p.deletion_influence(
            theta, xs, ids, a[mode], SCALE, per, P, mode, inv_sd=isd)) for name, ids in folds.items() for mode in (MODE_LOG, MODE_LINEAR)}
        calls["sensitivity_means_only"] = lambda: p.predict_sensitivity(theta, xs, return_var=False, chunk=1 << 20)
        if args.kernels:
            for fn in calls.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize(dev)
            continue
        out = {"script": "influence_time", "n": n, "N": p.N, "m": m, "periods": P, "dtype": "float64",
               "year_folds": int(folds["year"].max()) + 1, "largest_year_fold": int(np.bincount(years - years.min()).max())}
        for name, fn in calls.items():
            out[f"{name}_ms"] = device_ms(fn, 5)
        refit = device_ms(lambda: (p.factorize(theta, yd, noise), p.predict(theta, xs)), 3)
        out.update(one_refit_ms=refit, n_refits_s=refit * n / 1e3, loo_log_speedup_over_refits=refit * n / out["loo_log_ms"],
                   work_bytes_loo=int(p.lib.dgp_deletion_influence_workspace_bytes(p._h, m, n, 1, P)),
                   work_bytes_year=int(p.lib.dgp_deletion_influence_workspace_bytes(p._h, m, out["year_folds"], out["largest_year_fold"], P)))
        out.update(kernel_ms(calls["loo_log"], "loo_log"))
        out.update(kernel_ms(calls["year_log"], "year_log"))
        info = calls["year_log"]()[3]
        out["info_nonzero"] = int((info != 0).sum())
        try:
            out["sm_clock_mhz"] = torch.cuda.clock_rate()
        except Exception:  # noqa: BLE001  (no SMI library on the box)
            out["sm_clock_mhz"] = None
        print(json.dumps(out), flush=True)
        p._influence_ws = p._sens_ws = None
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
