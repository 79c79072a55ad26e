"""Device time of the leave-one-out fit step (``dgp_loo_fit_step``) beside the marginal-likelihood fit step (``dgp_fit_step``) on the
same plan, in one process: loadest d = 3, fp64, one site at n = 300, 2048, 8192 and a batch of 32 sites at n = 8192 (``--cases``
selects).  HIP events after a warm-up call, median of the repetitions.  ``extra_ms`` = loo - fit is everything the objective adds
(mirror pass, the symmetric product 2 M = F G^T, b = S c, two contractions, the row passes); ``extra_TFLOPs`` counts only the
product's B N^2 (N + 128) flop (lower 128-tiles, full k-range) over ALL of that time, so it is a lower bound of the product
kernel's rate; ``lauum_TFLOPs`` is B N^3 / 3 over the fit step's own HIP-event time of K^^-1 = L^-T L^-1 (``dgp_plan_get_timing``).
Prints one JSON line per case."""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, ".."), HERE]
from discontinuum_amd import _lib  # noqa: E402
from discontinuum_amd.backend import GPPlan  # noqa: E402
from flux_time import device_ms  # noqa: E402
from oracle import gp_oracle as orc  # noqa: E402

CASES = {"300": (300, 1), "2048": (2048, 1), "8192": (8192, 1), "32x8192": (8192, 32)}


def case(n, batch, dev):
    d = 3
    X, y = orc.synth_loadest(n, d, seed=0)
    theta = torch.tensor([0.9, 0.7, 1.0, 1.5, 0.6, 0.8, 1.2, 0.3, 0.9, 0.7, 1.1], dtype=torch.float64)
    noise = torch.full((n,), 0.01, dtype=torch.float64)
    X, y = torch.tensor(X), torch.tensor(y)
    lead = (batch,) if batch > 1 else ()
    rep = lambda t: t.to(dev).expand(lead + tuple(t.shape)).contiguous()  # noqa: E731
    p = GPPlan("loadest", n, d, device=dev, lookahead=1 if batch > 1 else True, batch=batch)
    p.set_inputs(rep(X))
    th = theta.expand(lead + (theta.numel(),)).contiguous()
    yd, nd = rep(y), rep(noise)
    out = p.loo_fit_step(th, yd, nd)[0]
    assert bool((out[..., _lib.OUT_INFO] == 0).all()) and bool(torch.isfinite(out[..., _lib.OUT_NLL]).all())
    reps = 3 if n >= 4096 else 10
    fit_ms = device_ms(lambda: p.fit_step(th, yd, nd), reps)
    loo_ms = device_ms(lambda: p.loo_fit_step(th, yd, nd), reps)
    value_ms = device_ms(lambda: p.loo_value(), reps)
    p.set_timing(True)
    p.fit_step(th, yd, nd)
    torch.cuda.synchronize()
    lauum_ms = p.get_timing()[_lib.TIME_LAUUM]
    p.set_timing(False)
    N = float(p.N)
    prod_flop = batch * N * N * (N + 128.0)
    return {"script": "loo_bench", "model": "loadest", "n": n, "N": p.N, "batch": batch, "dtype": "float64", "fit_step_ms": fit_ms,
            "loo_fit_step_ms": loo_ms, "ratio": loo_ms / fit_ms, "extra_ms": loo_ms - fit_ms, "loo_value_ms": value_ms,
            "product_flop": prod_flop, "extra_TFLOPs": prod_flop / max(loo_ms - fit_ms, 1e-9) / 1e9, "lauum_ms": lauum_ms,
            "lauum_TFLOPs": batch * N ** 3 / 3.0 / max(lauum_ms, 1e-9) / 1e9,
            "work_bytes": int(p.lib.dgp_loo_workspace_bytes(p._h))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="300,2048,8192,32x8192")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loo_bench.py measures on the GPU"
    dev = torch.device("cuda:0")
    for key in args.cases.split(","):
        n, batch = CASES[key]
        print(json.dumps(case(n, batch, dev)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
