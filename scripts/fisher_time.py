"""Device time of the Fisher information of the hyperparameters (``dgp_fisher``, independent of any prediction grid) beside
one fit step on the same plan: loadest d = 3 (P = 11 kernel directions) and rating (P = 16, plus the learned noise's diagonal
direction), fp64, single plans at n = 300, 4096, 8192 and a batch of 32 sites at n = 300.  HIP events after a warm-up call,
median of the repetitions; the rate is (P + E) (4/3) N^3 flop (2/3 N^3 for a diagonal direction) over that time.  Prints one
JSON line per case."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, ".."), HERE]
from discontinuum_amd.backend import GPPlan  # noqa: E402
from flux_time import device_ms  # noqa: E402
from oracle import gp_oracle as orc  # noqa: E402

CASES = [("loadest", 3, 300, 1), ("loadest", 3, 4096, 1), ("loadest", 3, 8192, 1), ("loadest", 3, 300, 32),
         ("rating", 2, 300, 1), ("rating", 2, 4096, 1), ("rating", 2, 8192, 1), ("rating", 2, 300, 32)]


def case(model, d, n, batch, dev):
    if model == "loadest":
        X, y = orc.synth_loadest(n, d, seed=0)
        theta = torch.tensor([0.9, 0.7, 1.0, 1.5, 0.6, 0.8, 1.2, 0.3, 0.9, 0.7, 1.1], dtype=torch.float64)
        noise = torch.full((n,), 0.01, dtype=torch.float64)
        diag = None
    else:
        X, y, yu = orc.synth_rating(n, seed=0)
        o = orc.RatingOracle.from_stage(X[:, 1])
        raw = torch.zeros(20, dtype=torch.float64)
        raw[1], raw[2], raw[3] = 1.6, 0.5, -5.0
        theta = o.constrained(raw)
        noise = o.noise(raw, n, torch.tensor(yu))
        diag = torch.ones(1, n, dtype=torch.float64)
    X, y = torch.tensor(X), torch.tensor(y)
    lead = (batch,) if batch > 1 else ()
    rep = lambda t: t.to(dev).expand(lead + tuple(t.shape)).contiguous()  # noqa: E731
    p = GPPlan(model, n, d, device=dev, lookahead=1 if batch > 1 else True, batch=batch)
    p.set_inputs(rep(X))
    th = theta.expand(lead + (theta.numel(),)).contiguous()
    yd, nd, dg = rep(y), rep(noise), None if diag is None else rep(diag)
    out = p.fit_step(th, yd, nd)[0]
    assert bool((out[..., 3] == 0).all())
    reps = 3 if n >= 4096 else 10
    fit_ms = device_ms(lambda: p.fit_step(th, yd, nd), reps)
    fisher_ms = device_ms(lambda: p.fisher(th, dg), reps)
    P, E, N = p.ntheta, 0 if dg is None else 1, p.N
    flop = batch * (P * 4.0 / 3.0 + E * 2.0 / 3.0) * float(N) ** 3
    return {"script": "fisher_time", "model": model, "n": n, "N": N, "batch": batch, "P": P, "E": E, "dtype": "float64",
            "fit_step_ms": fit_ms, "fisher_ms": fisher_ms, "fisher_in_fit_steps": fisher_ms / fit_ms, "flop": flop,
            "fisher_TFLOPs": flop / fisher_ms / 1e9,
            "work_bytes": int(p.lib.dgp_fisher_workspace_bytes(p._h, E))}


def main():
    assert torch.cuda.is_available(), "fisher_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    for model, d, n, batch in CASES:
        print(json.dumps(case(model, d, n, batch, dev)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
