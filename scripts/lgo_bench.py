"""Device time of the leave-group-out fit step (``dgp_lgo_fit_step``) beside the leave-one-out step (``dgp_loo_fit_step``) and the
marginal-likelihood step (``dgp_fit_step``): loadest d = 3, fp64, n = 2048 and n = 8192 with 8 contiguous folds, 64 contiguous
folds and folds of one, and a batch of 32 sites at n = 8192 with 8 folds (``--cases`` selects).  HIP events after a warm-up call,
median of the repetitions, ONE PROCESS PER CASE (the driver starts a fresh child for each).

``--baseline-root DIR``: a checkout of the PARENT commit with its library built.  Each case then also runs, in a child of its
own on the same device, ``fit_step`` and ``loo_fit_step`` from THAT checkout: the baseline of ``ratio_to_parent_loo`` is never the
code under test.  Without it the ratios are taken against this checkout's own ``loo_fit_step`` and say so (``baseline``).

``gfw_flop`` = 2 N sum_g b_g^2 (the product G = F W), ``sandwich_flop`` = N^2 (N + 128) (the lower 128-tiles of M2 = F G^T), for
the expectation from the flop count; ``flop_expectation`` = 1 + gfw_flop / sandwich_flop x (loo - fit) / loo of the baseline: the
product charged at the rate of everything ``loo_fit_step`` adds to ``fit_step``.  Prints one JSON line per case."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"2048/8": (2048, 1, 8), "2048/64": (2048, 1, 64), "2048/ones": (2048, 1, 0), "8192/8": (8192, 1, 8), "8192/64": (8192, 1, 64),
         "8192/ones": (8192, 1, 0), "32x8192/8": (8192, 32, 8)}


def measure(root, key, steps):
    """In a child: the median device milliseconds of ``steps`` for the case ``key`` with the package of the checkout ``root``."""
    sys.path[:0] = [root, os.path.join(root, "scripts")]
    import torch

    from discontinuum_amd import _lib
    from discontinuum_amd.backend import GPPlan
    from flux_time import device_ms
    from oracle import gp_oracle as orc

    n, batch, k = CASES[key]
    assert torch.cuda.is_available(), "lgo_bench.py measures on the GPU"
    dev = torch.device("cuda:0")
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
    groups = torch.arange(n) if k == 0 else torch.arange(n) * k // n  # k contiguous folds of n / k
    sizes = torch.bincount(groups).double()
    reps = 3 if n >= 4096 else 10
    res = {"N": p.N, "folds": int(groups.max()) + 1, "max_fold": int(sizes.max()), "gfw_flop": batch * 2.0 * p.N * float((sizes ** 2).sum()),
           "sandwich_flop": batch * float(p.N) ** 2 * (p.N + 128.0)}
    for step in steps:
        if step == "lgo":
            p.set_folds(groups.expand(lead + (n,)).contiguous())
            res["work_bytes"] = int(p.lib.dgp_lgo_workspace_bytes(p._h, p._folds[2], p._folds[3]))
        fn = {"fit": p.fit_step, "loo": p.loo_fit_step, "lgo": getattr(p, "lgo_fit_step", None)}[step]
        out = fn(th, yd, nd)[0]
        assert bool((out[..., _lib.OUT_INFO] == 0).all()) and bool(torch.isfinite(out[..., _lib.OUT_NLL]).all())
        res[f"{step}_fit_step_ms" if step != "fit" else "fit_step_ms"] = device_ms(lambda fn=fn: fn(th, yd, nd), reps)
    print("LGO_BENCH_CHILD " + json.dumps(res), flush=True)


def child(root, key, steps):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", key, "--root", root, "--steps", ",".join(steps)]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    for line in done.stdout.splitlines():
        if line.startswith("LGO_BENCH_CHILD "):
            return json.loads(line[len("LGO_BENCH_CHILD "):])
    raise RuntimeError(f"case {key} from {root} failed (exit {done.returncode}):\n{done.stdout[-2000:]}\n{done.stderr[-4000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=os.path.join(HERE, ".."))
    ap.add_argument("--steps", default="fit,loo,lgo")
    args = ap.parse_args()
    if args.child is not None:
        return measure(os.path.abspath(args.root), args.child, args.steps.split(","))
    for key in args.cases.split(","):
        n, batch, _k = CASES[key]
        new = child(os.path.abspath(args.root), key, ["fit", "loo", "lgo"])
        row = {"script": "lgo_bench", "model": "loadest", "case": key, "n": n, "batch": batch, "dtype": "float64", **new}
        base = new
        row["baseline"] = "this checkout"
        if args.baseline_root:
            base = child(os.path.abspath(args.baseline_root), key, ["fit", "loo"])
            row.update(baseline="parent checkout", parent_fit_step_ms=base["fit_step_ms"], parent_loo_fit_step_ms=base["loo_fit_step_ms"])
        row["ratio_to_parent_loo"] = new["lgo_fit_step_ms"] / base["loo_fit_step_ms"]
        row["ratio_to_parent_fit"] = new["lgo_fit_step_ms"] / base["fit_step_ms"]
        row["flop_expectation"] = 1.0 + row["gfw_flop"] / row["sandwich_flop"] * (
            (base["loo_fit_step_ms"] - base["fit_step_ms"]) / base["loo_fit_step_ms"])
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
