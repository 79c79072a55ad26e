"""Device time of the third-moment pass (``dgp_period_third_moments``) beside ``dgp_posterior_cov`` and ``dgp_period_moments`` on the
same covariance buffer, in one process: loadest d = 2, fp64, n = 1000 training points, one site at m = 7305 days with P = 20
yearly periods, m = 7305 with P = 1 (the whole record as one period) and m = 11 323 with P = 31 (``--cases`` selects; ``--tile``
forces a tile core).  HIP events after a warm-up call, median of the repetitions.  ``product_flop`` counts what the sandwich kernel executes by its own rule -- lower
128-tiles (64-tiles when the launch has few), 2 BT^2 flop per k of the range a tile pair shares, pairs that share none skipped --
and ``third_TFLOPs`` divides it by the time of the WHOLE call (prep, mirror, product, row and finish passes), so it is a lower bound
of the product kernel's rate.  Every result is checked against the dense formula in torch on the device (``k3_rel_err``).
Prints one JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, ".."), HERE]
from discontinuum_amd import _lib  # noqa: E402
from discontinuum_amd.backend import MODE_LOG, GPPlan  # noqa: E402
from flux_time import device_ms  # noqa: E402
from oracle import gp_oracle as orc  # noqa: E402

CASES = {"7305x20": (7305, 20), "7305x1": (7305, 1), "11323x31": (11323, 31)}


def product_flop(groups, M, tile):
    """Flop of the sandwich launch for non-decreasing ``groups`` (m,) on an M x M buffer, by the kernel's rule."""
    m, nb = len(groups), M // tile
    start = np.searchsorted(groups, groups, side="left")
    end = np.searchsorted(groups, groups, side="right")
    lo = np.array([start[b * tile:min((b + 1) * tile, m)].min() if b * tile < m else M for b in range(nb)])
    hi = np.array([end[b * tile:min((b + 1) * tile, m)].max() if b * tile < m else 0 for b in range(nb)])
    k0, k1 = np.maximum(lo[:, None], lo[None, :]), np.minimum(hi[:, None], hi[None, :])
    width = np.where(k1 > k0, np.minimum((k1 + 15) // 16 * 16, M) - k0 // 16 * 16, 0)
    return 2.0 * tile * tile * float(np.tril(width).sum())


def dense_k3(cov, m, mu, s2, w, groups, P):
    """The closed form period by period on the device: e = expm1(s2 C_gg), k3 = sum a a e (e diag(a) e^T) + 3 sum a (e a)^2."""
    out = torch.zeros(P, dtype=torch.float64, device=cov.device)
    a = w * torch.exp(mu + 0.5 * s2 * cov.diagonal()[:m])
    g = groups.cpu().numpy()
    for p in range(P):
        idx = np.nonzero(g == p)[0]
        i0, i1 = int(idx[0]), int(idx[-1]) + 1
        blk = cov[i0:i1, i0:i1]
        e = torch.expm1(s2 * (torch.tril(blk) + torch.tril(blk, -1).T))
        ap = a[i0:i1]
        out[p] = (ap[:, None] * ap[None, :] * e * ((e * ap[None, :]) @ e.T)).sum() + 3.0 * (ap * (e @ ap) ** 2).sum()
    return out


def case(m, P, dev, reps, tile=0):
    n, d = 1000, 2
    X, y = orc.synth_loadest(n, d, seed=2)
    X, y = torch.tensor(X), torch.tensor(y)
    theta = torch.full((orc.loadest_ntheta(d),), 0.6931471805599453, dtype=torch.float64)
    plan = GPPlan("loadest", n, d, dtype=torch.float64, device=dev)
    plan.set_inputs(X.to(dev).contiguous())
    plan.factorize(theta, (y - y.mean()).to(dev).contiguous(), torch.full((n,), 0.05, dtype=torch.float64, device=dev))
    t = torch.linspace(-2, 2, m, dtype=torch.float64)
    Xs = torch.stack([t, torch.sin(7 * t)], dim=1).to(dev).contiguous()
    kmean, cov = plan.posterior_cov(theta, Xs)
    g_host = np.minimum((np.arange(m) / 365.25).astype(np.int32), P - 1) if P > 1 else np.zeros(m, np.int32)
    assert int(g_host.max()) + 1 == P
    groups = torch.tensor(g_host, device=dev)
    w = torch.full((m,), 8.64, dtype=torch.float64, device=dev)
    mu, s2 = (0.5 * kmean + 1.0).contiguous(), 0.25
    k3 = plan.period_third_moments(cov, m, mu, s2, w, groups, P, tile=tile)
    ref = dense_k3(cov, m, mu, s2, w, groups, P)
    err = float((k3 - ref).abs().max() / ref.abs().max())
    _mean, pc = plan.period_moments(cov, m, mu, s2, w, groups, P, MODE_LOG)
    skew = (k3 / pc.diagonal() ** 1.5).cpu().numpy()
    cov_ms = device_ms(lambda: plan.posterior_cov(theta, Xs), reps)
    pm_ms = device_ms(lambda: plan.period_moments(cov, m, mu, s2, w, groups, P, MODE_LOG), reps)
    third_ms = device_ms(lambda: plan.period_third_moments(cov, m, mu, s2, w, groups, P, tile=tile), reps)
    M = int(cov.shape[0])
    nbk = M // 128
    if tile == 0:
        tile = 64 if nbk * (nbk + 1) // 2 <= 1000 else 128  # the rule of tile = 0 (DGP_OPT_LAUUM64_MAX_TILES' default)
    flop = product_flop(g_host, M, tile)
    return {"script": "skew_bench", "model": "loadest", "n": n, "m": m, "M": M, "P": P, "dtype": "float64", "tile": tile,
            "posterior_cov_ms": cov_ms, "period_moments_ms": pm_ms, "period_third_moments_ms": third_ms, "product_flop": flop,
            "third_TFLOPs": flop / max(third_ms, 1e-9) / 1e9, "k3_rel_err": err, "skewness_min": float(skew.min()),
            "skewness_max": float(skew.max()), "work_bytes": int(_lib.load().dgp_period_third_moments_workspace_bytes(m, P, 1))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="7305x20,7305x1,11323x31")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tile", type=int, default=0, choices=(0, 64, 128), help="force a tile core (0: the entry's own rule)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "skew_bench.py measures on the GPU"
    dev = torch.device("cuda:0")
    for key in args.cases.split(","):
        m, P = CASES[key]
        print(json.dumps(case(m, P, dev, args.reps, args.tile)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
