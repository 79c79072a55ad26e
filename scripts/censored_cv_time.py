"""Timing of dgp_laplace_cross_validate at n = 4096 with 30 % censored rows against one laplace_factorize cache build."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from discontinuum_amd.backend import GPPlan  # noqa: E402
from oracle import gp_oracle as orc  # noqa: E402
from tests import censored_helpers as ch  # noqa: E402

dev = torch.device("cuda:0")
n, d = 4096, 2
X, _ = orc.synth_loadest(n, d, seed=1)
y, side, v, m = ch.synth(X, 0.3, 1)
nt = orc.loadest_ntheta(d)
theta = torch.full((nt,), 0.6931471805599453, dtype=torch.float64) * torch.linspace(0.8, 1.3, nt, dtype=torch.float64)
plan = GPPlan("loadest", n, d, dtype=torch.float64, device=dev)
plan.set_inputs(torch.tensor(X).to(dev).contiguous())
T = lambda a, dt=torch.float64: torch.as_tensor(a, dtype=dt).to(dev).contiguous()  # noqa: E731
yd, vd, md, sd = T(y), T(v), T(m), T(side, torch.int32)


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts))


out, f_hat, stat = plan.laplace_factorize(theta, yd, md, vd, sd)
print("newton iterations", stat[0], "capped", stat[3], flush=True)
print("laplace_factorize cold (ms, median/min)", timed(lambda: plan.laplace_factorize(theta, yd, md, vd, sd)), flush=True)
print("laplace_factorize warm start (ms)", timed(lambda: plan.laplace_factorize(theta, yd, md, vd, sd, f=f_hat)), flush=True)
print("factorize alone (ms)", timed(lambda: plan.factorize(theta, yd - md, vd)), flush=True)
plan.laplace_factorize(theta, yd, md, vd, sd, f=f_hat)
loo = np.arange(n)
k10 = np.arange(n) * 10 // n
k64 = np.arange(n) % 64
print("cavity LOO (ms)", timed(lambda: plan.laplace_cross_validate(theta, yd, md, vd, sd, f_hat, loo)), flush=True)
print("cavity 10 folds (ms)", timed(lambda: plan.laplace_cross_validate(theta, yd, md, vd, sd, f_hat, k10)), flush=True)
print("cavity 64 folds (ms)", timed(lambda: plan.laplace_cross_validate(theta, yd, md, vd, sd, f_hat, k64)), flush=True)
print("plain cross_validate LOO on the same plan (ms)", timed(lambda: plan.cross_validate(loo)), flush=True)
print("plain cross_validate 10 folds (ms)", timed(lambda: plan.cross_validate(k10)), flush=True)
Xs = torch.tensor(X).to(dev).contiguous()
print("predict at Xs = X (ms)", timed(lambda: plan.predict(theta, Xs)), flush=True)
print("posterior_cov at Xs = X (ms)", timed(lambda: plan.posterior_cov(theta, Xs)), flush=True)
