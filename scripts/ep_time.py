"""Expectation propagation against Laplace on one record (loadest d = 3, n = 2048, 50 % censored), same hyperparameters: sweeps and
time per call, cold and warm; then ``ep_diag`` against its n^2 / 2 x 8-byte traffic bound (EXPERIMENTS.md).  Run from the repository
root: ``python scripts/ep_time.py``."""
import sys, time
sys.path.insert(0, ".")  # the repository root
import numpy as np, torch
from discontinuum_amd.backend import GPPlan
from oracle import gp_oracle as orc
from tests import interval_helpers as ih

dev = torch.device("cuda:0")
def to(*a):
    return tuple(torch.as_tensor(x, dtype=torch.int32 if np.asarray(x).dtype.kind == "i" else torch.float64).to(dev).contiguous() for x in a)
def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); r = fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    return r, 1e3 * float(np.median(ts))

for n in (2048,):
    d = 3
    X = torch.tensor(orc.synth_loadest(n, d, seed=11)[0])
    y, side, v, m, upper = ih.synth(X.numpy(), 0.5, 11)
    theta = torch.full((orc.loadest_ntheta(d),), 0.6931471805599453, dtype=torch.float64) * torch.linspace(0.8, 1.3, orc.loadest_ntheta(d), dtype=torch.float64)
    theta2 = theta * 1.01
    plan = GPPlan("loadest", n, d, device=dev)
    plan.set_inputs(X.to(dev).contiguous())
    yd, vd, md, sd, ud = to(y, v, m, side, upper)
    print(f"n={n} censored rows {(side != 0).sum()} kinds {sorted(set(side.tolist()))}", flush=True)
    (_o, _a, _dn), t_plain = timed(lambda: plan.fit_step(theta, (yd - md).contiguous(), vd))
    print(f"plain fit_step {t_plain:.3f} ms", flush=True)
    (o, dr, sites, st), t = timed(lambda: plan.ep_fit_step(theta, yd, md, vd, sd, upper=ud))
    print(f"EP cold: {st[0]:.0f} sweeps, {t:.3f} ms, stat {st}", flush=True)
    (o2, dr2, sites2, st2), t = timed(lambda: plan.ep_fit_step(theta, yd, md, vd, sd, sites=sites, upper=ud))
    print(f"EP warm, same theta: {st2[0]:.0f} sweeps, {t:.3f} ms", flush=True)
    (o3, dr3, sites3, st3), t = timed(lambda: plan.ep_fit_step(theta2, yd, md, vd, sd, sites=sites, upper=ud))
    print(f"EP warm, theta x 1.01: {st3[0]:.0f} sweeps, {t:.3f} ms", flush=True)
    (lo, ldr, f, ls), t = timed(lambda: plan.laplace_fit_step(theta, yd, md, vd, sd, upper=ud))
    print(f"Laplace cold: {ls[0]:.0f} Newton iterations, {t:.3f} ms", flush=True)
    (lo2, ldr2, f2, ls2), t = timed(lambda: plan.laplace_fit_step(theta, yd, md, vd, sd, f=f, upper=ud))
    print(f"Laplace warm, same theta: {ls2[0]:.0f} iterations, {t:.3f} ms", flush=True)
    (lo3, ldr3, f3, ls3), t = timed(lambda: plan.laplace_fit_step(theta2, yd, md, vd, sd, f=f, upper=ud))
    print(f"Laplace warm, theta x 1.01: {ls3[0]:.0f} iterations, {t:.3f} ms", flush=True)
    (_o, t_fac) = timed(lambda: plan.factorize(theta, (yd - md).contiguous(), vd))
    print(f"factorize alone {t_fac:.3f} ms; NLL EP {float(o[0]):.6f} Laplace {float(lo[0]):.6f}", flush=True)
    mu_ep = (sites[0] - sites[1] * dr); print(f"max |mu_EP - f_Laplace| / sigma on censored rows {float(((mu_ep - f).abs() / vd.sqrt())[sd != 0].max()):.3f}", flush=True)

for n in (2048, 8192):
    d = 3
    X = torch.tensor(orc.synth_loadest(n, d, seed=11)[0])
    plan = GPPlan("loadest", n, d, device=dev)
    plan.set_inputs(X.to(dev).contiguous())
    theta = torch.full((orc.loadest_ntheta(d),), 0.6931471805599453, dtype=torch.float64)
    r = torch.randn(n, dtype=torch.float64, device=dev); noise = torch.full((n,), 0.01, dtype=torch.float64, device=dev)
    plan.factorize(theta, r, noise)
    plan.ep_diag(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 200
    e0.record()
    for _ in range(reps):
        plan.ep_diag()
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    gb = n * n / 2 * 8 / 1e9
    print(f"ep_diag n={n}: {1e3 * ms:.1f} us per call (both launches), {gb * 1e3:.1f} MB -> {gb / (ms * 1e-3):.0f} GB/s", flush=True)
