"""The value of additional samples at the reference workflow's size (a daily grid over a 31-year record: m = 11 323 points,
P = 31 years, fp64) for a loadest-gp fit at n = 300: ``dgp_sample_value`` alone without and with 24 conditioning rows,
``dgp_period_moments`` (log mode) on the same buffer beside it, and the greedy ``LoadestGP.design`` at k = 24 as a whole.
Device times by HIP events after a warm-up call; achieved bytes/s over the M^2 elements the pass reads.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, ".."), HERE]
os.environ["TQDM_DISABLE"] = "1"
from discontinuum_amd import design as dsn  # noqa: E402
from discontinuum_amd.loadest_gp import LoadestGP  # noqa: E402
from discontinuum_amd.loads import DEFAULT_MAX_BYTES, flux_weights  # noqa: E402
from flux_time import M_DAYS, device_ms, record  # noqa: E402

SAMPLE_VAR = 0.01  # model-space noise of a hypothetical sample: the fixed observation variance of the loadest model
K_PICKS = 24


def main():
    assert torch.cuda.is_available(), "design_time.py measures on the GPU"
    obs, target, daily = record(300)
    model = LoadestGP()
    model.fit(obs, target, iterations=3)
    w = flux_weights(daily, {"units": "mg/l"})
    fit = dsn._prepare(model, daily, w, "YE", SAMPLE_VAR, DEFAULT_MAX_BYTES, extra_buffers=1)
    plan, P = model._plan, fit.P
    assert fit.m == M_DAYS and P == 31
    M = fit.cov.shape[-1]
    row = {"script": "design_time", "n": 300, "m": fit.m, "M": M, "P": P, "nterms": fit.nterms,
           "beta": float(fit.s2 * fit.diag.max())}
    with torch.no_grad():
        rows = dsn.conditioning_rows(fit, np.linspace(100, fit.m - 100, K_PICKS).astype(np.int64))
        obs_var = fit.obs_var
        call = lambda r: plan.sample_value(fit.cov, fit.m, fit.a, fit.s2, fit.groups, P, obs_var=obs_var, rows=r,  # noqa: E731
                                           nterms=fit.nterms)
        row["sample_value_rows0_ms"] = device_ms(lambda: call(None), 10)
        row["sample_value_rows24_ms"] = device_ms(lambda: call(rows), 10)
        row["sample_value_rows0_linear_ms"] = device_ms(
            lambda: plan.sample_value(fit.cov, fit.m, fit.a, fit.s2, fit.groups, P, obs_var=obs_var, nterms=1), 10)
        row["period_moments_ms"] = device_ms(
            lambda: plan.period_moments(fit.cov, fit.m, fit.mapped, fit.s2, fit.w, fit.groups, P, fit.mode), 10)
    nbytes = M * M * fit.cov.element_size()
    row["bytes"] = nbytes
    for key in ("sample_value_rows0", "sample_value_rows24", "sample_value_rows0_linear", "period_moments"):
        row[key + "_GBps"] = nbytes / row[key + "_ms"] / 1e6
    row["multiply_adds"] = 2.0 * fit.m * fit.m * fit.nterms
    row["sample_value_rows0_Gmadd_per_s"] = row["multiply_adds"] / row["sample_value_rows0_ms"] / 1e6
    del fit, rows
    torch.cuda.empty_cache()
    model.design(daily, 2, sample_var=SAMPLE_VAR)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    picked = model.design(daily, K_PICKS, sample_var=SAMPLE_VAR)
    torch.cuda.synchronize()
    row["design_k24_ms"] = (time.perf_counter() - t0) * 1e3
    row["design_k24_fraction_explained_min_max"] = [float(v) for v in (
        (picked["variance_explained"].values[-1] / picked["se_now"].values ** 2).min(),
        (picked["variance_explained"].values[-1] / picked["se_now"].values ** 2).max())]
    print(json.dumps(row))


if __name__ == "__main__":
    main()
