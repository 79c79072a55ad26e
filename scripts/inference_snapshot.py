#!/usr/bin/env python
"""Bitwise record of everything a ``GPPlan`` computes from a held factorisation, for refactors of the host glue that must not
move a number: seeded inputs, one fit, and the outputs of ``fit_step``, ``factorize``, ``predict``, ``predict_mean``,
``mean_vjp``, ``predict_terms`` / ``predict_slopes`` (with and without ``return_cov``), ``posterior_cov``,
``posterior_period_moments``, ``period_moments``, ``period_third_moments`` (tile 0, 64, 128), ``exceedance_moments``,
``posterior_exceedance_moments``, ``sample_value``, ``posterior_sample_value``, ``posterior_cov_columns``,
``lowrank_period_moments``, ``window_moments``, ``whiten`` and ``cross_validate``, the dense and streamed exceedance, excess and
rolling-window passes with every chunk width of their level loops and ``posterior_cov_block`` (``streamed_products``); for one site and the
ragged batch of three, ``fisher``, ``predict_sensitivity`` (also means only in chunks), ``deletion_influence``, ``loo_fit_step`` /
``loo_value``, ``bilinear``, ``laplace_factorize``, ``laplace_fit_step`` (with and without an interval row),
``laplace_cross_validate``, ``ep_fit_step`` cold and warm, ``ep_factorize``, ``ep_diag`` and the pointwise ``censored_terms`` /
``interval_terms`` / ``bvn_excess`` (``extra_products``); and, for one site, ``posterior_factor`` + ``sample_draws`` from a seeded
device generator, ``cross_gram`` and the single stages with their buffers (``single_site_products``).

    python scripts/inference_snapshot.py --write before.pt      # on the commit to compare against
    python scripts/inference_snapshot.py --compare before.pt    # on the new one: exit status 1 unless every tensor is equal

Shapes: n = 300 (N = 384), m = 200 (M = 256: pad columns exist), every chunked call once whole and once with ``chunk=128``
(two staged chunks); loadest d = 3 in float64 and rating d = 2 in float32 (refinement on); one site, a ragged batch of three
(300, 257, 129 rows) and a batch of nine (hyperparameters through the plan's device scratch and a pinned staging slot).
``--root`` selects the tree whose package is imported.  One JSON line per run."""
import argparse
import json
import os
import sys

M_POINTS, N_ROWS, GROUPS, LEVELS = 200, 300, 4, 2
CONFIGS = [(model, d, dtype, sizes)
           for model, d, dtype in (("loadest", 3, "f64"), ("rating", 2, "f32"))
           for sizes in ((300,), (300, 257, 129), (300,) * 9)]


def run_config(torch, GPPlan, backend, make_case, model, d, dtype, sizes, dev):
    """-> {name: CPU tensor} of one configuration."""
    B, n, m = len(sizes), N_ROWS, M_POINTS
    lead = () if B == 1 else (B,)
    cases = [make_case(model, d, n, seed=10 + b, perturb=0.2) for b in range(B)]
    tests = [make_case(model, d, m, seed=40 + b)[0] for b in range(B)]

    def stack(parts, dt):
        t = torch.stack([p.to(dt) for p in parts]) if B > 1 else parts[0].to(dt)
        return t.to(dev).contiguous()

    X, r, noise = (stack([c[k] for c in cases], dtype) for k in range(3))
    theta = torch.stack([c[3] for c in cases]) if B > 1 else cases[0][3]
    Xs = stack(tests, dtype)
    g = torch.Generator().manual_seed(7)
    wv = stack([torch.randn(m, generator=g, dtype=torch.float64) for _ in range(B)], dtype)
    mu = stack([0.3 * torch.randn(m, generator=g, dtype=torch.float64) for _ in range(B)], dtype)
    extra = stack([0.01 + 0.02 * torch.rand(m, generator=g, dtype=torch.float64) for _ in range(B)], dtype)
    w = stack([0.5 + torch.rand(m, generator=g, dtype=torch.float64) for _ in range(B)], torch.float64)
    thresh = stack([torch.randn(LEVELS, m, generator=g, dtype=torch.float64) for _ in range(B)], torch.float64)
    ids = (torch.arange(m) * GROUPS // m).to(torch.int32)
    ids[5::17] = -1
    groups = ids.expand(lead + (m,)).contiguous()
    scale2 = 0.25 if B == 1 else [0.25 + 0.05 * b for b in range(B)]
    folds = torch.arange(n) % 5
    folds[3::29] = -1
    folds = folds.expand(lead + (n,)).contiguous()

    plan = GPPlan(model, n, d, dtype=dtype, device=dev, batch=B)
    if B > 1:
        plan.set_site_sizes(sizes)
    plan.set_inputs(X)
    cols = [c for c in range(d) if int(plan.lib.dgp_model_input_differentiable(backend.model_id(model), d, c)) == 1]
    out = {}

    def keep(name, value):
        for i, t in enumerate(value if isinstance(value, (tuple, list)) else (value,)):
            if t is not None:
                out[f"{name}.{i}"] = t.detach().cpu()

    keep("fit_step", plan.fit_step(theta, r, noise))
    for site in sorted({0, B - 1}):  # the inverse factor the step left: site 0, and the shortest site of the ragged batch
        jac = torch.randn(sizes[site], 2, generator=torch.Generator().manual_seed(13), dtype=torch.float64).to(dev)
        keep(f"whiten_site{site}", plan.whiten(jac, site))
    keep("mean_vjp", plan.mean_vjp(theta, Xs, wv))
    keep("cross_validate_after_fit_step", plan.cross_validate(folds))
    keep("factorize", plan.factorize(theta, r, noise))
    keep("predict", plan.predict(theta, Xs))
    keep("predict_chunk128", plan.predict(theta, Xs, chunk=128))
    keep("predict_mean", plan.predict_mean(theta, Xs))
    for return_cov in (True, False):
        for chunk in (None, 128):
            tag = f"{'cov' if return_cov else 'mean'}_{'whole' if chunk is None else 'chunk128'}"
            keep(f"predict_terms_{tag}", plan.predict_terms(theta, Xs, chunk=chunk, return_cov=return_cov))
            keep(f"predict_slopes_{tag}", plan.predict_slopes(theta, Xs, cols, chunk=chunk, return_cov=return_cov))
    kmean, cov = plan.posterior_cov(theta, Xs)
    keep("posterior_cov", (kmean, torch.tril(cov)[..., :m, :m]))  # the part the layout defines
    keep("period_moments", plan.period_moments(cov, m, mu, scale2, w, groups, GROUPS, backend.MODE_LOG, extra_var=extra))
    for tile in (0, 64, 128):
        keep(f"period_third_moments_tile{tile}", plan.period_third_moments(cov, m, mu, scale2, w, groups, GROUPS, extra_var=extra, tile=tile))
    keep("exceedance_moments", plan.exceedance_moments(cov, m, mu, thresh, w, groups, GROUPS, extra_var=extra))
    keep("posterior_exceedance_moments",  # two panels of 128 rows
         plan.posterior_exceedance_moments(theta, Xs, mu, thresh, w, groups, GROUPS, extra_var=extra, panel_rows=128))
    given = stack([0.05 * torch.randn(3, m, generator=g, dtype=torch.float64) for _ in range(B)], torch.float64)
    keep("sample_value", plan.sample_value(cov, m, w, scale2, groups, GROUPS, obs_var=extra, rows=given, nterms=12))
    keep("sample_value_linear", plan.sample_value(cov, m, w, scale2, groups, GROUPS, nterms=1))
    i = torch.arange(m)
    lo = (i - 29).clamp_min(0).to(torch.int32).expand(lead + (m,)).contiguous()  # trailing windows of 30 points
    hi = (i + 1).to(torch.int32).expand(lead + (m,)).contiguous()
    wmean, wcov = plan.window_moments(cov, m, mu, lo, hi, a=w)
    keep("window_moments_linear", (wmean, torch.tril(wcov)[..., :m, :m]))
    wmean, wcov = plan.window_moments(cov, m, mu, lo, hi, a=w, mode=backend.MODE_LOG, scale2=scale2)
    keep("window_moments_log", (wmean, torch.tril(wcov)[..., :m, :m]))
    keep("posterior_period_moments_log", plan.posterior_period_moments(theta, Xs, mu, scale2, w, groups, GROUPS, backend.MODE_LOG))
    keep("posterior_period_moments_linear",
         plan.posterior_period_moments(theta, Xs, mu, scale2, w, groups, GROUPS, backend.MODE_LINEAR, extra_var=extra))
    keep("posterior_sample_value",  # two panels of 128 rows
         plan.posterior_sample_value(theta, Xs, w, scale2, groups, GROUPS, obs_var=extra, rows=given, nterms=12, panel_rows=128))
    keep("posterior_cov_columns", plan.posterior_cov_columns(theta, Xs, torch.tensor([0, 127, 128, m - 1]).expand(lead + (4,))))
    keep("lowrank_period_moments", plan.lowrank_period_moments(given.to(dev), m, mu.double(), scale2, w, groups, GROUPS, backend.MODE_LOG))
    streamed_products(torch, plan, backend, keep, stack, theta, Xs, cov, mu, extra, w, groups, scale2, lo, hi, dtype, make_case)
    keep("cross_validate", plan.cross_validate(folds))
    if B <= 3:  # the products whose host glue lives beside their kernels: one site and the ragged batch of three
        extra_products(torch, plan, backend, keep, theta, X, r, noise, Xs, w, folds, groups, extra, dtype, dev)
    if B == 1:
        single_site_products(torch, plan, keep, theta, r, noise, Xs, dev)
    torch.cuda.synchronize(dev)
    return out


def streamed_products(torch, plan, backend, keep, stack, theta, Xs, cov, mu, extra, w, groups, scale2, lo, hi, dtype, make_case):
    """The dense and streamed passes with every chunk width of their level loops -- the exceedance pair with 15 levels (chunks
    of 8, 4, 2, 1), the excess pair with 11 (a group of 8, then 3 as 2 + 1), the streamed ones with two panels of 128 rows --,
    ``window_variances`` dense and streamed in both modes, and blocks of the covariance; then the band products on a second
    set of 300 test points (M = 384) with windows of at most 7 points: the third panel's band starts at column 128."""
    B, m = plan.batch, M_POINTS
    lead = () if B == 1 else (B,)
    g = torch.Generator().manual_seed(9)
    t15, t11 = (stack([torch.randn(L, m, generator=g, dtype=torch.float64) for _ in range(B)], torch.float64) for L in (15, 11))
    keep("exceedance_moments_L15", plan.exceedance_moments(cov, m, mu, t15, w, groups, GROUPS, extra_var=extra))
    keep("posterior_exceedance_moments_L15",
         plan.posterior_exceedance_moments(theta, Xs, mu, t15, w, groups, GROUPS, extra_var=extra, panel_rows=128))
    for above in (True, False):
        tag = "above" if above else "below"
        keep(f"excess_moments_L11_{tag}", plan.excess_moments(cov, m, mu, scale2, t11, w, groups, GROUPS, above=above, extra_var=extra))
        keep(f"posterior_excess_moments_L11_{tag}",
             plan.posterior_excess_moments(theta, Xs, mu, scale2, t11, w, groups, GROUPS, above=above, extra_var=extra, panel_rows=128))
    modes = (("linear", backend.MODE_LINEAR, None), ("log", backend.MODE_LOG, scale2))
    for tag, mode, s2 in modes:
        keep(f"window_variances_{tag}", plan.window_variances(cov, m, mu, lo, hi, a=w, mode=mode, scale2=s2))
        keep(f"posterior_window_variances_{tag}",
             plan.posterior_window_variances(theta, Xs, mu, lo, hi, a=w, mode=mode, scale2=s2, panel_rows=128))
    keep("posterior_cov_block", torch.tril(plan.posterior_cov_block(theta, Xs, 128, 256, 0), diagonal=128))  # the defined part
    m3 = 300
    Xs3 = stack([make_case(plan.model, plan.d, m3, seed=70 + b)[0] for b in range(B)], dtype)
    mu3 = stack([0.3 * torch.randn(m3, generator=g, dtype=torch.float64) for _ in range(B)], dtype)
    w3 = stack([0.5 + torch.rand(m3, generator=g, dtype=torch.float64) for _ in range(B)], torch.float64)
    i = torch.arange(m3)
    lo3 = (i - 6).clamp_min(0).to(torch.int32).expand(lead + (m3,)).contiguous()  # trailing windows of 7 points
    hi3 = (i + 1).to(torch.int32).expand(lead + (m3,)).contiguous()
    for tag, mode, s2 in modes:
        keep(f"posterior_window_variances_m300_{tag}",
             plan.posterior_window_variances(theta, Xs3, mu3, lo3, hi3, a=w3, mode=mode, scale2=s2, panel_rows=128))
    keep("posterior_cov_block_m300", torch.tril(plan.posterior_cov_block(theta, Xs3, 256, 384, 128), diagonal=128))


def single_site_products(torch, plan, keep, theta, r, noise, Xs, dev):
    """posterior_factor + sample_draws (seeded device generator) and cross_gram on whatever factorisation the plan holds, then
    the single stages, which replace it: the defined part of every buffer after its stage, and stage_grad."""
    from discontinuum_amd import _lib

    n, m = plan.n, Xs.shape[0]
    try:
        mean, Lbuf, jitter = plan.posterior_factor(theta, Xs)
        keep("posterior_factor", (mean, torch.tril(Lbuf)[:m, :m], torch.tensor([jitter], dtype=torch.float64)))
        draws = plan.sample_draws(Lbuf, m, mean, 8, generator=torch.Generator(device=dev).manual_seed(5))
        keep("sample_draws", (draws, plan._last_z))
    except RuntimeError as e:  # not positive definite after the last jitter: part of the record
        keep("posterior_factor.error", torch.tensor([len(str(e)) > 0]))
    keep("cross_gram", plan.cross_gram(theta, Xs))
    stages = (("gram", _lib.BUF_A, (theta, noise)), ("potrf", _lib.BUF_A, ()), ("trtri", _lib.BUF_T, ()), ("lauum", _lib.BUF_S, ()),
              ("solve", _lib.BUF_ALPHA, (r,)))
    try:
        for name, which, args in stages:
            getattr(plan, "stage_" + name)(*args)
            buf = plan.buffer(which)
            keep("stage_" + name, buf[:n] if buf.dim() == 1 else torch.tril(buf)[:n, :n])
        keep("stage_grad", plan.stage_grad(theta))
    except _lib.DGPError as e:  # a refusal is part of the record
        keep("stage.error", torch.tensor([e.code]))


def extra_products(torch, plan, backend, keep, theta, X, r, noise, Xs, w, folds, groups, extra, dtype, dev):
    """fisher, predict_sensitivity, deletion_influence on the held factorisation; then, float64 only, the steps that replace it:
    loo_fit_step / loo_value, laplace_fit_step (a third of the rows censored; then with one interval row and ``upper``),
    laplace_cross_validate and ep_fit_step cold and warm (the last two: one site)."""
    from discontinuum_amd._lib import DGPError

    B, n = plan.batch, plan.n
    lead = () if B == 1 else (B,)
    g = torch.Generator().manual_seed(11)
    cols = torch.randn(lead + (2, n), generator=g, dtype=torch.float64).to(dtype).to(dev)
    rhs = torch.randn(lead + (2, n), generator=g, dtype=torch.float64).to(dtype).to(dev)

    def attempt(name, call):  # a refusal is part of the record: its code, and what the call left behind is compared by the next rows
        try:
            keep(name, call())
        except DGPError as e:
            keep(name + ".error", torch.tensor([e.code]))

    def stat_tensor(value):
        return torch.tensor(value, dtype=torch.float64)

    keep("fisher", plan.fisher(theta, diag=cols))
    keep("predict_sensitivity", plan.predict_sensitivity(theta, Xs, diag=cols, rhs=rhs))
    keep("predict_sensitivity_mean_chunk128", plan.predict_sensitivity(theta, Xs, diag=cols, rhs=rhs, chunk=128, return_var=False))
    inv_sd = (1.0 + w).to(torch.float64)
    scale = 0.5 if B == 1 else [0.5 + 0.1 * b for b in range(B)]
    keep("deletion_influence_linear",
         plan.deletion_influence(theta, Xs, folds, w, scale, groups, GROUPS, backend.MODE_LINEAR, inv_sd=inv_sd))
    keep("deletion_influence_log", plan.deletion_influence(theta, Xs, folds, w, scale, groups, GROUPS, backend.MODE_LOG))
    if dtype != torch.float64:
        return
    keep("loo_fit_step", plan.loo_fit_step(theta, r, noise))
    keep("loo_value", plan.loo_value())
    u, al = (torch.randn(lead + (n,), generator=g, dtype=torch.float64).to(dev) for _ in range(2))
    keep("bilinear", plan.bilinear(theta, u, al))
    side = torch.zeros(lead + (n,), dtype=torch.int32)
    side[..., ::3] = -1  # a third of the rows: the truth lies below the recorded value
    mean = torch.zeros_like(r)

    def factorized(res):  # (out, f_hat or (y~, n~), stat) of a *_factorize as tensors
        mid = res[1] if isinstance(res[1], tuple) else (res[1],)
        return (res[0],) + mid + (stat_tensor(res[2]),)

    attempt("laplace_factorize_censored", lambda: factorized(plan.laplace_factorize(theta, r, mean, noise, side.to(dev).contiguous())))

    def laplace(upper):
        res = plan.laplace_fit_step(theta, r, mean, noise, side.to(dev).contiguous(), upper=upper)
        return res[:3] + (stat_tensor(res[3]),)

    attempt("laplace_fit_step", lambda: laplace(None))
    side[..., 1] = 2  # one interval row: the truth in [y, y + 0.5]
    upper = r + 0.5
    side_dev = side.to(dev).contiguous()
    attempt("laplace_interval_fit_step", lambda: laplace(upper))
    if B != 1:
        return
    f_hat = out_f = None
    try:
        out_f = plan.laplace_factorize(theta, r, mean, noise, side_dev, upper=upper)
        f_hat = out_f[1]
        keep("laplace_factorize", out_f[:2] + (stat_tensor(out_f[2]),))
    except DGPError as e:
        keep("laplace_factorize.error", torch.tensor([e.code]))
    if f_hat is not None:
        def lcv():
            res = plan.laplace_cross_validate(theta, r, mean, noise, side_dev, f_hat, folds, upper=upper, shift=0.5)
            return tuple(res[k] for k in sorted(res))

        attempt("laplace_cross_validate", lcv)

    def ep(sites):
        res = plan.ep_fit_step(theta, r, mean, noise, side_dev, sites=sites, upper=upper)
        aux = plan.ep_aux
        return (res[0], res[1], res[2][0], res[2][1], stat_tensor(res[3]), aux["cav_mean"], aux["cav_var"], aux["logz"])

    attempt("ep_fit_step_cold", lambda: ep(None))
    if getattr(plan, "ep_sites", None) is not None:
        warm = tuple(t.clone() for t in plan.ep_sites)
        attempt("ep_fit_step_warm", lambda: ep(warm))
    attempt("ep_factorize", lambda: factorized(plan.ep_factorize(theta, r, mean, noise, side_dev, upper=upper)))
    attempt("ep_diag", plan.ep_diag)
    z = 3.0 * torch.randn(500, generator=g, dtype=torch.float64).to(dev)  # the pointwise functions of the censored fits
    delta = torch.rand(500, generator=g, dtype=torch.float64).to(dev)
    rho = (2.0 * torch.rand(500, generator=g, dtype=torch.float64) - 1.0).to(dev)
    keep("censored_terms", plan.censored_terms(z))
    keep("interval_terms", plan.interval_terms(z, delta))
    keep("bvn_excess", backend.bvn_excess(z, z.flip(0).contiguous(), rho))


def same_bits(torch, a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def main():
    ap = argparse.ArgumentParser()
    what = ap.add_mutually_exclusive_group(required=True)
    what.add_argument("--write", metavar="FILE")
    what.add_argument("--compare", metavar="FILE")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch

    from discontinuum_amd import backend
    from discontinuum_amd.backend import GPPlan
    from tests.test_gpu_stages import make_case

    dev = torch.device("cuda:0")
    snap = {}
    for model, d, dtype, sizes in CONFIGS:
        tensors = run_config(torch, GPPlan, backend, make_case, model, d, torch.float64 if dtype == "f64" else torch.float32, sizes, dev)
        for name, t in tensors.items():
            snap[f"{model}-{dtype}-batch{len(sizes)}/{name}"] = t
    result = {"root": os.path.abspath(args.root), "tensors": len(snap), "bytes": sum(t.numel() * t.element_size() for t in snap.values()),
              "device": torch.cuda.get_device_name(dev)}
    if args.write:
        torch.save(snap, args.write)
        result["written"] = args.write
    else:
        ref = torch.load(args.compare)
        differ = sorted(k for k in ref if k not in snap or not same_bits(torch, ref[k], snap[k]))
        added = sorted(k for k in snap if k not in ref)  # a product the compared commit did not have yet
        result.update(compared=args.compare, differ=differ, added=added, bitwise_equal=not differ)
    print(json.dumps(result))
    return 0 if args.write or not differ else 1


if __name__ == "__main__":
    sys.exit(main())
