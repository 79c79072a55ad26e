"""GPU parity of ``dgp_cross_validate`` (exact leave-one-out / leave-group-out cross-validation from the held
factorisation) against fp64 dense DELETION on the CPU -- an independent route: the fold's rows and columns are removed
from K^, the rest is Cholesky-solved and the fold conditioned on it -- and, at n = 8192 where the oracle does not reach,
against identities that rest on the fit step alone.

Bounds: fp64 plans 1e-8 relative to the vector's max-norm for ``resid`` / ``var`` and 1e-8 max(1, |lpd|) for ``lpd`` -- the
bound this suite holds alpha and K^^-1-derived quantities to (tests/test_gpu_stages.py); the two CPU routes (deletion and
the partitioned-inverse identity in fp64) agree to <= 5e-13 / 4e-13 / 2e-12 on the worst of these inputs, so the reference
itself stays four orders inside.  fp32 plans: abs 1e-3 in model space on ``resid`` and ``var``, the project's fp32 row for
the predictive mean / variance.  Every printed figure is a measurement, the assertions are the bounds.
"""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as orc
from tests.crossval_helpers import dense_deletion_cv, posterior_deletion_reference
from tests.test_gpu_stages import CASES, make_case, plan_for

pytestmark = pytest.mark.gpu


def _schemes(n):
    return {
        "loo": np.arange(n),
        "16-block": np.arange(n) * 16 // n,
        "5-random": np.random.default_rng(0).permutation(n) % 5,
    }


def _errors(got, ref):
    resid, var, lpd, info = (t.cpu() for t in got)
    e_r = ((resid - ref[0]).abs().max() / ref[0].abs().max()).item()
    e_v = ((var - ref[1]).abs().max() / ref[1].abs().max()).item()
    e_l = ((lpd - ref[2]).abs() / ref[2].abs().clamp(min=1.0)).max().item()
    return e_r, e_v, e_l, info


@pytest.mark.parametrize("model,d,n", CASES)
def test_parity_with_dense_deletion_fp64(model, d, n, gpu_device):
    dev = gpu_device
    X, r, noise, theta = make_case(model, d, n, seed=1, perturb=0.3)
    Khat = orc.GRAMS[model](X, X, theta) + torch.diag(noise)
    p = plan_for(model, d, n, X, torch.float64, dev)
    for name, groups in _schemes(n).items():
        ref = dense_deletion_cv(Khat, r, groups)
        for state in ("factorize", "fit_step"):
            if state == "factorize":
                p.factorize(theta, r.to(dev), noise.to(dev))
            else:
                p.fit_step(theta, r.to(dev), noise.to(dev))
            e_r, e_v, e_l, info = _errors(p.cross_validate(groups), ref)
            print(f"crossval fp64 {model} d={d} n={n} {name} after {state}: resid {e_r:.2e} var {e_v:.2e} lpd {e_l:.2e}")
            assert e_r < 1e-8 and e_v < 1e-8 and e_l < 1e-8, (name, state, e_r, e_v, e_l)
            assert bool((info == 0).all()), (name, state)


@pytest.mark.parametrize("model,d,n", [("rating", 2, 900), ("loadest", 3, 1000)])
def test_parity_with_dense_deletion_fp32(model, d, n, gpu_device):
    """Measured on MI355X (abs, model space; EXPERIMENTS.md): rating n = 900 resid <= 1.9e-4, var <= 5.4e-5; loadest n = 1000
    resid <= 1.8e-5, var <= 6.0e-6 -- a factor 5 inside the row at the worst."""
    dev = gpu_device
    X, r, noise, theta = make_case(model, d, n, seed=1, perturb=0.3)
    Khat = orc.GRAMS[model](X, X, theta) + torch.diag(noise)
    p = plan_for(model, d, n, X, torch.float32, dev)
    schemes = _schemes(n)
    for name in ("loo", "16-block"):
        ref = dense_deletion_cv(Khat, r, schemes[name])
        for state in ("factorize", "fit_step"):
            if state == "factorize":
                p.factorize(theta, r.float().to(dev), noise.float().to(dev))
            else:
                p.fit_step(theta, r.float().to(dev), noise.float().to(dev))
            resid, var, lpd, info = (t.cpu() for t in p.cross_validate(schemes[name]))
            assert resid.dtype == torch.float64 and var.dtype == torch.float64 and lpd.dtype == torch.float64
            e_r, e_v = (resid - ref[0]).abs().max().item(), (var - ref[1]).abs().max().item()
            print(f"crossval fp32 {model} n={n} {name} after {state}: resid abs {e_r:.2e} var abs {e_v:.2e}")
            assert e_r < 1e-3 and e_v < 1e-3, (name, state, e_r, e_v)
            assert bool((info == 0).all())


def test_self_consistency_at_full_size(gpu_device):
    """n = 8192 (the benchmark's size), fp64, one plan: leave-one-out against the fit step's own dnoise, 16 blocks against
    a CPU solve with the blocks of K^^-1 read from the plan, and the packed-panel route (after a bare factorize) against
    the gather route."""
    from discontinuum_amd import _lib
    from discontinuum_amd.backend import GPPlan

    dev, n, d = gpu_device, 8192, 3
    X, y = orc.synth_loadest(n, d, seed=0)
    Xd, yd = torch.tensor(X, device=dev), torch.tensor(y, device=dev)
    noise = torch.full((n,), 0.01, dtype=torch.float64, device=dev)
    theta = torch.tensor([0.9, 0.7, 1.0, 1.5, 0.6, 0.8, 1.2, 0.3, 0.9, 0.7, 1.1], dtype=torch.float64)
    p = GPPlan("loadest", n, d, device=dev)
    p.set_inputs(Xd)
    out, alpha, dnoise = p.fit_step(theta, yd, noise)
    assert out[_lib.OUT_INFO].item() == 0
    resid, var, lpd, info = p.cross_validate(np.arange(n))
    var_ref = 1.0 / (2.0 * dnoise + alpha ** 2)
    assert bool((info == 0).all())
    assert ((var - var_ref).abs().max() / var_ref.abs().max()).item() < 1e-9
    assert ((resid - alpha * var_ref).abs().max() / (alpha * var_ref).abs().max()).item() < 1e-9
    blocks = np.arange(n) * 16 // n
    rs, vs, ls, info_s = p.cross_validate(blocks)
    S = p.buffer(_lib.BUF_S)
    ref = torch.empty(n, dtype=torch.float64)
    for f in range(16):
        B = torch.as_tensor(np.nonzero(blocks == f)[0], device=dev)
        Sbb = S[B][:, B].cpu()
        Sbb = torch.tril(Sbb) + torch.tril(Sbb, -1).T
        ref[B.cpu()] = torch.linalg.solve(Sbb, alpha[B].cpu())
    assert bool((info_s == 0).all())
    assert ((rs.cpu() - ref).abs().max() / ref.abs().max()).item() < 1e-9
    o2 = p.factorize(theta, yd, noise)
    assert o2[_lib.OUT_INFO].item() == 0
    rp, vp, lp, info_p = p.cross_validate(blocks)
    assert bool((info_p == 0).all())
    assert ((rp - rs).abs().max() / rs.abs().max()).item() < 1e-9
    assert ((vp - vs).abs().max() / vs.abs().max()).item() < 1e-9
    assert ((lp - ls).abs() / ls.abs().clamp(min=1.0)).max().item() < 1e-9


def test_state_is_preserved(gpu_device):
    dev = gpu_device
    model, d, n = "rating", 2, 300
    X, r, noise, theta = make_case(model, d, n, seed=4, perturb=0.2)
    Xs, *_ = make_case(model, d, 77, seed=5)
    w = torch.randn(77, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).to(dev)
    p = plan_for(model, d, n, X, torch.float64, dev)
    schemes = _schemes(n)
    p.factorize(theta, r.to(dev), noise.to(dev))
    before = [t.clone() for t in p.predict(theta, Xs.to(dev))]
    for groups in schemes.values():
        p.cross_validate(groups)
    after = p.predict(theta, Xs.to(dev))
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    p.fit_step(theta, r.to(dev), noise.to(dev))
    vjp0 = [t.clone() for t in p.mean_vjp(theta, Xs.to(dev), w)]
    grad0 = p.stage_grad(theta).clone()
    for groups in schemes.values():
        p.cross_validate(groups)
    vjp1 = p.mean_vjp(theta, Xs.to(dev), w)
    assert all(torch.equal(a, b) for a, b in zip(vjp0, vjp1))
    assert torch.equal(grad0, p.stage_grad(theta))


def test_batched_ragged_plan_matches_single_site_plans(gpu_device):
    """Four ragged sites with their own folds in one batched plan against four single-site plans under the same
    ``max_group`` bound (the bound selects the route).  Where the single-site plan's factor L^-1 is bitwise the batched
    site's, the results must be bitwise equal; where the factorisation's schedule differs, to 1e-11 (the tolerance
    tests/test_gpu_headline_shape.py holds batched against single-site factors to).  Measured on MI355X: every site of
    this test is bitwise."""
    from discontinuum_amd import _lib
    from discontinuum_amd.backend import GPPlan

    dev, model, d = gpu_device, "loadest", 3
    sizes = [300, 384, 257, 128]
    B, n = len(sizes), max(sizes)
    cases = [make_case(model, d, nb, seed=60 + b, perturb=0.1) for b, nb in enumerate(sizes)]
    X = torch.full((B, n, d), float("nan"), dtype=torch.float64)
    r = torch.full((B, n), float("nan"), dtype=torch.float64)
    noise = torch.full((B, n), float("nan"), dtype=torch.float64)
    for b, (nb, c) in enumerate(zip(sizes, cases)):
        X[b, :nb], r[b, :nb], noise[b, :nb] = c[0], c[1], c[2]
    theta = torch.stack([c[3] for c in cases])
    pb = GPPlan(model, n, d, device=dev, lookahead=1, batch=B)
    pb.set_site_sizes(sizes)
    pb.set_inputs(X.to(dev).contiguous())
    singles = [plan_for(model, d, nb, c[0], torch.float64, dev, lookahead=1) for nb, c in zip(sizes, cases)]
    rng = np.random.default_rng(7)

    def folds(kind, nb, b):
        if kind == "loo":
            g = np.arange(nb)
            g[b] = -1  # every site leaves a different observation in
            return g
        if kind == "blocks":
            return np.arange(nb) * (6 + b) // nb  # 6..9 contiguous blocks of at most 64
        return rng.permutation(nb) % (4 + b % 2)  # 4 or 5 random folds of 26 .. 77: the blocked route

    bitwise = []
    for state in ("factorize", "fit_step"):
        if state == "factorize":
            pb.factorize(theta, r.to(dev).contiguous(), noise.to(dev).contiguous())
        else:
            pb.fit_step(theta, r.to(dev).contiguous(), noise.to(dev).contiguous())
        for nb, c, p1 in zip(sizes, cases, singles):
            (p1.factorize if state == "factorize" else p1.fit_step)(c[3], c[1].to(dev), c[2].to(dev))
        for kind, bound in (("loo", 1), ("blocks", 64), ("random", 128)):
            G = torch.full((B, n), -1, dtype=torch.int64)
            per_site = []
            for b, nb in enumerate(sizes):
                g = folds(kind, nb, b)
                per_site.append(g)
                G[b, :nb] = torch.as_tensor(g)
            rb, vb, lb, ib = (t.cpu() for t in pb.cross_validate(G, max_group=bound))
            assert bool((ib == 0).all())
            for b, (nb, p1) in enumerate(zip(sizes, singles)):
                r1, v1, l1, i1 = (t.cpu() for t in p1.cross_validate(per_site[b], max_group=min(bound, nb)))
                k = l1.shape[0]
                same_factor = torch.equal(torch.tril(pb.buffer(_lib.BUF_T, site=b)[:nb, :nb]), torch.tril(p1.buffer(_lib.BUF_T)[:nb, :nb]))
                same_factor &= torch.equal(pb.buffer(_lib.BUF_ALPHA, site=b)[:nb], p1.buffer(_lib.BUF_ALPHA)[:nb])
                if same_factor:
                    bitwise.append((state, kind, b))
                    assert torch.equal(rb[b, :nb], r1) and torch.equal(vb[b, :nb], v1) and torch.equal(lb[b, :k], l1), (state, kind, b)
                else:
                    assert (rb[b, :nb] - r1).abs().max() <= 1e-11 * r1.abs().max(), (state, kind, b)
                    assert (vb[b, :nb] - v1).abs().max() <= 1e-11 * v1.abs().max(), (state, kind, b)
                    assert ((lb[b, :k] - l1).abs() <= 1e-11 * l1.abs().clamp(min=1.0)).all(), (state, kind, b)
                assert bool((rb[b, nb:] == 0).all()) and bool((vb[b, nb:] == 0).all()) and bool((lb[b, k:] == 0).all())
                # and against deletion
                Khat = orc.GRAMS[model](cases[b][0], cases[b][0], cases[b][3]) + torch.diag(cases[b][2])
                ref = dense_deletion_cv(Khat, cases[b][1], per_site[b])
                assert (rb[b, :nb] - ref[0]).abs().max() <= 1e-8 * ref[0].abs().max()
                assert (vb[b, :nb] - ref[1]).abs().max() <= 1e-8 * ref[1].abs().max()
    print(f"crossval batched: {len(bitwise)} of {2 * 3 * B} (state, scheme, site) comparisons were bitwise")


def test_edge_sizes(gpu_device):
    dev = gpu_device
    # n = 1: the held-out prediction of the only observation is the prior
    X, r, noise, theta = make_case("loadest", 2, 1, seed=3)
    r = torch.nan_to_num(r, nan=0.3)  # the generator standardises y: undefined for a single observation
    p = plan_for("loadest", 2, 1, X, torch.float64, dev)
    p.factorize(theta, r.to(dev), noise.to(dev))
    Khat = orc.GRAMS["loadest"](X, X, theta) + torch.diag(noise)
    resid, var, lpd, info = (t.cpu() for t in p.cross_validate(np.zeros(1, dtype=int)))
    ref = dense_deletion_cv(Khat, r, np.zeros(1, dtype=int))
    assert abs(resid[0] - r[0]) <= 1e-12 * abs(r[0]) and abs(var[0] - Khat[0, 0]) <= 1e-12 * Khat[0, 0]
    assert abs(lpd[0] - ref[2][0]) <= 1e-10 * max(1.0, abs(ref[2][0])) and int(info[0]) == 0
    # n = 129, one past the tile
    n = 129
    X, r, noise, theta = make_case("loadest", 3, n, seed=5, perturb=0.2)
    Khat = orc.GRAMS["loadest"](X, X, theta) + torch.diag(noise)
    p = plan_for("loadest", 3, n, X, torch.float64, dev)
    all_but_one = np.zeros(n, dtype=int)
    all_but_one[17] = 1
    unused_id = np.arange(n) * 5 // n
    unused_id[unused_id >= 2] += 1  # fold id 2 is never used
    unused_id[[0, 64, 128]] = -1    # and three observations are never held out
    whole = np.zeros(n, dtype=int)  # one fold holding everything: the prior itself
    cases = {"loo": np.arange(n), "all but one": all_but_one, "unused id": unused_id, "whole": whole}
    for state in ("factorize", "fit_step"):
        (p.factorize if state == "factorize" else p.fit_step)(theta, r.to(dev), noise.to(dev))
        for name, groups in cases.items():
            ref = dense_deletion_cv(Khat, r, groups)
            got = p.cross_validate(groups)
            e_r, e_v, e_l, info = _errors(got, ref)
            assert e_r < 1e-8 and e_v < 1e-8 and e_l < 1e-8 and bool((info == 0).all()), (state, name, e_r, e_v, e_l)
            again = p.cross_validate(groups)
            assert all(torch.equal(a, b) for a, b in zip(got, again)), (state, name)
            if name == "unused id":
                resid, var, lpd, _ = (t.cpu() for t in got)
                assert lpd.shape[0] == 6 and lpd[2] == 0.0
                assert bool((resid[[0, 64, 128]] == 0).all()) and bool((var[[0, 64, 128]] == 0).all())
    with pytest.raises(ValueError):
        p.cross_validate(np.full(n, -1))
    with pytest.raises(ValueError):
        p.cross_validate(np.arange(n + 1))
    fresh = plan_for("loadest", 3, n, X, torch.float64, dev)
    with pytest.raises(Exception, match="factorisation"):
        fresh.cross_validate(np.arange(n))


def test_engine_cross_validate_on_the_device(gpu_device):
    """``LoadestGP().fit`` on the GPU, then ``cross_validate("YE")`` against deletion on the CPU built from that model's own
    state: rtol 1e-7 in data space (the 1e-8 model-space bound through the exponential, with a decade of room)."""
    from discontinuum_amd.loadest_gp import LoadestGP
    from discontinuum_amd.validation import cv_folds
    from tests.helpers import loadest_dataset

    covariates, target = loadest_dataset(n=120, seed=3)
    model = LoadestGP()
    model.fit(covariates, target, iterations=10)
    ds = model.cross_validate("YE")
    groups, labels = cv_folds(target.coords["time"].values, "YE")
    assert ds.attrs["n_folds"] == len(labels) == 6
    mu, var, _covs = posterior_deletion_reference(model, groups)
    assert np.allclose(ds["predicted"].values, model.dm.y_t(mu).values, rtol=1e-7, atol=0)
    assert np.allclose(ds["se"].values, model.dm.error_pipeline.inverse_transform(var).values, rtol=1e-7, atol=0)
    loo = model.cross_validate("loo")
    mu, var, _covs = posterior_deletion_reference(model, np.arange(120))
    assert np.allclose(loo["predicted"].values, model.dm.y_t(mu).values, rtol=1e-7, atol=0)
    assert np.isfinite(model.flux_bias(cv=loo))
