"""The per-pair evaluators of csrc/dgp_models.h across the hyperparameter domain, against the 40-digit fixtures of
tests/golden/make_domain_pairs.py: the corners (short / long / mixed lengthscales and outputscales, saturated and underflowing gates)
and two input-edge cases of loadest d = 2 and 3, rating and a composite tree with every factor kind, each through a float64
and a float32 plan.  Every other GPU parity test sits at ``init_raw()`` +- 0.3, where several lengthscales coincide.

a. values, no factorisation: ``stage_gram`` (with the identity pad) and ``cross_gram``, per entry of the sum of the
   outputscales: fp64 1e-13 (the bound of tests/test_gpu_stages.py, scaled), float32 5e-6.
b. derivative sweeps, no factorisation: ``bilinear`` (fp64) and ``stage_grad`` with the fixture's S and alpha written into
   the plan's buffers, per parameter of the stored sum |term|: fp64 1e-12, float32 1e-4; one batched plan of 10 sites (the
   hyperparameters travel through the device scratch), a different corner at every site.
c. products of a held factorisation with noise = 0.1 sum_os on every row (cond <= 1 + 10 n = 721, asserted): ``predict``,
   ``predict_terms``, ``predict_slopes`` with covariances, against numpy fp64 linear algebra on the fixture's matrices.
   fp64: means 1e-9 max(1, max |plane|), covariances 1e-8 x the two planes' prior standard deviations at the point (the
   fixture's prior block; for ``predict_terms`` each part's own k_c(x*, x*)); float32: 1e-3 of the same scales (SURVEY
   section 8d).  Where a scale is exactly 0 (a part the gate switches off) the entry must be exactly the reference's.

The derivations of the bounds and what the formulas alone measure against them (at most a quarter, tests/test_domain_cpu.py)
are in tests/domain_helpers.py and DESIGN.md, "Parity across the hyperparameter domain"."""
import functools

import numpy as np
import pytest
import torch

from tests import domain_helpers as dh

pytestmark = pytest.mark.gpu

CASES = dh.case_ids()
DTYPES = [(torch.float64, np.float64), (torch.float32, np.float32)]
DTYPE_IDS = ["fp64", "fp32"]
MEAN_BOUND = {np.float64: 1e-9, np.float32: 1e-3}
COV_BOUND = {np.float64: 1e-8, np.float32: 1e-3}


@functools.lru_cache(maxsize=None)
def model_name(model):
    if model == "composite":
        from tests import composite_helpers as comp

        return comp.define(dh.generator().COMPOSITE_SPEC)
    return dh.plan_model(model)[0]


def make_plan(case, tdt, dev, batch=1):
    from discontinuum_amd.backend import GPPlan

    fx = dh.load(case)
    model, _ = dh.split_id(case)
    p = GPPlan(model_name(model), fx["X"].shape[0], fx["X"].shape[1], dtype=tdt, device=dev, batch=batch)
    if batch == 1:
        p.set_inputs(torch.tensor(np.array(fx["X"])).to(dev, tdt).contiguous())
    return p, fx


def to_dev(a, tdt, dev):
    return torch.tensor(np.array(a, dtype=np.float64)).to(dev, tdt).contiguous()


@pytest.mark.parametrize("tdt,ndt", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", CASES)
def test_values(case, tdt, ndt, gpu_device):
    from discontinuum_amd import _lib

    dev = gpu_device
    p, fx = make_plan(case, tdt, dev)
    n, m, scale = fx["X"].shape[0], fx["Xs"].shape[0], fx["sum_os"]
    rng = np.random.default_rng(3)
    noise = (rng.uniform(0.05, 0.15, n) * scale).astype(np.float32).astype(np.float64)
    p.stage_gram(fx["theta"], to_dev(noise, tdt, dev))
    A = p.buffer(_lib.BUF_A)
    got = torch.tril(A[:n, :n]).cpu().double().numpy()
    e_gram = np.abs(got - np.tril(fx["K"] + np.diag(noise))).max() / scale
    Ks = p.cross_gram(fx["theta"], to_dev(fx["Xs"], tdt, dev)).cpu().double().numpy()
    e_cross = np.abs(Ks - fx["Ks"]).max() / scale
    print(f"{case} {ndt.__name__}: gram {e_gram:.2e}, cross {e_cross:.2e} of sum_os")
    assert Ks.shape == (n, m)
    assert e_gram <= dh.VALUE_BOUND[ndt] and e_cross <= dh.VALUE_BOUND[ndt]
    N = p.N
    assert N > n  # the identity pad, as tests/test_gpu_stages.py checks it
    pad = A[n:, :].cpu()
    assert torch.equal(torch.tril(pad[:, n:]), torch.eye(N - n, dtype=tdt))
    assert pad[:, :n].abs().max() == 0


@pytest.mark.parametrize("tdt,ndt", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", CASES)
def test_derivative_sweeps(case, tdt, ndt, gpu_device):
    from discontinuum_amd import _lib

    dev = gpu_device
    p, fx = make_plan(case, tdt, dev)
    n = fx["X"].shape[0]
    noise = torch.full((n,), 0.1 * fx["sum_os"], dtype=tdt, device=dev)
    p.stage_gram(fx["theta"], noise)
    # dgp_stage_grad reads exactly these two buffers and the inputs
    S, alpha = p.buffer(_lib.BUF_S), p.buffer(_lib.BUF_ALPHA)
    S.zero_()
    alpha.zero_()
    S[:n, :n] = to_dev(fx["S"], tdt, dev)
    alpha[:n] = to_dev(fx["alpha"], tdt, dev)
    g = p.stage_grad(fx["theta"]).cpu().double().numpy()
    ok, e_nll = dh.within(g, fx["g_nll"], fx["g_nll_scale"], dh.SWEEP_BOUND[ndt])
    print(f"{case} {ndt.__name__}: trace sweep {e_nll:.2e} of sum |term|")
    assert ok, (g, fx["g_nll"], fx["g_nll_scale"])
    if ndt is np.float64:
        gb = p.bilinear(fx["theta"], to_dev(fx["u"], tdt, dev), to_dev(fx["alpha"], tdt, dev)).cpu().numpy()
        ok, e_bil = dh.within(gb, fx["g_bil"], fx["g_bil_scale"], dh.SWEEP_BOUND[ndt])
        print(f"{case}: bilinear sweep {e_bil:.2e} of sum |term|")
        assert ok, (gb, fx["g_bil"], fx["g_bil_scale"])


def test_batched_bilinear_a_different_corner_at_every_site(gpu_device):
    """Ten loadest d = 3 sites in one plan -- more than 8, so the hyperparameters travel through the device scratch slots --
    and no two with the same hyperparameters: sites 0 .. 4 are the five corner fixtures (n = 72), sites 5 .. 9 the extra
    sites of domain_loadest3_batch.npz (n = 24, a ragged batch; the unused rows are NaN).  Each site is checked on its own."""
    dev = gpu_device
    corners = [dh.load(f"loadest3_{c}") for c in ("centre", "short", "long", "mixed", "mixedp")]
    fb = dh.load_batch()
    sites = [(fx["X"], fx["theta"], fx["u"], fx["alpha"], fx["g_bil"], fx["g_bil_scale"]) for fx in corners]
    sites += [tuple(fb[k][b] for k in ("X", "theta", "u", "alpha", "g_bil", "g_bil_scale")) for b in range(fb["theta"].shape[0])]
    B, n = len(sites), corners[0]["X"].shape[0]
    assert B == 10 and len({tuple(s[1]) for s in sites}) == B
    p, _ = make_plan("loadest3_centre", torch.float64, dev, batch=B)
    p.set_site_sizes([s[0].shape[0] for s in sites])
    X = torch.full((B, n, 3), float("nan"), dtype=torch.float64)
    u, a = (torch.full((B, n), float("nan"), dtype=torch.float64) for _ in range(2))
    for b, s in enumerate(sites):
        nb = s[0].shape[0]
        X[b, :nb], u[b, :nb], a[b, :nb] = (torch.tensor(np.array(v)) for v in (s[0], s[2], s[3]))
    p.set_inputs(X.to(dev).contiguous())
    theta = torch.stack([torch.tensor(np.array(s[1])) for s in sites])
    got = p.bilinear(theta, u.to(dev).contiguous(), a.to(dev).contiguous()).cpu().numpy()
    assert got.shape == (B, p.ntheta)
    for b, s in enumerate(sites):
        ok, err = dh.within(got[b], s[4], s[5], dh.SWEEP_BOUND[np.float64])
        print(f"site {b}: bilinear sweep {err:.2e} of sum |term|")
        assert ok, (b, got[b], s[4])


def reference_products(fx, r, ndt):
    """numpy fp64 linear algebra on the fixture's matrices -> per product (means (planes, m), covariances (planes, planes,
    m), prior standard deviations (planes, m))."""
    n = fx["K"].shape[0]
    noise = ndt(dh.NOISE_FRACTION * fx["sum_os"]).astype(np.float64)
    Khat = fx["K"] + noise * np.eye(n)
    assert np.linalg.cond(Khat) <= 1 + n / dh.NOISE_FRACTION
    L = np.linalg.cholesky(Khat)
    alpha = np.linalg.solve(Khat, r)
    prior = dh.unpack_prior(fx["prior"])
    C = fx["parts"].shape[0]

    def posterior(planes, prior_block):
        V = [np.linalg.solve(L, K) for K in planes]
        mean = np.stack([K.T @ alpha for K in planes])
        cov = np.stack([np.stack([prior_block[a][b] - (V[a] * V[b]).sum(0) for b in range(len(planes))]) for a in range(len(planes))])
        return mean, cov

    zero = np.zeros_like(fx["kss"])
    return {
        "predict": posterior([fx["Ks"]], [[fx["kss"]]]) + (np.sqrt(prior[0, 0])[None],),
        # every part against its OWN prior standard deviation at the point (a part that is switched off must come back 0)
        "terms": posterior(list(fx["parts"]), [[fx["parts_kss"][c] if c == e else zero for e in range(C)] for c in range(C)])
        + (np.sqrt(fx["parts_kss"]),),
        "slopes": posterior([fx["Ks"], *fx["dKs"]], prior) + (np.sqrt(np.stack([prior[a, a] for a in range(prior.shape[0])])),),
    }


def packed(cov):
    return np.stack([cov[a, b] for a in range(cov.shape[0]) for b in range(a + 1)])


def check_product(what, mean, cov, ref, ndt):
    ref_mean, ref_cov, sd = ref
    mean, cov = mean.cpu().double().numpy().reshape(ref_mean.shape), cov.cpu().double().numpy()
    cov = cov.reshape(-1, cov.shape[-1])
    e_mean = max(np.abs(mean[a] - ref_mean[a]).max() / max(1.0, np.abs(ref_mean[a]).max()) for a in range(len(ref_mean)))
    P = len(ref_mean)
    scale = np.stack([sd[a] * sd[b] for a in range(P) for b in range(a + 1)])
    ok, e_cov = dh.within(cov, packed(ref_cov), scale, COV_BOUND[ndt])
    print(f"{what}: mean {e_mean:.2e} of max(1, max |plane|), covariance {e_cov:.2e} of the prior standard deviations")
    assert e_mean <= MEAN_BOUND[ndt] and ok, (what, e_mean, e_cov)


@pytest.mark.parametrize("tdt,ndt", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("case", CASES)
def test_products_of_a_held_factorisation(case, tdt, ndt, gpu_device):
    from discontinuum_amd import _lib

    dev = gpu_device
    p, fx = make_plan(case, tdt, dev)
    model, corner = dh.split_id(case)
    n = fx["X"].shape[0]
    theta, Xs, cols = fx["theta"], to_dev(fx["Xs"], tdt, dev), [int(c) for c in fx["slope_cols"]]
    noise = torch.full((n,), dh.NOISE_FRACTION * fx["sum_os"], dtype=tdt, device=dev)
    r = (fx["r"] * np.sqrt(fx["sum_os"])).astype(ndt).astype(np.float64)
    out = p.factorize(theta, to_dev(r, tdt, dev), noise).cpu()
    assert int(out[_lib.OUT_INFO]) == 0
    ref = reference_products(fx, r, ndt)
    mean, var = p.predict(theta, Xs)
    check_product(f"{case} {ndt.__name__} predict", mean, var, ref["predict"], ndt)
    check_product(f"{case} {ndt.__name__} predict_terms", *p.predict_terms(theta, Xs, return_cov=True), ref["terms"], ndt)
    check_product(f"{case} {ndt.__name__} predict_slopes", *p.predict_slopes(theta, Xs, cols, return_cov=True), ref["slopes"], ndt)
    if corner in dh.generator().EDGES:
        # test point 2 IS train point 5.  With r = K^ e_5 the weights are alpha = e_5, and the posterior mean slope there is
        # the derivative of ONE cross entry at coincident points: exactly 0 in every stationary part (all columns of loadest
        # and the composite, the time column of rating), which a quotient by the distance would turn into 0 / 0
        r5 = (fx["K"][:, 5] + np.eye(n)[5] * float(ndt(dh.NOISE_FRACTION * fx["sum_os"]))).astype(ndt).astype(np.float64)
        assert int(p.factorize(theta, to_dev(r5, tdt, dev), noise).cpu()[_lib.OUT_INFO]) == 0
        ref5 = reference_products(fx, r5, ndt)["slopes"]
        smean, scov = p.predict_slopes(theta, Xs, cols, return_cov=True)
        check_product(f"{case} {ndt.__name__} slopes at the coincident pair", smean, scov, ref5, ndt)
        smean = smean.cpu().double().numpy()
        for q in range(len(cols)):
            if model != "rating" or cols[q] == 0:
                assert fx["dKs"][q, 5, 2] == 0
                assert abs(smean[1 + q, 2]) <= MEAN_BOUND[ndt] * max(1.0, np.abs(ref5[0][1 + q]).max()), (q, smean[1 + q, 2])
