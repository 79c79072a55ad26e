"""Censored observations in batched plans without a GPU: the C ABI of the batched entries (names, argument validation before any
launch) and the host side of ``fit_many(censored=...)`` -- both host paths, the hand-back, the refusals, the distributed fit --
over the oracle-backed batched double of tests/censored_batched_helpers.py."""
import ctypes as C
import io
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from discontinuum_amd import _lib
from discontinuum_amd.loadest_gp import LoadestGP
from tests.censored_batched_helpers import BatchedLaplaceOraclePlan
from tests.helpers import loadest_dataset, rating_dataset

LN2 = 0.6931471805599453
SIZES = (31, 44, 27)
NAMES = ("dgp_laplace_batched_workspace_bytes", "dgp_laplace_batched_fit_step", "dgp_laplace_batched_factorize")


def test_abi_declares_the_batched_censored_entries():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dgp_hip.h")).read()
    for name in NAMES + ("dgp_debug_bilinear_batched",):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header, name
    h64, h32 = C.c_void_p(), C.c_void_p()
    assert lib.dgp_plan_create(_lib.MODEL_LOADEST, _lib.F64, 100, 2, C.byref(h64)) == 0
    assert lib.dgp_plan_create(_lib.MODEL_LOADEST, _lib.F32, 100, 2, C.byref(h32)) == 0
    for h in (h64, h32):
        assert lib.dgp_plan_set_batch(h, 4) == 0
    one_site = C.c_void_p()
    assert lib.dgp_plan_create(_lib.MODEL_LOADEST, _lib.F64, 100, 2, C.byref(one_site)) == 0
    need1, need4 = lib.dgp_laplace_batched_workspace_bytes(one_site), lib.dgp_laplace_batched_workspace_bytes(h64)
    assert need1 == lib.dgp_laplace_workspace_bytes(one_site) and need4 > 3 * need1 and need4 > 4 * 13 * 100 * 8
    assert lib.dgp_laplace_batched_workspace_bytes(h32) == 0 and lib.dgp_laplace_batched_workspace_bytes(None) == 0
    # argument validation before any launch, without a device
    stat = (C.c_double * 16)()
    theta = (C.c_double * 36)(*([LN2] * 36))
    one = C.c_void_p(256)  # never dereferenced: every call below fails before a launch
    fit, fac = lib.dgp_laplace_batched_fit_step, lib.dgp_laplace_batched_factorize
    assert fit(h32, theta, one, one, one, one, one, 5, 1e-10, one, 1 << 24, one, one, stat, None) == -1
    assert b"float64" in lib.dgp_last_error()
    assert fit(h64, theta, one, one, one, one, None, 5, 1e-10, one, 1 << 24, one, one, stat, None) == -1
    assert b"f_dev" in lib.dgp_last_error()
    assert fac(h64, theta, one, one, one, one, one, 0, 1e-10, one, 1 << 24, one, stat, None) == -1
    assert fit(h64, theta, one, one, one, one, one, 5, 1e-10, one, 1 << 24, one, one, stat, None) == -3  # no workspace
    assert fac(h64, theta, one, one, one, one, one, 5, 1e-10, one, 1 << 24, one, stat, None) == -3
    # the single-site entries keep refusing a batched plan
    assert lib.dgp_laplace_factorize(h64, theta, one, one, one, one, one, 5, 1e-10, one, 1 << 24, one, stat, None) == -1
    assert b"batched" in lib.dgp_last_error()
    for h in (h64, h32, one_site):
        assert lib.dgp_plan_destroy(h) == 0


@pytest.fixture()
def cpu_engine(monkeypatch):
    from discontinuum_amd import multisite_fit

    monkeypatch.setattr(LoadestGP, "_plan_factory", staticmethod(BatchedLaplaceOraclePlan))
    monkeypatch.setattr(LoadestGP, "device", "cpu")
    monkeypatch.setattr(multisite_fit, "GPPlan", BatchedLaplaceOraclePlan)
    monkeypatch.setattr(BatchedLaplaceOraclePlan, "laplace_calls_total", 0)
    return LoadestGP


def _mask(target, k):
    """The k smallest values become non-detects reported at a common detection limit (k = 0: nothing censored)."""
    vals = np.asarray(target.values, dtype=np.float64)
    order = np.argsort(vals)
    mask = np.zeros(len(vals), dtype=bool)
    mask[order[:k]] = True
    reported = vals.copy()
    reported[mask] = vals[order[k]]
    return type(target)(reported, dims=target.dims, coords=target.coords, name=target.name, attrs=getattr(target, "attrs", {})), mask


def _sites(ks=(6, 0, 5), sizes=SIZES):
    """-> (datasets with the limits in place, masks); the site with k = 0 is uncensored (its mask is None)."""
    data, masks = [], []
    for i, (n, k) in enumerate(zip(sizes, ks)):
        cov, target = loadest_dataset(n, seed=10 + i)
        reported, mask = _mask(target, k)
        data.append((cov, reported))
        masks.append(mask if k else None)
    return data, masks


def _flat(m):
    return torch.cat([p.detach().reshape(-1).double() for _, p in sorted(m.model.named_parameters())]
                     + [p.detach().reshape(-1).double() for _, p in sorted(m.likelihood.named_parameters())])


def test_closed_form_and_autograd_paths_give_the_same_trajectory(cpu_engine):
    """The tolerance of ``test_fit_many_closed_form_follows_the_autograd_trajectory``: parameters 1e-12, objectives 1e-12 relative."""
    from discontinuum_amd import multisite_fit

    data, masks = _sites()
    seeds = list(range(len(SIZES)))
    ma = [cpu_engine() for _ in SIZES]
    oa = multisite_fit.fit_many(ma, data, iterations=6, site_seeds=seeds, censored=masks)
    assert multisite_fit.LAST_TIMING["closed_form"] and BatchedLaplaceOraclePlan.laplace_calls_total == 6
    mb = [cpu_engine() for _ in SIZES]
    ob = multisite_fit.fit_many(mb, data, iterations=6, site_seeds=seeds, censored=masks, closed_form=False)
    assert not multisite_fit.LAST_TIMING["closed_form"] and BatchedLaplaceOraclePlan.laplace_calls_total == 12
    diff = max(float((_flat(a) - _flat(b)).abs().max()) for a, b in zip(ma, mb))
    assert diff <= 1e-12, diff
    assert float(((oa - ob).abs() / ob.abs()).max()) <= 1e-12
    # ... and differs from the fit that takes the limits for samples
    mc = [cpu_engine() for _ in SIZES]
    multisite_fit.fit_many(mc, data, iterations=6, site_seeds=seeds)
    assert float((_flat(mc[0]) - _flat(ma[0])).abs().max()) > 1e-4
    assert float((_flat(mc[1]) - _flat(ma[1])).abs().max()) <= 1e-12  # the uncensored site's trajectory is its own


def test_fit_many_against_sequential_fits_and_the_hand_back(cpu_engine):
    from discontinuum_amd import multisite_fit

    data, masks = _sites()
    seeds = list(range(len(SIZES)))
    models = [cpu_engine() for _ in SIZES]
    multisite_fit.fit_many(models, data, iterations=8, site_seeds=seeds, censored=masks)
    for b, (m, (cov, reported), mask) in enumerate(zip(models, data, masks)):
        solo = cpu_engine()
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seeds[b])
            solo.fit(cov, reported, iterations=8, censored=mask)
        assert float((_flat(m) - _flat(solo)).abs().max()) <= 1e-6, b
        # hand-back: the side vector, the last status, and predictions from the model's own plan equal the solo fit's
        if mask is None:
            assert m._censor is None and m.laplace_status_ is None
        else:
            assert m._censor.side.tolist() == np.where(mask, -1, 0).tolist() and m._censor.f is not None
            it, dmax, _halvings, capped = m.laplace_status_
            assert 0 <= it <= 30 and dmax <= m.laplace_tol and capped == 0
        mu, se = m.predict(cov)
        mu1, se1 = solo.predict(cov)
        assert np.allclose(mu.values, mu1.values, rtol=1e-5, atol=0) and np.allclose(se.values, se1.values, rtol=1e-5, atol=0)
    # a checkpoint of a handed-back model round-trips the mask
    buf = io.BytesIO()
    models[0].save(buf)
    buf.seek(0)
    back = cpu_engine.load(buf, *data[0])
    assert back._censor is not None and back._censor.side.tolist() == np.where(masks[0], -1, 0).tolist()


def test_masks_without_a_censored_row_take_the_plain_path(cpu_engine):
    from discontinuum_amd import multisite_fit

    data, _ = _sites(ks=(0, 0, 0))
    seeds = list(range(len(SIZES)))
    fits = []
    for censored in (None, [None] * 3, [np.zeros(n, dtype=bool) for n in SIZES], [None, np.zeros(SIZES[1], dtype=int), None]):
        models = [cpu_engine() for _ in SIZES]
        multisite_fit.fit_many(models, data, iterations=4, site_seeds=seeds, censored=censored)
        assert all(m._censor is None and m.laplace_status_ is None for m in models)
        fits.append(torch.cat([_flat(m) for m in models]))
    assert BatchedLaplaceOraclePlan.laplace_calls_total == 0
    assert all(torch.equal(fits[0], f) for f in fits[1:])
    with pytest.raises(ValueError, match="one entry per site"):
        multisite_fit.fit_many([cpu_engine() for _ in SIZES], data, iterations=1, censored=[None])
    with pytest.raises(ValueError, match="align"):
        multisite_fit.fit_many([cpu_engine() for _ in SIZES], data, iterations=1, censored=[None, np.ones(3, dtype=bool), None])


def test_refusals(cpu_engine, monkeypatch):
    from discontinuum_amd import multisite_fit
    from discontinuum_amd.rating_gp import RatingGP

    data, masks = _sites()
    # rating-gp: a learned noise term has no gradient in a censored fit
    monkeypatch.setattr(RatingGP, "_plan_factory", staticmethod(BatchedLaplaceOraclePlan))
    monkeypatch.setattr(RatingGP, "device", "cpu")
    rdata = [rating_dataset(30, seed=i) for i in range(2)]
    rmask = np.zeros(30, dtype=bool)
    rmask[:4] = True
    with pytest.raises(NotImplementedError, match="censored"):
        multisite_fit.fit_many([RatingGP(), RatingGP()], rdata, iterations=1, censored=[rmask, None])
    # a learned-noise likelihood on a loadest model
    noisy = [cpu_engine() for _ in SIZES]
    real = multisite_fit._site_sides

    def with_learned_noise(models, *a):
        models[0].likelihood.second_noise_covar = object()
        try:
            return real(models, *a)
        finally:
            del models[0].likelihood.second_noise_covar

    monkeypatch.setattr(multisite_fit, "_site_sides", with_learned_noise)
    with pytest.raises(NotImplementedError, match="censored"):
        multisite_fit.fit_many(noisy, data, iterations=1, censored=masks)
    monkeypatch.setattr(multisite_fit, "_site_sides", real)
    # fp32 models
    monkeypatch.setattr(LoadestGP, "dtype", torch.float32)
    with pytest.raises(NotImplementedError, match="censored"):
        multisite_fit.fit_many([cpu_engine() for _ in SIZES], data, iterations=1, censored=masks)
    monkeypatch.setattr(LoadestGP, "dtype", torch.float64)
    assert BatchedLaplaceOraclePlan.laplace_calls_total == 0
    # the 4-entry record form still raises, in both entry points
    cov, reported = data[0]
    for fn in (multisite_fit.fit_many, multisite_fit.fit_many_distributed):
        with pytest.raises(NotImplementedError, match="censored="):
            fn([cpu_engine()], [(cov, reported, None, masks[0])])
    # hyperparameter_uncertainty_many refuses a censored model with the engine's own text
    models = [cpu_engine() for _ in SIZES]
    multisite_fit.fit_many(models, data, iterations=2, censored=masks)
    with pytest.raises(NotImplementedError, match="not available for a fit with censored observations"):
        multisite_fit.hyperparameter_uncertainty_many(models)


def test_predict_many_builds_the_laplace_cache(cpu_engine):
    from discontinuum_amd import multisite_fit

    data, masks = _sites()
    models = [cpu_engine() for _ in SIZES]
    multisite_fit.fit_many(models, data, iterations=4, site_seeds=[0, 1, 2], censored=masks)
    calls = BatchedLaplaceOraclePlan.laplace_calls_total
    got = multisite_fit.predict_many(models, [cov for cov, _ in data])
    assert BatchedLaplaceOraclePlan.laplace_calls_total == calls + 1  # ONE batched laplace_factorize
    for m, (cov, _), (mu, se) in zip(models, data, got):
        mu1, se1 = m.predict(cov)
        assert np.allclose(mu.values, mu1.values, rtol=1e-9, atol=0) and np.allclose(se.values, se1.values, rtol=1e-9, atol=0)


def test_one_site_and_a_resumed_run(cpu_engine):
    """One censored site through ``fit_many`` (the unbatched plan) lands where its solo fit lands; a run split by ``return_state``
    / ``resume`` cold-starts the modes and equals the uninterrupted run to the mode tolerance (the modes are not in the state)."""
    from discontinuum_amd import multisite_fit

    data, masks = _sites()
    one = [cpu_engine()]
    multisite_fit.fit_many(one, data[:1], iterations=5, censored=masks[:1])
    solo = cpu_engine()
    solo.fit(*data[0], iterations=5, censored=masks[0])
    assert float((_flat(one[0]) - _flat(solo)).abs().max()) <= 1e-6 and one[0].laplace_status_[1] <= one[0].laplace_tol
    whole = [cpu_engine() for _ in SIZES]
    multisite_fit.fit_many(whole, data, iterations=6, censored=masks)
    split = [cpu_engine() for _ in SIZES]
    _, state = multisite_fit.fit_many(split, data, iterations=3, censored=masks, return_state=True)
    assert set(state.as_dict()) == set(multisite_fit.FitManyState.FIELDS)  # unchanged: no modes in it
    multisite_fit.fit_many(split, data, iterations=3, censored=masks, resume=state)
    assert max(float((_flat(a) - _flat(b)).abs().max()) for a, b in zip(whole, split)) <= 1e-8


# ---- the distributed fit over a two-rank gloo group, in the pattern of tests/test_fit_many_gloo.py
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from discontinuum_amd import multisite_fit

        LoadestGP._plan_factory = staticmethod(BatchedLaplaceOraclePlan)
        LoadestGP.device = "cpu"
        multisite_fit.GPPlan = BatchedLaplaceOraclePlan
        data, masks = _sites()
        models = [LoadestGP() for _ in SIZES]
        objs, table = multisite_fit.fit_many_distributed(models, data, iterations=5, censored=masks)
        sides = [None if m._censor is None else m._censor.side.tolist() for m in models]
        other = 1 if rank == 0 else 0  # a site this rank did NOT train
        mu, _se = models[2 if other == 0 else 1].predict(data[2 if other == 0 else 1][0])
        q.put((rank, {"objs": objs.numpy(), "table": table.numpy(), "params": [_flat(m).numpy() for m in models], "sides": sides,
                      "pred": np.asarray(mu.values)}))
    finally:
        dist.destroy_process_group()


def test_two_ranks_match_the_single_process_fit(cpu_engine):
    from discontinuum_amd import multisite_fit

    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=600) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    torch.set_num_threads(2)
    data, masks = _sites()
    models = [cpu_engine() for _ in SIZES]
    objs = multisite_fit.fit_many(models, data, iterations=5, site_seeds=[0, 1, 2], censored=masks)
    expect = [None if mk is None else np.where(mk, -1, 0).tolist() for mk in masks]
    for rank in (0, 1):
        out = got[rank]
        # the warm start makes a site's trajectory depend on its own history alone: the same to the mode tolerance
        assert np.allclose(out["objs"], objs.numpy(), rtol=1e-8, atol=0)
        for i, m in enumerate(models):
            assert np.abs(out["params"][i] - _flat(m).numpy()).max() <= 1e-8, (rank, i)
        assert out["sides"] == expect  # also for the sites the rank loaded from the table
    assert np.array_equal(got[0]["table"], got[1]["table"])
    mu, _ = models[2].predict(data[2][0])  # rank 1 owns site 1 only: it predicted site 2 from the table + the censoring it set
    assert np.allclose(got[1]["pred"], np.asarray(mu.values), rtol=1e-6, atol=0)
