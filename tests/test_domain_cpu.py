"""The 40-digit fixtures of tests/golden/make_domain_pairs.py on their own (no GPU): they load, they are what the committed
script writes, their parameter order is the oracle's, and the bounds tests/test_gpu_domain.py applies to the device leave
the formulas themselves a factor of four (tests/domain_helpers.py, DESIGN.md "Parity across the hyperparameter domain")."""
import mpmath as mp
import numpy as np
import pytest
import torch

from oracle import gp_oracle as orc
from tests import domain_helpers as dh

CASES = dh.case_ids()
DTYPES = [np.float64, np.float32]


def test_every_corner_has_its_fixture():
    g = dh.generator()
    assert len(CASES) == 29 and len(set(CASES)) == 29
    for model, table in g.CORNERS.items():
        assert set(table) == {"centre", "short", "long", "mixed", "mixedp"} | ({"deep"} if model == "rating" else set())
        for corner, theta in table.items():
            assert np.array_equal(dh.load(f"{model}_{corner}")["theta"], np.asarray(theta, dtype=np.float64))
        for edge in g.EDGES:
            assert np.array_equal(dh.load(f"{model}_{edge}")["theta"], np.asarray(table["centre"], dtype=np.float64))


@pytest.mark.parametrize("case", CASES)
def test_fixture_shapes_are_consistent(case):
    g, fx = dh.generator(), dh.load(case)
    model, corner = dh.split_id(case)
    n, m, d = g.N, g.M, g.MODEL_D[model]
    P, Q = len(fx["theta"]), len(fx["slope_cols"])
    C = {"loadest2": 3, "loadest3": 3, "rating": 5, "composite": len(g.COMPOSITE_TERMS)}[model]
    assert (n, m) == (72, 20) and fx["X"].shape == (n, d) and fx["Xs"].shape == (m, d)
    assert fx["K_tril"].shape == (n * (n + 1) // 2,) and fx["Ks"].shape == (n, m) and fx["kss"].shape == (m,)
    assert fx["parts"].shape == (C, n, m) and fx["parts_kss"].shape == (C, m)
    assert list(fx["slope_cols"]) == g.slope_cols(model) and fx["dKs"].shape == (Q, n, m)
    assert fx["prior"].shape == ((1 + Q) * (2 + Q) // 2, m)
    for k in ("u", "alpha", "r"):
        assert fx[k].shape == (n,)
    for k in ("g_bil", "g_bil_scale", "g_nll", "g_nll_scale"):
        assert fx[k].shape == (P,) and np.isfinite(fx[k]).all()
    assert all(np.isfinite(v).all() for v in fx.values() if isinstance(v, np.ndarray))
    # one file serves both dtypes: everything a plan receives is representable in float32
    for k in ("X", "Xs", "u", "alpha", "r", "S"):
        assert np.array_equal(fx[k].astype(np.float32).astype(np.float64), fx[k]), k
    # the parts sum to the entry, the value plane of the prior block is k(x*, x*), the scales dominate the sums
    assert np.abs(fx["parts"].sum(0) - fx["Ks"]).max() <= 4e-16 * fx["sum_os"]
    assert np.abs(fx["parts_kss"].sum(0) - fx["kss"]).max() <= 4e-16 * fx["sum_os"]
    assert np.array_equal(fx["prior"][0], fx["kss"])
    assert (np.abs(fx["g_bil"]) <= fx["g_bil_scale"]).all() and (np.abs(fx["g_nll"]) <= fx["g_nll_scale"]).all()
    assert fx["sum_os"] == g.sum_os(model, fx["theta"])
    # the inputs are the committed script's draws, the edges are where the GPU tests look for them
    X, Xs = g.draw_inputs(model, corner)
    u, alpha, r, S = g.draw_weights(model, corner)
    for k, v in (("X", X), ("Xs", Xs), ("u", u), ("alpha", alpha), ("r", r), ("S", S)):
        assert np.array_equal(fx[k], v), k
    if corner in g.EDGES:
        assert np.array_equal(fx["X"][7], fx["X"][3]) and np.array_equal(fx["Xs"][2], fx["X"][5])
        assert np.all(fx["dKs"][:, 5, 2][[c for c in range(Q) if model != "rating" or c == 0]] == 0)
        assert (fx["X"][:, 0].min() > 1900) == (corner == "edge2000")
        if model == "rating":
            assert fx["X"][40, 1] == np.float32(1e-6) and fx["Xs"][6, 1] == np.float32(1e-6)


@pytest.mark.parametrize("case", CASES)
def test_committed_numbers_come_from_the_committed_script(case):
    """A seeded subsample of 50 stored numbers per fixture, evaluated again with mpmath: bit for bit."""
    g, fx = dh.generator(), dh.load(case)
    model, _ = dh.split_id(case)
    mp.mp.dps = g.DPS
    th = g.mpv(fx["theta"])
    X, Xs = [g.mpv(row) for row in fx["X"]], [g.mpv(row) for row in fx["Xs"]]
    rng = np.random.default_rng(g.hash_name("check" + case))
    n, m = g.N, g.M
    checked = 0
    for _ in range(25):
        i = int(rng.integers(0, n))
        j = int(rng.integers(0, i + 1))
        assert fx["K"][i, j] == float(g.entry(model, X[i], X[j], th))
        checked += 1
    for _ in range(5):
        i, j = int(rng.integers(0, n)), int(rng.integers(0, m))
        parts = g.entry_parts(model, X[i], Xs[j], th)
        assert fx["Ks"][i, j] == float(mp.fsum(parts))
        assert list(fx["parts"][:, i, j]) == [float(v) for v in parts]
        assert list(fx["dKs"][:, i, j]) == [float(g.entry_slope(model, X[i], Xs[j], th, c)) for c in fx["slope_cols"]]
        checked += 1 + len(parts) + len(fx["slope_cols"])
    j = int(rng.integers(0, m))
    B = g.prior_block(model, Xs[j], th)
    assert fx["kss"][j] == float(g.entry(model, Xs[j], Xs[j], th))
    assert list(fx["prior"][:, j]) == [float(B[a][b]) for a in range(len(B)) for b in range(a + 1)]
    checked += 1 + fx["prior"].shape[0]
    assert checked >= 50


@pytest.mark.parametrize("model", ["loadest2", "loadest3", "rating", "composite"])
def test_generator_and_oracle_agree_on_the_parameter_order(model):
    """At the centre the torch-fp64 oracle is a usable reference (away from it, it is not: DESIGN.md): 1e-15 of the sum of the
    outputscales pins the generator's parameter order -- and the composite's description -- to the oracle's."""
    g, fx = dh.generator(), dh.load(f"{model}_centre")
    gram = orc.composite_gram(g.COMPOSITE_SPEC) if model == "composite" else orc.GRAMS[dh.plan_model(model)[0]]
    X, Xs, theta = (torch.tensor(np.array(fx[k])) for k in ("X", "Xs", "theta"))
    err = max(np.abs(np.tril(gram(X, X, theta).numpy() - fx["K"])).max(), np.abs(gram(X, Xs, theta).numpy() - fx["Ks"]).max())
    print(f"{model} centre: oracle vs 40-digit reference {err / fx['sum_os']:.2e} of the sum of the outputscales")
    assert err <= 1e-15 * fx["sum_os"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", CASES)
def test_the_formulas_alone_hold_a_quarter_of_every_bound(case, dtype):
    """Plain numpy emulations of each model's pair formula and of its closed-form hyperparameter derivatives, at the plan's
    precision: the GPU tests' bounds are attainable, with room, at every corner."""
    fx = dh.load(case)
    model, _ = dh.split_id(case)
    K, dK = dh.emulate(model, fx["X"], fx["X"], fx["theta"], dtype, grad=True)
    Ks = dh.emulate(model, fx["X"], fx["Xs"], fx["theta"], dtype)
    e_val = max(np.abs(np.tril(K.astype(np.float64) - fx["K"])).max(), np.abs(Ks - fx["Ks"]).max()) / fx["sum_os"]
    g_bil, g_nll = dh.sweeps(dK, fx["u"], fx["alpha"], fx["S"], dtype)
    ok_bil, e_bil = dh.within(g_bil, fx["g_bil"], fx["g_bil_scale"], dh.SWEEP_BOUND[dtype] / 4)
    ok_nll, e_nll = dh.within(g_nll, fx["g_nll"], fx["g_nll_scale"], dh.SWEEP_BOUND[dtype] / 4)
    print(f"{case} {dtype.__name__}: values {e_val:.2e} of sum_os, bilinear {e_bil:.2e} and trace sweep {e_nll:.2e} of sum |term|")
    assert e_val <= dh.VALUE_BOUND[dtype] / 4
    assert ok_bil and ok_nll


def test_the_batched_sweeps_extra_sites():
    """The five extra sites of the batched bilinear sweep: distinct hyperparameters, from the corner fixtures' and from each
    other's; a seeded subsample against mpmath bit for bit is not needed -- the fp64 emulation of the formulas reproduces every
    stored sum to a quarter of the bound, which ties the file to the script's formulas."""
    g, fb = dh.generator(), dh.load_batch()
    thetas = [tuple(t) for t in fb["theta"]] + [tuple(g.CORNERS["loadest3"][c]) for c in ("centre", "short", "long", "mixed", "mixedp")]
    assert len(set(thetas)) == 10 and fb["X"].shape == (5, g.BATCH_N, 3)
    assert np.array_equal(fb["theta"], np.asarray(g.BATCH_EXTRA, dtype=np.float64))
    for b in range(5):
        _, dK = dh.emulate("loadest3", fb["X"][b], fb["X"][b], fb["theta"][b], np.float64, grad=True)
        got = np.einsum("i,pij,j->p", fb["u"][b], dK, fb["alpha"][b])
        ok, worst = dh.within(got, fb["g_bil"][b], fb["g_bil_scale"][b], dh.SWEEP_BOUND[np.float64] / 4)
        print(f"extra site {b}: bilinear {worst:.2e} of sum |term|")
        assert ok
