"""The host side of the generic composite evaluator, without a GPU: the seeded trees of tests/composite_helpers.py are well
conditioned and cover what they promise, ``dgp_composite_define`` refuses malformed descriptions (-2), reuses the id of an
identical one and reports a full registry (-5, in a child process, so that this suite's own registry is not filled), and the
lowering's description / parameter order reproduces a direct evaluation of the ``gp.kernels`` tree."""
import json
import subprocess
import sys

import numpy as np
import torch

from discontinuum_amd import _lib
from oracle import gp_oracle as orc
from tests import composite_helpers as H

E_MODEL, E_FULL = -2, -5


def test_cases_are_well_conditioned_and_cover_what_they_promise():
    """cond(K^) <= 1e6 and a finite oracle gradient for every case at n = 300, plain and with the edge rows (a duplicated
    row, two points one period apart).  Bound: lambda_max(K) <= n sum_t sigma_t^2 <= 300 x 12 and lambda_min(K^) >= the
    noise 0.05, so cond <= 7.2e4 for ANY draw; 1e6 leaves the fp64 bounds of the GPU sweep their usual room."""
    assert len(H.CASES) == 28 and len(H.RANDOM) == H.N_RANDOM == 20 and len(H.HAND_BUILT) == 8
    assert len({c.spec for c in H.CASES}) == len(H.CASES) <= 28  # distinct structures
    assert H.DROPPED == 5  # draws with more than 24 parameters, dropped at generation
    worst, checked = 0.0, 0
    for i, case in enumerate(H.CASES):
        assert case.theta.numel() == case.ntheta <= H.MAX_THETA
        name = H.define(case.spec)
        for edge in (False, True):
            X, r, noise = H.data(i, 300, edge)
            if edge:
                assert torch.equal(X[7], X[3])
                per = H.first_period(case)
                if per is not None:
                    assert abs(float(X[9, per[1]] - X[5, per[1]]) - per[0]) < 1e-14
            Khat = H.gram_of(case)(X, X, case.theta) + torch.diag(noise)
            cond = float(torch.linalg.cond(Khat))
            worst = max(worst, cond)
            assert cond <= 1e6, (case.name, edge, cond)
            val, g_theta, g_r, g_noise = orc.nll_data_and_grads(name, X, r, noise, case.theta)
            assert all(bool(torch.isfinite(t).all()) for t in (val, g_theta, g_r, g_noise)), (case.name, edge)
            checked += 1
    assert checked == 2 * len(H.CASES)  # no case is skipped
    print(f"composite cases: worst cond(K^) {worst:.2e} over {checked} data sets, {H.DROPPED} draws dropped")
    # the coverage the list promises
    factors = [f for c in H.CASES for _s, fs in c.terms for f in fs]
    assert {f[0] for f in factors} == {H.RBF, H.MATERN, H.PERIODIC}
    assert {f[1] for f in factors if f[0] == H.MATERN} == {1, 3, 5}
    assert any(f[2] for f in factors) and any(not f[2] and len(f[3]) > 1 for f in factors)  # ARD and shared lengthscales
    assert {bool(s) for c in H.CASES for s, _fs in c.terms} == {True, False}
    assert {c.d for c in H.CASES} == {1, 2, 3, 4, 5, 6}
    assert max(len(c.terms) for c in H.CASES) == 6 and max(c.ntheta for c in H.CASES) == 24
    big = H.CASES[H.BIGGEST]
    assert big.hand_built and len(big.terms) == 6 and all(len(fs) == 3 for _s, fs in big.terms) and big.ntheta == 24
    assert any(c.ntheta == 1 and c.d == 6 and not c.terms[0][0] for c in H.CASES)
    assert any(len(c.terms) > 1 and not any(s for s, _fs in c.terms) for c in H.CASES)  # every term unscaled
    for kind in ((H.RBF, 0), (H.MATERN, 1), (H.MATERN, 3), (H.MATERN, 5), (H.PERIODIC, 0)):  # every kind alone at d = 1
        alone = [c for c in H.CASES if c.d == 1 and len(c.terms) == 1 and c.terms[0][0] and [f[:2] for f in c.terms[0][1]] == [kind]]
        assert len(alone) == 1 and (alone[0].hand_built or kind == (H.MATERN, 3)), kind  # Matern 3/2 alone: a random draw
    shared = [c for c in H.CASES if c.hand_built and {(H.PERIODIC, 0), (H.MATERN, 1), (H.RBF, 0)} <=
              {(f[0], f[1]) for _s, fs in c.terms for f in fs if 0 in f[3]}]
    assert shared  # one column under a Periodic, a Matern-1/2 and an (ARD) RBF factor


def _rbf_tree(d=2, nterms=1, nfac=1):
    return H.build_spec(d, [(True, [(H.RBF, 0, False, (0,))] * nfac)] * nterms)


MALFORMED = {
    "truncated": _rbf_tree()[:-1],
    "truncated inside a term": _rbf_tree()[:3],
    "trailing ints": _rbf_tree() + [0],
    "d = 0": [0, 1, 1, 1, 0, 0, 0, 1, 0],
    "d = 7": [7, 1, 1, 1, 0, 0, 0, 1, 0],
    "0 terms": [2, 0],
    "7 terms": _rbf_tree(nterms=7),
    "0 factors": [2, 1, 1, 0],
    "4 factors": _rbf_tree(nfac=4),
    "unknown type": [2, 1, 1, 1, 3, 0, 0, 1, 0],
    "negative type": [2, 1, 1, 1, -1, 0, 0, 1, 0],
    "Matern with 2 nu = 2": [2, 1, 1, 1, 1, 2, 0, 1, 0],
    "Periodic on two columns": [2, 1, 1, 1, 2, 0, 0, 2, 0, 1],
    "column = d": [2, 1, 1, 1, 0, 0, 0, 1, 2],
    "negative column": [2, 1, 1, 1, 0, 0, 0, 1, -1],
    "more columns than d": [2, 1, 1, 1, 0, 0, 0, 3, 0, 1, 1],
    # 6 scaled terms x 3 one-lengthscale factors = 24 parameters, and one ARD lengthscale more
    "25 parameters": H.build_spec(2, [(True, [(H.RBF, 0, False, (0,))] * 3)] * 5
                                  + [(True, [(H.RBF, 0, False, (0,))] * 2 + [(H.RBF, 0, True, (0, 1))])]),
}


def test_define_refuses_malformed_descriptions():
    lib = _lib.load()
    assert H.ntheta(MALFORMED["25 parameters"]) == 25  # (24 are accepted: the 6 x 3 tree of CASES)
    for what, spec in MALFORMED.items():
        rc, mid = H.define_raw(spec)
        assert rc == E_MODEL and mid == -1, (what, rc, mid)  # refused, the id is left alone
        assert b"malformed" in lib.dgp_last_error(), what


def test_define_reuses_ids_and_answers_the_size_queries():
    lib = _lib.load()
    ids = []
    for case in H.CASES:
        rc, mid = H.define_raw(case.spec)
        again = H.define_raw(case.spec)
        assert rc == 0 and again == (0, mid), case.name  # the same description twice: the same id
        assert lib.dgp_model_ntheta(mid, case.d) == case.ntheta and lib.dgp_model_nterms(mid, case.d) == len(case.terms)
        for wrong in {1, 2, 3, 4, 5, 6, 7} - {case.d}:
            assert lib.dgp_model_ntheta(mid, wrong) == -1 and lib.dgp_model_nterms(mid, wrong) == -1, (case.name, wrong)
        allowed = H.differentiable_columns(case.spec)
        for col in range(case.d):
            assert lib.dgp_model_input_differentiable(mid, case.d, col) == int(col in allowed), (case.name, col)
        assert lib.dgp_model_input_differentiable(mid, case.d, case.d) == -1
        ids.append(mid)
    assert len(set(ids)) == len(H.CASES)  # distinct structures, distinct ids
    # ids are slots counted from COMPOSITE_BASE: with every case registered, whatever else this process registered before,
    # the registry (64 per process) is within the budget -- H.define asserts the same on every call of the GPU sweep
    assert H.COMPOSITE_BASE <= min(ids) and max(ids) - H.COMPOSITE_BASE < H.REGISTRY_BUDGET, (min(ids), max(ids))
    assert lib.dgp_model_ntheta(max(ids) + 1000, 2) == -1 and lib.dgp_model_nterms(15, 2) == -1


# registers distinct valid structures through ctypes alone (no torch, no package import) until the call fails
_FILL = r"""
import ctypes as C, json, sys
lib = C.CDLL(sys.argv[1])
lib.dgp_composite_define.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
lib.dgp_model_ntheta.argtypes = [C.c_int, C.c_int]
lib.dgp_last_error.restype = C.c_char_p
codes, ids = [], []
specs = [[d, 1, scaled, 1, kind, nu2, 0, 1, col] for d in range(1, 7) for col in range(d) for scaled in (0, 1)
         for kind, nu2 in ((0, 0), (1, 1), (1, 3), (1, 5))]
for spec in specs[:70]:
    arr, mid = (C.c_int * len(spec))(*spec), C.c_int(-1)
    codes.append(lib.dgp_composite_define(arr, len(spec), C.byref(mid)))
    ids.append(mid.value)
    if codes[-1] != 0:
        break
first = specs[0]
arr, mid = (C.c_int * len(first))(*first), C.c_int(-1)
again = lib.dgp_composite_define(arr, len(first), C.byref(mid))  # an identical description needs no slot
print(json.dumps({"codes": codes, "ids": ids, "message": lib.dgp_last_error().decode(), "again": [again, mid.value],
                  "ntheta": [lib.dgp_model_ntheta(i, s[0]) for i, s in zip(ids[:-1], specs)],
                  "expected": [1 + s[2] for s in specs[:len(ids) - 1]]}))
"""


def test_registry_full_is_reported_in_a_child_process():
    run = subprocess.run([sys.executable, "-c", _FILL, _lib.LIB_PATH], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    out = json.loads(run.stdout.strip().splitlines()[-1])
    assert out["codes"] == [0] * 64 + [E_FULL], out["codes"]  # the 65th distinct structure is the first refused
    assert out["ids"] == list(range(H.COMPOSITE_BASE, H.COMPOSITE_BASE + 64)) + [-1]  # slots in order from the base
    assert "full" in out["message"]
    assert out["again"] == [0, out["ids"][0]]
    assert out["ntheta"] == out["expected"]  # the ids registered earlier still answer


def test_lowering_against_a_direct_walk_of_the_kernel_tree():
    """Ten random ``gp.kernels`` trees (built from the first ten random descriptions): the Gram of the lowering's description
    at the lowering's parameter vector against ``tree_gram``, which never sees either; 1e-14."""
    from discontinuum_amd.gp.lowering import composite_spec, lower

    worst = 0.0
    for i in H.RANDOM[:10]:
        case = H.CASES[i]
        cov = H.tree_from_spec(case.spec, case.theta)
        spec, _parts = composite_spec(cov, case.d)
        assert tuple(spec) == case.spec, case.name
        model, theta_fn = lower(cov, case.d)
        assert model == H.define(case.spec)  # the structure CASES registered: no new slot
        theta = theta_fn().detach()
        assert theta.shape == case.theta.shape and float((theta - case.theta).abs().max()) < 1e-12
        rng = np.random.default_rng(i)
        X1, X2 = H.points(rng, 40, case.d), H.points(rng, 30, case.d)
        err = float((orc.composite_gram(spec)(X1, X2, theta) - H.tree_gram(cov)(X1, X2)).abs().max())
        worst = max(worst, err)
        assert err <= 1e-14, (case.name, err)
    print(f"lowering against the tree walk: worst Gram difference {worst:.2e}")
