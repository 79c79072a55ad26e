"""The leave-group-out training objective without a GPU: the closed-form gradient the device code implements against autograd,
central differences and brute-force deletion of every fold, its two end points (folds of one = leave-one-out, one fold of every
row = the marginal likelihood), the host paths (``fit(objective="lgo", folds=...)``, ``fit_many``, checkpoints, the refusals) on
the oracle-backed plan double of tests/lgo_helpers.py, and the four C entries' declarations and refusals before any launch."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib, multisite_fit
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.rating_gp import RatingGP
from discontinuum_amd.validation import cv_folds
from oracle import gp_oracle as orc
from tests.helpers import loadest_dataset, rating_dataset
from tests.lgo_helpers import LgoOraclePlan, brute_force_lgo, closed_form, lgo_from_khat, lgo_value_and_grads
from tests.loo_helpers import khat, loo_value_and_grads


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(LgoOraclePlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    monkeypatch.setattr(multisite_fit, "GPPlan", LgoOraclePlan)
    torch.manual_seed(0)


def _dense_case(n=37, seed=0):
    X, y = orc.synth_loadest(n, 3, seed)
    X, y = torch.tensor(X), torch.tensor(y)
    theta = torch.full((orc.loadest_ntheta(3),), 0.7, dtype=torch.float64) + 0.1 * torch.rand(
        orc.loadest_ntheta(3), dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    noise = 0.01 + 0.02 * torch.rand(n, dtype=torch.float64, generator=torch.Generator().manual_seed(seed + 1))
    return X, y, noise, theta


def _scattered(n, seed=0):
    """Five scattered folds of unequal size (ids 0, 1, 2, 4, 5: fold 3 is empty) and two rows in no fold."""
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    ids = torch.tensor([0, 1, 2, 4, 5, 0, 4])
    g = torch.empty(n, dtype=torch.int64)
    g[perm] = ids[torch.arange(n) % 7]
    g[perm[:2]] = -1
    return g


def test_closed_form_gradient_matches_autograd_and_central_differences():
    """dL/dK^ = 1/2 (M2 - b alpha^T - alpha b^T), dL/dr = b, dL/dnoise_i = 1/2 (M2)_ii - b_i alpha_i: the formulas of
    dgp_lgo.hip, at n = 37 with five scattered folds of unequal size and two rows in no fold.  Bounds: autograd differentiates the
    same fp64 expression (1e-10 of the largest entry); a central difference of step h = 1e-6 carries O(h^2) truncation plus
    eps / h rounding (1e-6 relative)."""
    X, r, noise, theta = _dense_case()
    groups = _scattered(37)
    Kh = khat("loadest", X, theta, noise).requires_grad_(True)
    rr = r.clone().requires_grad_(True)
    val = lgo_from_khat(Kh, rr, groups)
    gK, gr = torch.autograd.grad(val, (Kh, rr))
    gK = 0.5 * (gK + gK.T)
    v, M2, b, alpha = closed_form(Kh.detach(), r, groups)
    assert abs(v - val.detach()) <= 1e-13 * abs(v)
    G = 0.5 * (M2 - torch.outer(b, alpha) - torch.outer(alpha, b))
    assert (G - gK).abs().max() <= 1e-10 * gK.abs().max()
    assert (b - gr).abs().max() <= 1e-10 * gr.abs().max()
    # through the kernel, as the device contracts it: dL/dtheta_p = sum_ij G_ij dK_ij/dtheta_p; dL/dnoise = diag G
    _val, g_theta, g_r, g_noise = lgo_value_and_grads("loadest", X, r, noise, theta, groups)
    th = theta.clone().requires_grad_(True)
    K = orc.GRAMS["loadest"](X, X, th)
    (contr,) = torch.autograd.grad((K * G).sum(), th)
    assert (contr - g_theta).abs().max() <= 1e-10 * g_theta.abs().max()
    assert (torch.diagonal(G) - g_noise).abs().max() <= 1e-10 * g_noise.abs().max()
    assert (0.5 * torch.diagonal(M2) - b * alpha - g_noise).abs().max() <= 1e-10 * g_noise.abs().max()
    h = 1e-6
    f = lambda th_, r_, nz_: lgo_from_khat(khat("loadest", X, th_, nz_), r_, groups)  # noqa: E731
    for p in range(theta.numel()):
        e = torch.zeros_like(theta)
        e[p] = h
        fd = (f(theta + e, r, noise) - f(theta - e, r, noise)) / (2 * h)
        assert abs(fd - contr[p]) <= 1e-6 * max(1.0, contr.abs().max().item()), (p, fd, contr[p])
    unheld = int(torch.nonzero(groups < 0)[0])
    for i in (0, 7, 36, unheld):
        e = torch.zeros_like(r)
        e[i] = h
        fd = (f(theta, r + e, noise) - f(theta, r - e, noise)) / (2 * h)
        assert abs(fd - b[i]) <= 1e-6 * b.abs().max()
        fd = (f(theta, r, noise + e) - f(theta, r, noise - e)) / (2 * h)
        assert abs(fd - G[i, i]) <= 1e-6 * torch.diagonal(G).abs().max()


def test_restatement_matches_brute_force_deletion_of_every_fold():
    X, r, noise, theta = _dense_case(n=37, seed=3)
    Kh = khat("loadest", X, theta, noise)
    for groups in (_scattered(37, seed=1), torch.arange(37) // 10, torch.arange(37)):
        a, b = lgo_from_khat(Kh, r, groups), brute_force_lgo(Kh, r, groups)
        assert abs(a - b) <= 1e-11 * abs(b)


def test_the_two_end_points():
    """One fold of every row is the marginal likelihood (the oracle's NLL and gradient); folds of one are leave-one-out."""
    X, r, noise, theta = _dense_case(n=37, seed=2)
    val, g_theta, g_r, g_noise = lgo_value_and_grads("loadest", X, r, noise, theta, torch.zeros(37, dtype=torch.int64))
    th, rr, nz = (t.clone().requires_grad_(True) for t in (theta, r, noise))
    Kh = khat("loadest", X, th, nz)
    nll = 0.5 * rr @ torch.linalg.solve(Kh, rr) + 0.5 * torch.linalg.slogdet(Kh)[1] + 0.5 * 37 * np.log(2 * np.pi)
    ref = torch.autograd.grad(nll, (th, rr, nz))
    assert abs(val - nll.detach()) <= 1e-12 * abs(nll.detach())
    for a, b in zip((g_theta, g_r, g_noise), ref):
        assert (a - b).abs().max() <= 1e-9 * b.abs().max()
    plan = LgoOraclePlan("loadest", 37, 3)
    plan.set_inputs(X)
    plan.set_folds(torch.zeros(37, dtype=torch.int64))
    out = plan.lgo_fit_step(theta, r, noise)[0]
    fit = plan.fit_step(theta, r, noise)[0]
    assert abs(out[_lib.OUT_NLL] - fit[_lib.OUT_NLL]) <= 1e-12 * abs(fit[_lib.OUT_NLL])
    P = theta.numel()
    assert (out[_lib.OUT_DTHETA:_lib.OUT_DTHETA + P] - fit[_lib.OUT_DTHETA:_lib.OUT_DTHETA + P]).abs().max() <= 1e-9 * fit[
        _lib.OUT_DTHETA:_lib.OUT_DTHETA + P].abs().max()
    one = lgo_value_and_grads("loadest", X, r, noise, theta, torch.arange(37))
    loo = loo_value_and_grads("loadest", X, r, noise, theta)
    assert abs(one[0] - loo[0]) <= 1e-12 * abs(loo[0])
    for a, b in zip(one[1:], loo[1:]):
        assert (a - b).abs().max() <= 1e-9 * b.abs().max()


def _fit(family, objective, explicit, iterations, monkeypatch, n=45, **kw):
    monkeypatch.setattr(MarginalHIP, "explicit_host_algebra", explicit)
    torch.manual_seed(123)
    if family == "loadest":
        cov, tgt = loadest_dataset(n, seed=4)
        m = LoadestGP()
        args = dict(covariates=cov, target=tgt)
    else:
        cov, tgt, unc = rating_dataset(40, seed=4)
        m = RatingGP()
        args = dict(covariates=cov, target=tgt, target_unc=unc, monotonic_penalty_weight=0.5, grid_size=16)
    trace = []
    import tqdm

    real = tqdm.std.tqdm.set_postfix_str

    def spy(self, s="", refresh=True):
        trace.append(float(s.split("obj=")[1].split(",")[0]))
        return real(self, s, refresh)

    monkeypatch.setattr(tqdm.std.tqdm, "set_postfix_str", spy)
    if objective != "default":
        kw["objective"] = objective
    m.fit(iterations=iterations, learning_rate=0.1, scheduler=False, **args, **kw)
    return m, trace, args


def _explicit_ids(n):
    g = np.arange(n) % 3
    g[5] = -1
    return g


@pytest.mark.parametrize("folds", ["YE", 4, ("random", 3, 0), "explicit"])
def test_engine_fit_on_the_double_both_host_paths(folds, monkeypatch):
    """``fit(objective="lgo", folds=...)`` decreases its objective; the closed-form and the autograd host paths agree to 1e-12 over
    10 iterations (the same arithmetic in a different order); ``objective_folds_`` is what ``cv_folds`` gives on the times."""
    scheme = _explicit_ids(45) if folds == "explicit" else folds
    ma, ta, args = _fit("loadest", "lgo", True, 10, monkeypatch, folds=scheme)
    assert ma.objective_ == "lgo" and ma._plan.lgo_calls >= 10 and ma._plan.calls == 0 and ma._plan.loo_calls == 0
    assert ta[-1] < ta[0]
    expect = cv_folds(np.asarray(args["target"].coords["time"].values), scheme)[0]
    assert np.array_equal(ma.objective_folds_, expect)
    if folds == "explicit":
        assert ma.objective_folds_[5] == -1
    mb, _tb, _ = _fit("loadest", "lgo", False, 10, monkeypatch, folds=scheme)
    pa = torch.cat([p.detach().reshape(-1) for p in ma.model.parameters()])
    pb = torch.cat([p.detach().reshape(-1) for p in mb.model.parameters()])
    assert mb._plan.lgo_calls >= 10 and mb._plan.calls == 0
    assert (pa - pb).abs().max() <= 1e-12 * max(1.0, pb.abs().max().item()), (pa - pb).abs().max()


def test_rating_gp_with_learned_noise(monkeypatch):
    torch.manual_seed(5)  # the penalty grids of rating-gp draw from the global generator
    ma, ta, _ = _fit("rating", "lgo", True, 10, monkeypatch, folds=4)
    assert ma.objective_ == "lgo" and ma._plan.lgo_calls >= 10 and ta[-1] < ta[0]
    torch.manual_seed(5)
    mb, _tb, _ = _fit("rating", "lgo", False, 10, monkeypatch, folds=4)
    pa = torch.cat([p.detach().reshape(-1) for p in ma.model.parameters()])
    pb = torch.cat([p.detach().reshape(-1) for p in mb.model.parameters()])
    assert (pa - pb).abs().max() <= 1e-12 * max(1.0, pb.abs().max().item()), (pa - pb).abs().max()


def test_other_objectives_make_no_lgo_call_and_the_keyword_errors(monkeypatch):
    for objective in ("default", "mll", None, "loo"):
        for explicit in (True, False):
            m, _, _ = _fit("loadest", objective, explicit, 3, monkeypatch)
            assert m._plan.lgo_calls == 0 and m.objective_folds_ is None
            assert m.objective_ == ("loo" if objective == "loo" else "mll")
    cov, tgt = loadest_dataset(20)
    with pytest.raises(ValueError, match="folds"):
        LoadestGP().fit(cov, tgt, iterations=1, objective="lgo")
    for objective in ("mll", "loo", None):
        with pytest.raises(ValueError, match="folds"):
            LoadestGP().fit(cov, tgt, iterations=1, objective=objective, folds=4)
    with pytest.raises(ValueError, match="folds"):
        LoadestGP().fit(cov, tgt, iterations=1, folds="YE")
    with pytest.raises(ValueError, match="set_folds"):
        LgoOraclePlan("loadest", 20, 3).lgo_fit_step(None, None, None)


def test_checkpoint_round_trip():
    cov, tgt = loadest_dataset(30)
    m = LoadestGP()
    ids = _explicit_ids(30)
    m.fit(cov, tgt, iterations=3, objective="lgo", folds=ids)
    buf = io.BytesIO()
    m.save(buf)
    record = torch.load(io.BytesIO(buf.getvalue()), map_location="cpu", weights_only=True)
    assert record["objective"] == "lgo" and np.array_equal(record["objective_folds"].numpy(), ids)
    buf.seek(0)
    m2 = LoadestGP.load(buf, cov, tgt)
    assert m2.objective_ == "lgo" and np.array_equal(m2.objective_folds_, ids)
    assert torch.equal(m2._plan._folds, torch.as_tensor(ids))  # the restored plan holds them: the data term can be evaluated
    d = LoadestGP()
    torch.manual_seed(0)
    d.fit(cov, tgt, iterations=3)
    buf = io.BytesIO()
    d.save(buf)
    record = torch.load(io.BytesIO(buf.getvalue()), map_location="cpu", weights_only=True)
    assert "objective" not in record and "objective_folds" not in record  # a default fit's checkpoint is what it was
    buf.seek(0)
    assert LoadestGP.load(buf, cov, tgt).objective_folds_ is None
    loo = LoadestGP()
    loo.fit(cov, tgt, iterations=2, objective="loo")
    buf = io.BytesIO()
    loo.save(buf)
    assert "objective_folds" not in torch.load(io.BytesIO(buf.getvalue()), map_location="cpu", weights_only=True)


@pytest.mark.parametrize("closed_form", [True, False])
def test_fit_many_equals_single_fits(closed_form, monkeypatch):
    """Three ragged sites with per-site folds through ``fit_many(objective="lgo")`` against three single fits: the tolerance
    tests/test_loo_cpu.py uses for the same comparison -- parameters to 1e-9 after 6 iterations."""
    sizes = (31, 44, 27)
    data = [loadest_dataset(n, seed=10 + i) for i, n in enumerate(sizes)]
    schemes = [3, ("random", 4, 1), _explicit_ids(27)]
    singles = []
    for i, (cov, tgt) in enumerate(data):
        torch.manual_seed(i)
        m = LoadestGP()
        m.fit(cov, tgt, iterations=6, objective="lgo", folds=schemes[i])
        singles.append(m)
    many = [LoadestGP() for _ in sizes]
    objs, state = multisite_fit.fit_many(many, data, iterations=6, site_seeds=list(range(len(sizes))), objective="lgo", folds=schemes,
                                         closed_form=closed_form, return_state=True)
    assert bool(torch.isfinite(objs).all())
    assert tuple(state.folds.shape) == (3, 44) and int(state.folds[0, 31:].max()) == -1 and "folds" in state.as_dict()
    for a, b in zip(many, singles):
        assert a.objective_ == "lgo" and np.array_equal(a.objective_folds_, b.objective_folds_)
        pa = torch.cat([p.detach().reshape(-1) for _, p in sorted(a.model.named_parameters())])
        pb = torch.cat([p.detach().reshape(-1) for _, p in sorted(b.model.named_parameters())])
        assert (pa - pb).abs().max() <= 1e-9 * max(1.0, pb.abs().max().item()), (pa - pb).abs().max()
    # one scheme for every site; a resumed call takes the folds from the state
    same = [LoadestGP() for _ in sizes]
    _o, st = multisite_fit.fit_many(same, data, iterations=2, site_seeds=[0, 1, 2], objective="lgo", folds=3, closed_form=closed_form,
                                    return_state=True)
    assert all(np.array_equal(m.objective_folds_, cv_folds(np.asarray(d[1].coords["time"].values), 3)[0]) for m, d in zip(same, data))
    multisite_fit.fit_many(same, data, iterations=1, site_seeds=[0, 1, 2], objective="lgo", closed_form=closed_form, resume=st)
    assert all(m.objective_ == "lgo" and m.objective_folds_ is not None for m in same)
    dflt = [LoadestGP() for _ in sizes]
    _o, st0 = multisite_fit.fit_many(dflt, data, iterations=2, site_seeds=[0, 1, 2], closed_form=closed_form, return_state=True)
    assert all(m.objective_ == "mll" and m.objective_folds_ is None for m in dflt) and "folds" not in st0.as_dict()
    with pytest.raises(ValueError, match="folds"):
        multisite_fit.fit_many(dflt, data, iterations=1, objective="lgo")
    with pytest.raises(ValueError, match="folds"):
        multisite_fit.fit_many(dflt, data, iterations=1, objective="loo", folds=3)
    with pytest.raises(ValueError, match="one scheme per site"):
        multisite_fit.fit_many(dflt, data, iterations=1, objective="lgo", folds=[3, 3])


def test_censored_fits_are_refused():
    cov, tgt = loadest_dataset(30)
    mask = np.zeros(30, dtype=bool)
    mask[3] = True
    with pytest.raises(NotImplementedError, match='objective="lgo".*not samples'):
        LoadestGP().fit(cov, tgt, iterations=1, objective="lgo", folds=3, censored=mask)
    with pytest.raises(NotImplementedError, match='objective="lgo".*not samples'):
        multisite_fit.fit_many([LoadestGP(), LoadestGP()], [loadest_dataset(20, seed=1), loadest_dataset(25, seed=2)], iterations=1,
                               objective="lgo", folds=3, censored=[None, np.arange(25) == 4])
    m = LoadestGP()
    m.fit(cov, tgt, iterations=1, objective="lgo", folds=3, censored=np.zeros(30, dtype=bool))  # no censored row: the plain fit
    assert m.objective_ == "lgo"


# ------------------------------------------------------------------------------------------------ the C entries, no device
NAMES = ("dgp_lgo_workspace_bytes", "dgp_lgo_value_workspace_bytes", "dgp_lgo_fit_step", "dgp_lgo_value")


def test_abi_is_declared_bound_and_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    names = set(NAMES)
    assert names <= set(_lib.EXT2_SIGNATURES) and not names & set(_lib.SIGNATURES) and not names & set(_lib.EXT_SIGNATURES)
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    ext2 = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "dgp_hip_ext2.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(dgp_[a-z_0-9]+)\s*\(", ext2))
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "dgp_hip.h")).read(), flags=re.S)
    assert not names & set(re.findall(r"\b(dgp_[a-z_0-9]+)\s*\(", main))
    for name in names:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.EXT2_SIGNATURES[name][1] and fn.restype == _lib.EXT2_SIGNATURES[name][0]
    q, qv, f, v = (getattr(lib, name) for name in NAMES)
    one = C.c_void_p(256)  # never dereferenced: every call below returns before any launch
    th = (C.c_double * 8)()
    assert q(None, 2, 10) == 0 and qv(None, 2, 10) == 0
    assert f(None, th, one, one, one, one, 2, 10, one, 1 << 40, one, one, one, None) == -1 and b"null plan" in lib.dgp_last_error()
    assert v(None, one, one, 2, 10, one, 1 << 40, one, None) == -1 and b"null plan" in lib.dgp_last_error()
    n = 200
    h32 = C.c_void_p()
    assert lib.dgp_plan_create(_lib.MODEL_LOADEST, _lib.F32, n, 3, C.byref(h32)) == 0
    try:
        assert q(h32, 2, 100) == 0 and qv(h32, 2, 100) == 0
        assert f(h32, th, one, one, one, one, 2, 100, one, 1 << 40, one, one, one, None) == -1 and b"float64" in lib.dgp_last_error()
        assert v(h32, one, one, 2, 100, one, 1 << 40, one, None) == -1 and b"float64" in lib.dgp_last_error()
    finally:
        lib.dgp_plan_destroy(h32)
    for batch in (1, 3):
        h = C.c_void_p()
        assert lib.dgp_plan_create(_lib.MODEL_LOADEST, _lib.F64, n, 3, C.byref(h)) == 0
        try:
            if batch > 1:
                assert lib.dgp_plan_set_batch(h, batch) == 0
            N = 256
            for ng, mg in ((0, 10), (n + 1, 10), (2, 0), (2, n + 1), (-1, 10)):
                assert q(h, ng, mg) == 0 and qv(h, ng, mg) == 0
            # three N x N matrices per site; the blocks: N round_up(max_group, 128) doubles per site and one tile of rows
            assert q(h, 2, 100) > qv(h, 2, 100) > 0 and q(h, 2, 100) >= batch * 3 * N * N * 8
            assert q(h, 4, 1) < q(h, 4, 2) == q(h, 4, 64) < q(h, 4, 65)
            grow = q(h, 4, 129) - q(h, 4, 128) - (lib.dgp_cross_validate_workspace_bytes(h, 4, 129)
                                                  - lib.dgp_cross_validate_workspace_bytes(h, 4, 128))
            assert grow == 8 * 128 * (batch * N + 128)
            assert f(h, th, one, one, one, one, 2, 100, one, 1 << 40, one, one, one, None) == -3  # no plan workspace yet
            if batch > 1:
                continue  # (a batched plan's workspace call copies the site sizes to the device)
            assert lib.dgp_plan_set_workspace(h, C.c_void_p(1 << 20), lib.dgp_plan_workspace_bytes(h)) == 0  # never dereferenced
            need, needv = q(h, 2, 100), qv(h, 2, 100)
            ok = [h, th, one, one, one, one, 2, 100, one, need, one, None, None, None]
            okv = [h, one, one, 2, 100, one, needv, one, None]

            def call(fn, base, **kw):
                a = list(base)
                for i, val in kw.items():
                    a[int(i[1:])] = val
                return fn(*a)

            for i in (1, 2, 3, 4, 5, 10):  # theta, r, noise, order, start, out
                assert call(f, ok, **{f"a{i}": None}) == -1 and b"null" in lib.dgp_last_error(), i
            for i in (1, 2, 7):  # order, start, out2
                assert call(v, okv, **{f"a{i}": None}) == -1 and b"null" in lib.dgp_last_error(), i
            for ng, mg in ((0, 100), (n + 1, 100), (2, 0), (2, n + 1)):
                assert call(f, ok, a6=ng, a7=mg) == -1 and b"size" in lib.dgp_last_error()
                assert call(v, okv, a3=ng, a4=mg) == -1 and b"size" in lib.dgp_last_error()
            assert call(f, ok, a8=None) == -3 and call(f, ok, a9=need - 1) == -3 and b"workspace" in lib.dgp_last_error()
            assert call(v, okv, a5=None) == -3 and call(v, okv, a6=needv - 1) == -3
            assert call(f, ok, a8=C.c_void_p(264)) == -1 and b"aligned" in lib.dgp_last_error()
            assert call(v, okv, a5=C.c_void_p(264)) == -1 and b"aligned" in lib.dgp_last_error()
            assert call(f, ok) == -4 and b"dgp_set_inputs" in lib.dgp_last_error()  # DGP_E_STATE: no inputs
            assert call(v, okv) == -4 and b"K^^-1" in lib.dgp_last_error()  # DGP_E_STATE: no held inverse
        finally:
            lib.dgp_plan_destroy(h)
