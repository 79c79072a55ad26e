"""The leave-group-out training objective on the device (``dgp_lgo_fit_step`` / ``dgp_lgo_value``) against its dense restatement
(tests/lgo_helpers.py: torch fp64 on the oracle's Gram matrix, gradients by autograd).  The bounds are the ones
tests/test_gpu_loo.py takes from tests/test_gpu_stages.py: value relative 1e-10, dtheta 1e-8 of its max-norm, dr / dnoise
relative 1e-8, the reduced slots 1e-8 of their absolute sums.  The fold layouts hit every route of the fold blocks: folds of
one (the column scaling), up to 64 rows (the LDS route, 64 x 64 tiles), 65 and more (the block route, 128 x 128 tiles)."""
import ctypes as C

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from tests import composite_helpers as ch
from tests.lgo_helpers import LgoOraclePlan, lgo_value_and_grads
from tests.test_gpu_loo import _case, _weights
from tests.test_gpu_stages import plan_for

pytestmark = pytest.mark.gpu


def folds_for(layout, n, seed=0):
    """Fold ids (n,) int64 of a named layout."""
    if layout == "ones":
        return torch.arange(n)
    if layout == "all":
        return torch.zeros(n, dtype=torch.int64)
    if layout == "scattered":  # 5 scattered folds of unequal size, two rows in no fold, fold 3 of the 6 ids EMPTY
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(100 + seed))
        ids = torch.tensor([0, 1, 2, 4, 5, 0, 1, 2, 4])  # (the largest fold holds 2 / 9 of the rows: 58 of 257, the LDS route)
        g = torch.empty(n, dtype=torch.int64)
        g[perm] = ids[torch.arange(n) % 9]
        g[perm[:2]] = -1
        return g
    if layout == "blocks65":  # contiguous folds of 65: just over the LDS route
        return torch.arange(n) // 65
    if layout == "halves":  # 129 / 128 at n = 257: crosses a 128 block
        return (torch.arange(n) >= (n + 1) // 2).to(torch.int64)
    raise ValueError(layout)


LAYOUTS = [(2, "ones"), (2, "all"), (127, "ones"), (127, "scattered"), (130, "ones"), (130, "scattered"), (130, "blocks65"),
           (130, "all"), (257, "ones"), (257, "scattered"), (257, "halves")]
PLAN_CASES = [(m, d, n, lay) for m, d in (("loadest", 2), ("loadest", 3), ("rating", 2)) for n, lay in LAYOUTS]


def _errors(ref, w, out, dr, dnoise, P, n):
    val, g_theta, g_r, g_noise = ref
    out, dr, dnoise = out.cpu(), dr.cpu(), dnoise.cpu()
    return {
        "value": (abs(out[_lib.OUT_NLL] - val) / abs(val)).item(),
        "dtheta": ((out[_lib.OUT_DTHETA:_lib.OUT_DTHETA + P] - g_theta).abs().max() / g_theta.abs().max()).item(),
        "dr": ((dr[:n] - g_r).abs().max() / g_r.abs().max()).item(),
        "dnoise": ((dnoise[:n] - g_noise).abs().max() / g_noise.abs().max()).item(),
        "sum_dr": (abs(out[_lib.OUT_SUM_DR] - g_r.sum()) / g_r.abs().sum()).item(),
        "dr_w0": (abs(out[_lib.OUT_DR_W0] - (g_r * w[0]).sum()) / (g_r * w[0]).abs().sum()).item(),
        "dr_w1": (abs(out[_lib.OUT_DR_W0 + 1] - (g_r * w[1]).sum()) / (g_r * w[1]).abs().sum()).item(),
        "sum_dnoise": (abs(out[_lib.OUT_SUM_DNOISE] - g_noise.sum()) / g_noise.abs().sum()).item(),
    }


def _check(model, X, r, noise, theta, groups, w, out, dr, dnoise, label=""):
    """-> the worst error per column, each asserted against its bound."""
    P, n = theta.numel(), r.numel()
    errs = _errors(lgo_value_and_grads(model, X, r, noise, theta, groups), w, out, dr, dnoise, P, n)
    print("lgo errors", label, {k: f"{v:.2e}" for k, v in errs.items()})
    out = out.cpu()
    assert int(out[_lib.OUT_INFO]) == 0
    assert errs["value"] < 1e-10, errs
    for k in ("dtheta", "dr", "dnoise", "sum_dr", "dr_w0", "dr_w1", "sum_dnoise"):
        assert errs[k] < 1e-8, (k, errs)
    assert bool((out[_lib.OUT_DTHETA + P:_lib.OUT_SUM_DR] == 0).all())
    return errs


def _row_close(a, b, P, n, label):
    """Two result triples (out, dr, dnoise) agree to the bounds of the module, the second as the reference."""
    ref = (b[0][_lib.OUT_NLL].cpu(), b[0][_lib.OUT_DTHETA:_lib.OUT_DTHETA + P].cpu(), b[1][:n].cpu(), b[2][:n].cpu())
    w = torch.ones(2, n, dtype=torch.float64)
    errs = {k: v for k, v in _errors(ref, w, a[0], a[1], a[2], P, n).items() if not k.startswith("dr_w")}  # (other weights)
    print("lgo row errors", label, {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["value"] < 1e-10, errs
    for k in ("dtheta", "dr", "dnoise", "sum_dr", "sum_dnoise"):
        assert errs[k] < 1e-8, (k, errs)


@pytest.mark.parametrize("model,d,n,layout", PLAN_CASES)
def test_plan_level_against_the_restatement(model, d, n, layout, gpu_device):
    """Measured on MI355X, worst over these cases: value 2.2e-14, dtheta 7.5e-14, dr 3.4e-13, dnoise 8.2e-13, reduced slots 1.1e-13
    ("Leave-group-out training objective")."""
    dev = gpu_device
    X, r, noise, theta = _case(model, d, n)
    groups = folds_for(layout, n)
    w = _weights(n)
    p = plan_for(model, d, n, X, torch.float64, dev)
    p.set_dr_weights(w.to(dev).contiguous())
    p.set_folds(groups)
    res = p.lgo_fit_step(theta, r.to(dev), noise.to(dev))
    _check(model, X, r, noise, theta, groups, w, *res, f"{model} d={d} n={n} {layout}")
    val = p.lgo_value().cpu()
    assert val[0] == res[0][_lib.OUT_NLL].cpu() and val[1] == 0
    P = theta.numel()
    if layout == "ones":  # the other end point: the leave-one-out step's own row
        _row_close(res, p.loo_fit_step(theta, r.to(dev), noise.to(dev)), P, n, "against loo_fit_step")
    if layout == "all":  # one fold of every row: the marginal likelihood, fit_step's row
        _row_close(res, p.fit_step(theta, r.to(dev), noise.to(dev)), P, n, "against fit_step")


@pytest.mark.parametrize("layout", ["scattered", "halves"])
@pytest.mark.parametrize("max_tiles", [0, 1000000])
def test_both_tile_cores_at_three_by_three_tiles(max_tiles, layout, gpu_device):
    """n = 257 (N = 384): the sandwich on the 128 x 128 direct-to-LDS core (selector 0) and on the 64 x 64 register-staged one."""
    dev = gpu_device
    X, r, noise, theta = _case("loadest", 3, 257, seed=4)
    groups = folds_for(layout, 257, seed=4)
    w = _weights(257)
    p = plan_for("loadest", 3, 257, X, torch.float64, dev)
    p.set_option(_lib.OPT_LAUUM64_MAX_TILES, max_tiles)
    p.set_dr_weights(w.to(dev).contiguous())
    p.set_folds(groups)
    _check("loadest", X, r, noise, theta, groups, w, *p.lgo_fit_step(theta, r.to(dev), noise.to(dev)), f"selector {max_tiles} {layout}")


@pytest.mark.parametrize("layout", ["scattered", "blocks65"])
def test_composite_tree(layout, gpu_device):
    dev = gpu_device
    idx = ch.HAND_BUILT[0]
    case = ch.CASES[idx]
    name = ch.define(case.spec)
    n = 130
    X, r, noise = ch.data(idx, n)
    groups = folds_for(layout, n)
    w = _weights(n)
    p = plan_for(name, case.d, n, X, torch.float64, dev)
    p.set_dr_weights(w.to(dev).contiguous())
    p.set_folds(groups)
    _check(name, X, r, noise, case.theta, groups, w, *p.lgo_fit_step(case.theta, r.to(dev), noise.to(dev)), f"{case.name} {layout}")


def _batch(sizes, layouts, dev):
    from discontinuum_amd.backend import GPPlan

    model, d, B, n = "loadest", 3, len(sizes), max(sizes)
    cases = [_case(model, d, nb, seed=10 + b) for b, nb in enumerate(sizes)]
    X = torch.full((B, n, d), float("nan"), dtype=torch.float64)
    r = torch.full((B, n), float("nan"), dtype=torch.float64)
    noise = torch.full((B, n), float("nan"), dtype=torch.float64)
    w = torch.full((B, 2, n), float("nan"), dtype=torch.float64)
    groups = torch.full((B, n), -1, dtype=torch.int64)
    ws = [_weights(nb, seed=b) for b, nb in enumerate(sizes)]
    gs = [folds_for(lay, nb, seed=b) for b, (nb, lay) in enumerate(zip(sizes, layouts))]
    for b, (nb, c) in enumerate(zip(sizes, cases)):
        X[b, :nb], r[b, :nb], noise[b, :nb], w[b, :, :nb], groups[b, :nb] = c[0], c[1], c[2], ws[b], gs[b]
    theta = torch.stack([c[3] for c in cases])
    pb = GPPlan(model, n, d, device=dev, lookahead=1, batch=B)
    pb.set_site_sizes(sizes)
    pb.set_inputs(X.to(dev).contiguous())
    pb.set_dr_weights(w.to(dev).contiguous())
    pb.set_folds(groups)
    res = [t.cpu() for t in pb.lgo_fit_step(theta, r.to(dev).contiguous(), noise.to(dev).contiguous())]
    again = [t.cpu() for t in pb.lgo_fit_step(theta, r.to(dev).contiguous(), noise.to(dev).contiguous())]
    for a, b in zip(res, again):  # two identical calls
        assert torch.equal(a, b)
    return pb, cases, ws, gs, res


def test_ragged_batch_matches_single_site_plans(gpu_device):
    """3 sites (257, 130, 127) with 2, 2 and 5 (of 6 ids) folds; site 0 is bitwise the same in a batch of 11; NaN in every unused
    tail."""
    dev = gpu_device
    sizes, layouts = (257, 130, 127), ("halves", "blocks65", "scattered")
    pb, cases, ws, gs, (out, dr, dnoise) = _batch(sizes, layouts, dev)
    val2 = pb.lgo_value().cpu()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dr).all()) and bool(torch.isfinite(dnoise).all())
    P = pb.ntheta
    for b, (nb, c) in enumerate(zip(sizes, cases)):
        _check("loadest", c[0], c[1], c[2], c[3], gs[b], ws[b], out[b], dr[b], dnoise[b], f"site {b} n={nb}")
        assert bool((dr[b, nb:] == 0).all()) and bool((dnoise[b, nb:] == 0).all())
        assert val2[b, 0] == out[b, _lib.OUT_NLL] and val2[b, 1] == 0
        p1 = plan_for("loadest", 3, nb, c[0], torch.float64, dev, lookahead=1)
        p1.set_dr_weights(ws[b].to(dev).contiguous())
        p1.set_folds(gs[b])
        single = p1.lgo_fit_step(c[3], c[1].to(dev), c[2].to(dev))
        _row_close((out[b], dr[b], dnoise[b]), single, P, nb, f"site {b} against its own plan")
    sizes11 = sizes + (1, 2, 64, 128, 129, 200, 33, 256)
    layouts11 = layouts + ("ones", "all", "scattered", "scattered", "blocks65", "scattered", "scattered", "scattered")
    _pb, cases11, ws11, gs11, (out11, dr11, dnoise11) = _batch(sizes11, layouts11, dev)
    assert torch.equal(out11[0], out[0]) and torch.equal(dr11[0], dr[0]) and torch.equal(dnoise11[0], dnoise[0])
    assert bool(torch.isfinite(out11).all()) and bool(torch.isfinite(dr11).all()) and bool(torch.isfinite(dnoise11).all())
    for b, (nb, c) in enumerate(zip(sizes11, cases11)):  # sizes 1, 2, a tile, a tile and one: every site against the restatement
        _check("loadest", c[0], c[1], c[2], c[3], gs11[b], ws11[b], out11[b], dr11[b], dnoise11[b], f"batch of 11, site {b} n={nb}")
        assert bool((dr11[b, nb:] == 0).all()) and bool((dnoise11[b, nb:] == 0).all())


@pytest.mark.parametrize("n,k", [(128, 3), (256, 5), (256, 3), (384, 5)])
def test_last_fold_ends_on_the_last_row_of_the_padded_matrix(n, k, gpu_device):
    """n a multiple of 128 (N = n) and a ragged last fold: its last k-tile of 16 would pass row N of the gathered operand.  Both
    routes (folds of 43 / 52: LDS route, 64-tiles; 86 / 77: block route, 128-tiles), with the work area full of NaN before the
    call: a read past the operand, or of anything the call did not write, shows as NaN."""
    dev = gpu_device
    X, r, noise, theta = _case("loadest", 3, n, seed=7)
    groups = torch.arange(n) * k // n
    sizes = torch.bincount(groups)
    start = int(sizes[:-1].sum())
    assert start + (int(sizes[-1]) + 15) // 16 * 16 > n  # the case is the one meant
    w = _weights(n)
    p = plan_for("loadest", 3, n, X, torch.float64, dev)
    assert p.N == n
    p.set_dr_weights(w.to(dev).contiguous())
    p.set_folds(groups)
    p.lgo_fit_step(theta, r.to(dev), noise.to(dev))  # (allocates the work area)
    p._loo_ws.fill_(255)  # every double a NaN
    res = p.lgo_fit_step(theta, r.to(dev), noise.to(dev))
    p._loo_ws.zero_()
    _check("loadest", X, r, noise, theta, groups, w, *res, f"n={n} {k} folds, last fold at {start}")
    p._loo_ws.fill_(255)
    again = p.lgo_fit_step(theta, r.to(dev), noise.to(dev))
    p._loo_ws.zero_()  # (the block returns to the allocator's cache: leave no NaN behind for whoever gets it next)
    for a, b in zip(res, again):
        assert torch.equal(a, b)


def test_fold_blocks_do_not_depend_on_the_core_that_inverts_them(gpu_device):
    """The block route makes C_g = M^-T M^-1 with the library's lauum, whose core (64- or 128-tiles) follows tiles x slots of the
    chunk, hence the batch: the selector forced both ways gives the same bits."""
    dev = gpu_device
    X, r, noise, theta = _case("loadest", 3, 257, seed=4)
    rows = []
    for max_tiles in (0, 1000000):
        p = plan_for("loadest", 3, 257, X, torch.float64, dev)
        p.set_option(_lib.OPT_LAUUM64_MAX_TILES, max_tiles)
        p.set_folds(folds_for("halves", 257))
        rows.append([t.cpu() for t in p.lgo_fit_step(theta, r.to(dev), noise.to(dev))])
    for a, b in zip(*rows):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n,layout,route", [(130, "scattered", "lds"), (257, "halves", "block")])
def test_a_fold_that_is_not_positive_definite_is_reported_by_its_index(n, layout, route, gpu_device):
    """With a factorisation whose own status is 0 every G_g is positive definite up to rounding, so the fold's status is reached
    here by spoiling the held inverse: a negative diagonal entry of S in a row of fold 1 (and of no other fold).  INFO = 1 + the
    fold's index, the value NaN, return code 0."""
    dev = gpu_device
    X, r, noise, theta = _case("loadest", 3, n, seed=8)
    groups = folds_for(layout, n)
    p = plan_for("loadest", 3, n, X, torch.float64, dev)
    p.set_folds(groups)
    out = p.lgo_fit_step(theta, r.to(dev), noise.to(dev))[0].cpu()
    assert out[_lib.OUT_INFO] == 0 and torch.isfinite(out[_lib.OUT_NLL])
    S = p.buffer(_lib.BUF_S)
    i = int(torch.nonzero(groups == 1)[0])
    S[i, i] = -1.0
    val = p.lgo_value().cpu()
    assert val[1] == 2 and torch.isnan(val[0]), (route, val)


@pytest.mark.parametrize("n,layout", [(130, "scattered"), (130, "blocks65"), (257, "halves"), (257, "ones")])
def test_value_agrees_with_cross_validation(n, layout, gpu_device):
    """Two device paths: lgo_value = -sum lpd of dgp_cross_validate on the same folds."""
    dev = gpu_device
    X, r, noise, theta = _case("loadest", 3, n, seed=5)
    groups = folds_for(layout, n, seed=5)
    p = plan_for("loadest", 3, n, X, torch.float64, dev)
    p.set_folds(groups)
    out = p.lgo_fit_step(theta, r.to(dev), noise.to(dev))[0]
    val = p.lgo_value().cpu()
    _resid, _var, lpd, info = p.cross_validate(groups)
    ref = -lpd.sum().item()
    assert int(info.abs().max()) == 0 and val[1] == 0
    assert abs(val[0].item() - ref) <= 1e-10 * abs(ref)
    assert val[0] == out[_lib.OUT_NLL].cpu()
    out_f = p.fit_step(theta, r.to(dev), noise.to(dev))[0]  # ... and from the inverse a plain fit step leaves
    assert p.lgo_value().cpu()[0] == val[0] and torch.isfinite(out_f[0])


def test_leaves_the_plan_as_fit_step_does_and_the_other_steps_alone(gpu_device):
    dev = gpu_device
    model, d, n = "rating", 2, 257
    X, r, noise, theta = _case(model, d, n, seed=2)
    Xs = X[:50].to(dev).contiguous()
    rd, nd = r.to(dev), noise.to(dev)
    clean = plan_for(model, d, n, X, torch.float64, dev)  # never calls an lgo entry
    loo_clean = [t.clone() for t in clean.loo_fit_step(theta, rd, nd)]
    p = plan_for(model, d, n, X, torch.float64, dev)
    f_out = p.fit_step(theta, rd, nd)[0].clone()
    alpha0 = p.buffer(_lib.BUF_ALPHA).clone()
    S0, T0 = p.buffer(_lib.BUF_S).clone(), p.buffer(_lib.BUF_T).clone()
    pred0 = [t.clone() for t in p.predict(theta, Xs)]
    for layout in ("scattered", "halves"):
        p.set_folds(folds_for(layout, n))
        first = [t.clone() for t in p.lgo_fit_step(theta, rd, nd)]
        assert torch.equal(p.buffer(_lib.BUF_ALPHA), alpha0)
        assert torch.equal(torch.tril(p.buffer(_lib.BUF_S)[:n, :n]), torch.tril(S0[:n, :n]))
        assert torch.equal(torch.tril(p.buffer(_lib.BUF_T)[:n, :n]), torch.tril(T0[:n, :n]))
        pred1 = p.predict(theta, Xs)
        assert torch.equal(pred0[0], pred1[0]) and torch.equal(pred0[1], pred1[1])
        for k in (_lib.OUT_QUAD, _lib.OUT_LOGDET, _lib.OUT_INFO):
            assert first[0][k] == f_out[k]
        for a, b in zip(first, p.lgo_fit_step(theta, rd, nd)):
            assert torch.equal(a, b)
    for a, b in zip(loo_clean, p.loo_fit_step(theta, rd, nd)):
        assert torch.equal(a, b)
    assert torch.equal(f_out, p.fit_step(theta, rd, nd)[0])


def test_errors_and_a_site_that_is_not_positive_definite(gpu_device):
    from discontinuum_amd.backend import GPPlan

    dev = gpu_device
    model, d, n = "loadest", 3, 130
    X, r, noise, theta = _case(model, d, n, seed=6)
    groups = folds_for("scattered", n)
    p = plan_for(model, d, n, X, torch.float64, dev)
    lib = p.lib
    with pytest.raises(ValueError, match="set_folds"):
        p.lgo_fit_step(theta, r.to(dev), noise.to(dev))
    with pytest.raises(ValueError, match="set_folds"):
        p.lgo_value()
    p.set_folds(groups)
    order, start, ngroups, max_group = p._folds
    with pytest.raises(Exception, match="K\\^\\^-1|inverse"):  # no factorisation yet
        p.lgo_value()
    p.factorize(theta, r.to(dev), noise.to(dev))  # a factorisation without S
    with pytest.raises(Exception, match="K\\^\\^-1|inverse"):
        p.lgo_value()
    need = int(lib.dgp_lgo_workspace_bytes(p._h, ngroups, max_group))
    assert need >= 3 * p.N * p.N * 8
    assert lib.dgp_lgo_workspace_bytes(p._h, 0, max_group) == 0 and lib.dgp_lgo_workspace_bytes(p._h, ngroups, n + 1) == 0
    work = torch.empty(need + 512, dtype=torch.uint8, device=dev)
    base = work.data_ptr() + (-work.data_ptr()) % 256
    out = torch.full((_lib.OUT_LEN,), 7.0, dtype=torch.float64, device=dev)
    th = (C.c_double * p.ntheta)(*theta.tolist())
    rd, nd = r.to(dev), noise.to(dev)

    def call(ptr, nbytes, ng=ngroups, mg=max_group):
        with torch.cuda.device(dev):
            return lib.dgp_lgo_fit_step(p._h, th, C.c_void_p(rd.data_ptr()), C.c_void_p(nd.data_ptr()), C.c_void_p(order.data_ptr()),
                                        C.c_void_p(start.data_ptr()), ng, mg, C.c_void_p(ptr), nbytes, C.c_void_p(out.data_ptr()),
                                        None, None, C.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert call(base, need - 1) == -3 and call(0, need) == -3  # DGP_E_WORKSPACE
    assert call(base + 8, need) == -1 and b"aligned" in lib.dgp_last_error()
    assert call(base, need, ng=0) == -1 and call(base, need, mg=n + 1) == -1
    assert lib.dgp_lgo_fit_step(p._h, None, None, None, None, None, ngroups, max_group, C.c_void_p(base), need, None, None, None,
                                None) == -1
    torch.cuda.synchronize(dev)
    assert bool((out == 7.0).all())  # nothing was launched
    assert call(base, need) == 0  # dr / dnoise are optional, as for dgp_fit_step
    torch.cuda.synchronize(dev)
    assert torch.equal(out, p.lgo_fit_step(theta, rd, nd)[0])
    p32 = plan_for(model, d, n, X, torch.float32, dev)
    assert lib.dgp_lgo_workspace_bytes(p32._h, ngroups, max_group) == 0
    p32.set_folds(groups)
    with pytest.raises(Exception, match="float64"):
        p32.lgo_fit_step(theta, r.float().to(dev), noise.float().to(dev))
    # a fold made singular as the leave-one-out test makes its bad row: two identical rows, both in fold 0, whose noise cancels
    # the diagonal -- the site reports it, the other site of the batch is untouched
    Xb = X.clone()
    Xb[40] = Xb[41]
    bad = noise.clone()
    bad[40] = bad[41] = -0.5
    g2 = groups.clone()
    g2[40] = g2[41] = 0
    pb = GPPlan(model, n, d, device=dev, lookahead=1, batch=2)
    pb.set_inputs(torch.stack([Xb, X]).to(dev).contiguous())
    pb.set_folds(torch.stack([g2, g2]))
    args = (theta.repeat(2, 1), torch.stack([r, r]).to(dev).contiguous(), torch.stack([bad, noise]).to(dev).contiguous())
    o2, dr2, dn2 = pb.lgo_fit_step(*args)
    o2 = o2.cpu()
    assert o2[0, _lib.OUT_INFO] >= 1 and not torch.isfinite(o2[0, _lib.OUT_NLL])
    p.set_folds(g2)
    good = p.lgo_fit_step(theta, rd, nd)
    assert o2[1, _lib.OUT_INFO] == 0
    assert torch.equal(o2[1], good[0].cpu()) and torch.equal(dr2[1].cpu(), good[1].cpu()) and torch.equal(dn2[1].cpu(), good[2].cpu())


def test_engine_fit_against_the_double(gpu_device):
    from discontinuum_amd.loadest_gp import LoadestGP
    from tests.helpers import loadest_dataset

    cov, tgt = loadest_dataset(n=120, seed=3)[:2]
    traces = {}
    models = {}
    for kind in ("gpu", "double"):
        torch.manual_seed(0)
        m = LoadestGP()
        if kind == "double":
            m.device = "cpu"
            m._plan_factory = LgoOraclePlan
        trace = []
        import discontinuum_amd.gp.explicit as ex

        orig = ex.ExplicitObjective.evaluate

        def spy(self, *a, _orig=orig, _trace=trace, **k):
            v = _orig(self, *a, **k)
            _trace.append(v)
            return v

        ex.ExplicitObjective.evaluate = spy
        try:
            m.fit(cov, tgt, iterations=5, objective="lgo", folds=4)
        finally:
            ex.ExplicitObjective.evaluate = orig
        traces[kind], models[kind] = np.asarray(trace), m
    assert len(traces["gpu"]) == 5 and models["gpu"].objective_ == "lgo"
    print("lgo engine traces", traces)
    np.testing.assert_allclose(traces["gpu"], traces["double"], rtol=1e-7)
    mu_g, se_g = models["gpu"].predict(cov)
    mu_d, se_d = models["double"].predict(cov)
    np.testing.assert_allclose(mu_g.values, mu_d.values, rtol=1e-7)
    np.testing.assert_allclose(se_g.values, se_d.values, rtol=1e-7)
    # -elpd of cross_validate(4) at the final hyperparameters = the data term of an objective evaluated there
    m = models["gpu"]
    cv = m.cross_validate(4)
    from discontinuum_amd.gp.mll import ExactMarginalLogLikelihood

    mll = ExactMarginalLogLikelihood(m.likelihood, m.model)
    with torch.no_grad():
        total = float(-mll(m._prior(), m._train_y)) * 120 + float(mll.log_prior())
    np.testing.assert_allclose(-cv.attrs["elpd"], total, rtol=1e-7)
