"""The streamed value of additional samples (``streamed=True`` of ``sample_value`` / ``design_value`` / ``design``) on CPU, with
the device plan replaced by a numpy double whose ``posterior_sample_value`` walks the covariance PANEL BY PANEL in the kernel's
accounting -- a block of 64 candidates takes, from a panel, the panel's rows at or after the block and, when its own rows lie in
the panel, every day before it; entries above the diagonal of a panel are NaN and the diagonal is the predicted variance -- so
that the pair bookkeeping itself is tested here: every ordered pair (day, candidate) exactly once.  The streamed Datasets equal
the dense ones, the default calls never reach a new plan method, the refusals, and the five new C names are declared, bound
and refuse bad arguments without a device."""
from __future__ import annotations

import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from discontinuum_amd.backend import stream_panel_rows
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.engines.base import ModelConfig
from tests.design_helpers import DesignOraclePlan
from tests.flux_helpers import daily_loadest, dense_period_moments

PANEL = 128


def _np(t):
    return None if t is None else torch.as_tensor(t).detach().cpu().double().numpy()


class StreamPlan(DesignOraclePlan):
    """``DesignOraclePlan`` plus the three streamed entries, in numpy, and counters of every call to them."""

    counts: dict = {}
    pair_counts: list = []

    def _dense_cov(self, theta, Xs):
        _mu, cov = DesignOraclePlan.posterior_cov(self, theta, Xs)
        C_ = _np(cov)
        return np.tril(C_) + np.tril(C_, -1).T

    def posterior_period_moments(self, theta, Xs, mu, scale2, w, groups, ngroups, mode, extra_var=None):
        return dense_period_moments(self._dense_cov(theta, Xs), mu, scale2, w, groups, ngroups, mode, extra_var)

    def sample_value_panel_rows(self, m, ngroups, nrows, nterms, max_bytes=None):
        M = -(-m // 128) * 128
        per_panel = 8 * 128 * M
        fixed = 8 * (M * (2 + ngroups * nterms) + ngroups)
        return stream_panel_rows(fixed + per_panel, per_panel if M > 128 else 0, M, max_bytes, "the streamed value of samples")

    def posterior_sample_value(self, theta, Xs, a, scale2, groups, ngroups, obs_var=None, rows=None, nterms=None, panel_rows=None,
                               max_bytes=None):
        StreamPlan.counts["posterior_sample_value"] = StreamPlan.counts.get("posterior_sample_value", 0) + 1
        Cfull = self._dense_cov(theta, Xs)
        var = _np(self.predict(theta, Xs)[1])
        m = Cfull.shape[0]
        M = -(-m // 128) * 128
        R = min(int(panel_rows), M)
        assert R > 0 and R % 128 == 0
        a, g, s2, K, P = _np(a), _np(groups).astype(np.int64), float(scale2), int(nterms), int(ngroups)
        B = np.zeros((0, m)) if rows is None else _np(rows)
        tau2 = np.zeros(m) if obs_var is None else _np(obs_var)
        v = var - (B ** 2).sum(axis=0) + tau2
        rs = np.where(v > 0, 1.0 / np.sqrt(np.where(v > 0, v, 1.0)), 0.0)
        S = np.zeros((P, K, M))
        seen = np.zeros((m, m), dtype=np.int64)  # [day, candidate]
        for p0 in range(0, M, R):
            p1 = min(p0 + R, M)
            panel = np.full((p1 - p0, M), np.nan)  # rows p0 .. p1 - 1 of C, columns up to the row's own: the rest is never read
            for i in range(p0, min(p1, m)):
                panel[i - p0, : i + 1] = Cfull[i, : i + 1]
            for c0 in range(0, p1, 64):
                cand = np.arange(c0, min(c0 + 64, m))
                if not cand.size:
                    continue
                own = c0 >= p0
                days = np.arange(0 if own else p0, min(p1, m))
                for p in range(P):
                    dp = days[g[days] == p]
                    if not dp.size:
                        continue
                    x = np.empty((dp.size, cand.size))
                    for k, i in enumerate(dp):
                        below = cand <= i  # C[i][c] from the row of day i, which must lie in the panel
                        if below.any():
                            assert p0 <= i < p1
                            x[k, below] = panel[i - p0, cand[below]]
                        if (~below).any():  # C[c][i] from the candidates' rows: only when they lie in the panel
                            assert own
                            x[k, ~below] = panel[cand[~below] - p0, i]
                        if i in cand:
                            x[k, i - c0] = var[i]  # the diagonal: the predicted variance
                    seen[np.ix_(dp, cand)] += 1
                    x = x - B[:, dp].T @ B[:, cand]
                    b = x * rs[cand][None, :]
                    assert np.all(np.isfinite(b))
                    pw = a[dp][:, None] * np.ones_like(b)
                    for k in range(K):
                        pw = pw * b
                        S[p, k, cand] += pw.sum(axis=0)
        StreamPlan.pair_counts.append(seen[g >= 0])
        coef = np.array([s2 ** (k + 1) / math.factorial(k + 1) for k in range(K)])
        gain = np.einsum("k,pkc->pc", coef, S[:, :, :m] ** 2)
        return torch.tensor(gain), torch.tensor(np.where(v > 0, v, 0.0))

    def posterior_cov_columns(self, theta, Xs, idx):
        StreamPlan.counts["posterior_cov_columns"] = StreamPlan.counts.get("posterior_cov_columns", 0) + 1
        idx = [int(i) for i in np.asarray(idx).reshape(-1)]
        assert 1 <= len(idx) <= 64
        return torch.tensor(self._dense_cov(theta, Xs)[idx, :])

    def lowrank_period_moments(self, rows, m, mu, scale2, w, groups, ngroups, mode):
        StreamPlan.counts["lowrank_period_moments"] = StreamPlan.counts.get("lowrank_period_moments", 0) + 1
        B = _np(rows)
        assert 1 <= B.shape[0] <= 64 and B.shape[1] == m
        return dense_period_moments(B.T @ B, mu, scale2, w, groups, ngroups, mode)


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(StreamPlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)
    StreamPlan.counts, StreamPlan.pair_counts = {}, []


_MODELS = {}


def _loadest(transform="log"):
    if transform not in _MODELS:
        cov_obs, target, daily = daily_loadest(seed=0, step_days=5)  # 220 days, three years: M = 256, two 128-row panels
        model = LoadestGP() if transform == "log" else LoadestGP(model_config=ModelConfig(transform=transform))
        model.fit(cov_obs, target, iterations=10)
        _MODELS[transform] = (model, daily)
    return _MODELS[transform]


def _budget(model, daily, rows=PANEL):
    """The ``max_bytes`` at which the double's size formula (M = 256, 3 periods, the record's series length) leaves exactly
    ``rows`` panel rows."""
    K = model.sample_value(daily).attrs["nterms"]
    return 8 * (256 * (2 + 3 * K) + 3) + 8 * rows * 256


def _close(dense, streamed, rtol=1e-10):
    assert set(dense) == set(streamed)
    for key in dense:
        x, y = np.asarray(dense[key].values), np.asarray(streamed[key].values)
        if x.dtype.kind != "f":
            assert np.array_equal(x, y), key
        else:
            assert np.allclose(x, y, rtol=rtol, atol=rtol * float(np.abs(x).max())), (key, float(np.abs(x - y).max()))
    for key in dense.coords:
        assert np.array_equal(np.asarray(dense.coords[key].values), np.asarray(streamed.coords[key].values)), key
    assert dense.attrs == streamed.attrs


# ------------------------------------------------------------------------------------------------ streamed == dense
@pytest.mark.parametrize("transform", ["log", "standard"])
def test_streamed_datasets_equal_the_dense_ones(transform):
    model, daily = _loadest(transform)
    time = daily.coords["time"].values
    budget = _budget(model, daily)
    kw = dict(sample_var=0.02)
    for given in (None, time[[10, 95, 200]]):
        dense = model.sample_value(daily, given=given, **kw)
        assert not StreamPlan.counts
        streamed = model.sample_value(daily, given=given, streamed=True, max_bytes=budget, **kw)
        _close(dense, streamed)
        assert StreamPlan.counts.pop("posterior_sample_value") == 1
        assert StreamPlan.counts.pop("posterior_cov_columns", 0) == (0 if given is None else 1)
        assert StreamPlan.counts.pop("lowrank_period_moments", 0) == (0 if given is None else 1) and not StreamPlan.counts
        assert (dense.attrs["nterms"] == 1) == (transform == "standard")
    # the double walked two panels and met every ordered pair (day of a period, candidate) exactly once
    assert StreamPlan.pair_counts and all(np.all(seen == 1) for seen in StreamPlan.pair_counts)
    for samples in ([95], [10, 95, 96, 200], [50, 50, 7]):  # (a day may repeat: replicate samples)
        dense, V = model.design_value(daily, samples, return_cov=True, **kw)
        streamed, V2 = model.design_value(daily, samples, return_cov=True, streamed=True, max_bytes=budget, **kw)
        _close(dense, streamed)
        assert np.allclose(V, V2, rtol=0, atol=1e-10 * np.abs(V).max())
    StreamPlan.counts = {}
    mask = np.zeros(len(time), dtype=bool)
    mask[[3, 50, 120, 121]] = True
    for args in (dict(k=4), dict(k=3, objective="absolute", given=time[[10, 95]]), dict(k=3, candidates=mask),
                 dict(k=3, candidates=[50], replicates=True)):
        dense = model.design(daily, **args, **kw)
        assert not StreamPlan.counts
        streamed = model.design(daily, streamed=True, max_bytes=budget, **args, **kw)
        _close(dense, streamed, rtol=1e-9)
        assert StreamPlan.counts.pop("posterior_sample_value") == args["k"]
        StreamPlan.counts = {}
    assert all(np.all(seen == 1) for seen in StreamPlan.pair_counts)


def test_the_double_takes_the_forced_panel_and_full_height_agrees():
    model, daily = _loadest()
    seen = []
    real = StreamPlan.posterior_sample_value

    def spy(self, *a, **kw):
        seen.append(kw["panel_rows"])
        return real(self, *a, **kw)

    StreamPlan.posterior_sample_value = spy
    try:
        short = model.sample_value(daily, streamed=True, max_bytes=_budget(model, daily, 128))
        full = model.sample_value(daily, streamed=True)
    finally:
        StreamPlan.posterior_sample_value = real
    assert seen == [128, 256]
    _close(short, full, rtol=1e-12)


# ------------------------------------------------------------------------------------------------ default path, refusals
def test_default_calls_never_reach_the_new_plan_methods_and_refusals_stay():
    model, daily = _loadest()
    model.sample_value(daily, given=[4])
    model.design_value(daily, [1, 2])
    model.design(daily, 2)
    assert not StreamPlan.counts
    # the dense refusals, texts unchanged; streamed=True is never chosen automatically
    with pytest.raises(ValueError, match=r"^the value of samples needs the dense posterior covariance: a footprint of \d+ bytes for m = 220 "
                                         r"points exceeds max_bytes = 100000$"):
        model.sample_value(daily, max_bytes=100_000)
    with pytest.raises(ValueError, match=r"^the value of samples needs the dense posterior covariance and a second \(M, M\) buffer: a "
                                         r"footprint of \d+ bytes for m = 220 points exceeds max_bytes = 100000$"):
        model.design(daily, 2, max_bytes=100_000)
    assert not StreamPlan.counts
    # a budget too small for a 128-row panel names the bytes
    for call in (lambda: model.sample_value(daily, streamed=True, max_bytes=100_000),
                 lambda: model.design_value(daily, [3], streamed=True, max_bytes=100_000),
                 lambda: model.design(daily, 2, streamed=True, max_bytes=100_000)):
        with pytest.raises(ValueError, match=r"the streamed value of samples needs a work area of \d+ bytes with the smallest panel \(128 "
                                             r"rows\), which exceeds max_bytes = 100000$"):
            call()
    assert not StreamPlan.counts
    with pytest.raises(ValueError, match="at most 64"):
        model.design(daily, 65, streamed=True)
    with pytest.raises(ValueError, match="at most 64 samples"):
        model.design_value(daily, np.arange(65), streamed=True)
    with pytest.raises(ValueError, match="given: 2030-01-01"):
        model.sample_value(daily, given=["2030-01-01"], streamed=True)


# ------------------------------------------------------------------------------------------------ the C entries, no device
NAMES = ("dgp_posterior_sample_value_workspace_bytes", "dgp_posterior_sample_value", "dgp_posterior_cov_columns_workspace_bytes",
         "dgp_posterior_cov_columns", "dgp_lowrank_period_moments")


def test_abi_is_declared_bound_and_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    names = set(NAMES)
    assert names <= set(_lib.EXT2_SIGNATURES) and not names & set(_lib.SIGNATURES) and not names & set(_lib.EXT_SIGNATURES)
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    ext2 = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "dgp_hip_ext2.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(dgp_[a-z_0-9]+)\s*\(", ext2))
    for name in NAMES:
        fn = getattr(lib, name)  # (an export of the library)
        assert fn.argtypes == _lib.EXT2_SIGNATURES[name][1] and fn.restype == _lib.EXT2_SIGNATURES[name][0]
    q, f = lib.dgp_posterior_sample_value_workspace_bytes, lib.dgp_posterior_sample_value
    qc, fc = lib.dgp_posterior_cov_columns_workspace_bytes, lib.dgp_posterior_cov_columns
    assert q(None, 100, 2, 0, 1, 128) == 0 and qc(None, 100, 1) == 0
    one = C.c_void_p(256)  # never dereferenced: every call below returns before any launch
    th = (C.c_double * 8)()
    assert f(None, th, one, 100, one, one, one, 2, None, None, 0, 1, 128, one, 1 << 20, one, one, None) == -1
    assert fc(None, th, one, 100, one, 1, one, 1 << 20, one, None) == -1
    h = C.c_void_p()
    assert lib.dgp_plan_create(_lib.MODEL_LOADEST, _lib.F64, 200, 3, C.byref(h)) == 0
    try:
        assert q(h, 100, 2, 0, 1, 128) > 0 and q(h, 100, 2, 0, 1, 256) == q(h, 100, 2, 0, 1, 128)  # M = 128: the panel is capped at M
        assert q(h, 300, 2, 0, 1, 256) - q(h, 300, 2, 0, 1, 128) == 8 * 128 * 384                  # one more panel row block
        assert q(h, 300, 2, 0, 9, 128) - q(h, 300, 2, 0, 8, 128) == 8 * 2 * 384                    # S grows by P M doubles per term
        assert q(h, 300, 2, 64, 8, 128) == q(h, 300, 2, 0, 8, 128)
        for bad_rows in (0, -128, 64, 100, 200):
            assert q(h, 100, 2, 0, 1, bad_rows) == 0
        for bad in ((0, 2, 0, 1), ((1 << 20) + 1, 2, 0, 1), (100, 0, 0, 1), (100, 65536, 0, 1), (100, 2, -1, 1), (100, 2, 65, 1),
                    (100, 2, 0, 0), (100, 2, 0, 65)):
            assert q(h, *bad, 128) == 0, bad
        assert qc(h, 100, 1) > 0 and qc(h, 100, 64) == qc(h, 100, 1)
        for bad in ((0, 1), ((1 << 20) + 1, 1), (100, 0), (100, 65)):
            assert qc(h, *bad) == 0, bad
        ok = (h, th, one, 100, one, one, one, 2, None, one, 2, 4, 128, one, 1 << 30, one, one, None)

        def call(**kw):
            a = list(ok)
            for i, v in kw.items():
                a[int(i[1:])] = v
            return f(*a)

        for i in (1, 2, 4, 5, 6, 9, 15, 16):  # theta, Xs, a, scale2, group, rows (nrows = 2), gain_out, var_out
            assert call(**{f"a{i}": None}) == -1 and b"null" in lib.dgp_last_error(), i
        for kw in (dict(a3=0), dict(a7=0), dict(a7=65536), dict(a10=-1), dict(a10=65), dict(a11=0), dict(a11=65)):
            assert call(**kw) == -1 and b"size" in lib.dgp_last_error(), kw
        for rows in (0, 64, 100, 129, -128):
            assert call(a12=rows) == -1 and b"panel_rows" in lib.dgp_last_error()
        assert call() == -4 and b"factorisation" in lib.dgp_last_error()  # DGP_E_STATE: nothing factorised yet
        okc = (h, th, one, 100, one, 2, one, 1 << 30, one, None)
        for i in (1, 2, 4, 8):
            a = list(okc)
            a[i] = None
            assert fc(*a) == -1 and b"null" in lib.dgp_last_error(), i
        for i, v in ((3, 0), (5, 0), (5, 65)):
            a = list(okc)
            a[i] = v
            assert fc(*a) == -1 and b"size" in lib.dgp_last_error(), (i, v)
        assert fc(*okc) == -4 and b"factorisation" in lib.dgp_last_error()
    finally:
        lib.dgp_plan_destroy(h)
    fl = lib.dgp_lowrank_period_moments
    okl = [1, one, 4, 100, 1, one, one, one, one, 2, one, 1 << 30, one, one, None]
    for i in (1, 5, 6, 7, 8, 12, 13):
        a = list(okl)
        a[i] = None
        assert fl(*a) == -1 and b"null" in lib.dgp_last_error(), i
    for i, v in ((0, 2), (2, 0), (2, 65), (3, 0), (4, 0), (4, 1025), (9, 0)):
        a = list(okl)
        a[i] = v
        assert fl(*a) == -1, (i, v)
    need = lib.dgp_period_moments_workspace_bytes(100, 2, 1)
    a = list(okl)
    a[11] = need - 1
    assert fl(*a) == -3 and b"workspace" in lib.dgp_last_error()
    a[10], a[11] = None, need
    assert fl(*a) == -3
