"""Streamed rolling means (``streamed=True`` of ``rolling_mean`` and of ``exceedance_probability(window=)``) on CPU, with the
device plan replaced by an oracle-backed double that records what it is handed: the streamed branch takes ``predict_mean`` and
ONE ``posterior_window_variances`` and never forms the dense covariance or its windowed product, gives the dense Dataset to
rounding, hands ``max_bytes`` to the plan where the dense path refuses, the refusals old and new, ``window_panel_rows``
against a brute-force scan of the C workspace query, and the argument checks of the three new C entries (no device)."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib
from discontinuum_amd.backend import MODE_LINEAR, MODE_LOG, GPPlan
from discontinuum_amd.engines.base import ModelConfig
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.loads import target_transform
from discontinuum_amd.rolling import record_windows
from discontinuum_amd.xr_compat import Dataset
from tests.flux_helpers import daily_loadest
from tests.window_stream_helpers import WindowStreamOraclePlan as Spy
from tests.window_stream_helpers import window_stream_bytes


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(Spy))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)
    Spy.calls = []


_MODELS = {}
SPAN = dict(start="2012-06-01", end="2013-06-01")  # one year of days: m = 365


def _loadest(transform="log"):
    if transform not in _MODELS:
        cov_obs, target, daily = daily_loadest(n_obs=40, **SPAN)
        model = LoadestGP() if transform == "log" else LoadestGP(model_config=ModelConfig(transform=transform))
        model.fit(cov_obs, target, iterations=10)
        _MODELS[transform] = (model, daily)
    return _MODELS[transform]


def _with_gaps(daily):
    """The record with two gaps and thinned stretches: windows of "30D" hold 8 to 30 points."""
    i = np.arange(len(daily.coords["time"].values))
    keep = ((i < 120) | ((i >= 150) & (i < 260)) | (i >= 300)) & ~((i >= 60) & (i < 110) & (i % 3 != 0))
    flow = daily["flow"]
    return Dataset({"flow": ("time", np.asarray(flow.values)[keep], dict(flow.attrs))}, coords={"time": daily.coords["time"].values[keep]})


def _names(kind=None):
    return [name for name, _d in Spy.calls if kind is None or name == kind]


def _same(got, ref, tag):
    """The same Dataset to 1e-12: variables, attrs, coordinates, the integers exactly."""
    assert set(got) == set(ref) and got.attrs == ref.attrs, tag
    assert np.array_equal(got.coords["time"].values, ref.coords["time"].values), tag
    assert np.array_equal(got["n_points"].values, ref["n_points"].values), tag
    for k in ("mean", "se", "lower", "upper"):
        x, y = np.asarray(got[k].values, np.float64), np.asarray(ref[k].values, np.float64)
        assert x.shape == y.shape and np.allclose(x, y, rtol=1e-12, atol=0), (tag, k, float(np.max(np.abs(x - y) / np.abs(y))))
        assert got[k].attrs == ref[k].attrs, (tag, k)


# ------------------------------------------------------------------------------------------------ the host product
@pytest.mark.parametrize("case", ["log-geometric", "log-arithmetic", "linear", "center", "gaps"])
def test_streamed_rolling_mean_is_the_dense_dataset_and_never_forms_the_covariance(case):
    model, daily = _loadest("standard" if case == "linear" else "log")
    kw = dict(statistic="mean") if case == "log-arithmetic" else dict(align="center") if case == "center" else {}
    if case == "gaps":
        daily, kw = _with_gaps(daily), dict(min_periods=8)
    dense = model.rolling_mean(daily, "30D", **kw)
    assert _names() == ["posterior_cov", "window_moments"]  # the default path is what it was
    Spy.calls = []
    streamed = model.rolling_mean(daily, "30D", streamed=True, **kw)
    assert _names() == ["predict_mean", "posterior_window_variances"]  # no posterior_cov, no window_moments
    _same(streamed, dense, case)
    call = Spy.calls[-1][1]
    Xnew, _times, lo, hi, out = record_windows(model, daily, "30D", kw.get("align", "right"), kw.get("min_periods"))
    mode, s, t = target_transform(model.dm)
    latent = (model._plan.predict_mean(model._factor_theta, Xnew) + model.model.prior_mean(Xnew)).detach().numpy()
    assert call["m"] == Xnew.shape[0] and np.array_equal(call["lo"], lo) and np.array_equal(call["hi"], hi) and call["a"] is None
    if case == "log-arithmetic":
        assert call["mode"] == MODE_LOG and call["scale2"] == s * s and np.allclose(call["mu"], s * latent + t, rtol=1e-12, atol=0)
    else:
        assert call["mode"] == MODE_LINEAR and call["scale2"] is None and np.allclose(call["mu"], latent, rtol=1e-12, atol=0)
    assert call["panel_rows"] is None and len(streamed["mean"].values) == len(out)
    if case == "gaps":
        n = streamed["n_points"].values
        assert n.min() == 8 and n.max() == 30 and len(n) < Xnew.shape[0]


@pytest.mark.parametrize("case", ["log", "linear", "center", "gaps"])
def test_streamed_exceedance_probability_of_the_rolling_mean(case):
    model, daily = _loadest("standard" if case == "linear" else "log")
    kw = dict(align="center") if case == "center" else {}
    if case == "gaps":
        daily, kw = _with_gaps(daily), dict(min_periods=8)
    tau = float(np.median(model.rolling_mean(daily, "30D", **kw)["mean"].values))
    Spy.calls = []
    for above in (True, False):
        dense = model.exceedance_probability(daily, tau, above=above, window="30D", **kw)
        streamed = model.exceedance_probability(daily, tau, above=above, window="30D", streamed=True, **kw)
        assert np.allclose(streamed.values, dense.values, rtol=0, atol=1e-12) and streamed.attrs == dense.attrs
        assert np.array_equal(streamed.coords["time"].values, dense.coords["time"].values)
    assert _names() == ["posterior_cov", "window_moments", "predict_mean", "posterior_window_variances"] * 2
    assert Spy.calls[-1][1]["mode"] == MODE_LINEAR
    assert dense.values.min() < 0.5 < dense.values.max()


def test_under_a_small_budget_the_dense_call_raises_and_the_streamed_one_hands_it_to_the_plan():
    model, daily = _loadest()
    budget = 1_000_000  # the dense footprint of m = 365 is several megabytes
    with pytest.raises(ValueError, match=r"footprint of \d+ bytes.*max_bytes = 1000000; pass streamed=True$"):
        model.rolling_mean(daily, "30D", max_bytes=budget)
    with pytest.raises(ValueError, match=r"footprint of \d+ bytes.*max_bytes = 1000000; pass streamed=True$"):
        model.exceedance_probability(daily, 1.0, window="30D", max_bytes=budget)
    assert not _names("posterior_cov") and not _names("posterior_window_variances")
    ds = model.rolling_mean(daily, "30D", streamed=True, max_bytes=budget)
    assert Spy.calls[-1][0] == "posterior_window_variances" and Spy.calls[-1][1]["max_bytes"] == budget
    p = model.exceedance_probability(daily, 1.0, window="30D", streamed=True, max_bytes=budget)
    assert Spy.calls[-1][0] == "posterior_window_variances" and Spy.calls[-1][1]["max_bytes"] == budget
    assert len(ds["mean"].values) == len(p.values) == 365 - 29 and not _names("posterior_cov") and not _names("window_moments")
    # selection is never automatic: without the keyword nothing streamed ran above, and the windowed counting products, which have
    # no streamed form, keep their text
    with pytest.raises(ValueError, match=r"max_bytes = 1000000$"):
        model.exceedance(daily, threshold=1.0, window="30D", max_bytes=budget)
    with pytest.raises(ValueError, match=r"max_bytes = 1000000$"):
        model.duration_curve(daily, levels=[1.0], window="30D", max_bytes=budget)


def test_refusals_new_and_pinned():
    model, daily = _loadest()
    with pytest.raises(ValueError, match="covariance between outputs.*dense path"):
        model.rolling_mean(daily, "30D", streamed=True, return_cov=True)
    with pytest.raises(ValueError, match="streamed=True applies to the rolling mean"):
        model.exceedance_probability(daily, 1.0, streamed=True)
    with pytest.raises(ValueError, match="noise of an averaged"):
        model.exceedance_probability(daily, 1.0, window="30D", streamed=True, pred_noise=True)
    with pytest.raises(ValueError, match="geometric"):
        _loadest("standard")[0].rolling_mean(daily, "30D", statistic="geometric_mean", streamed=True)
    # the windowed counting products need the full windowed covariance: their refusal stays
    with pytest.raises(NotImplementedError, match="row halo"):
        model.exceedance(daily, threshold=1.0, window="30D", streamed=True)
    with pytest.raises(NotImplementedError, match="row halo"):
        model.duration_curve(daily, levels=[1.0], window="30D", streamed=True)
    assert not Spy.calls


# ------------------------------------------------------------------------------------------------ the library, no device
def _host_plan(lib, n=200, d=3, dtype=_lib.F64):
    """A ``GPPlan`` shell around a C plan without workspace or device: what ``window_panel_rows`` reads."""
    h = C.c_void_p()
    assert lib.dgp_plan_create(_lib.MODEL_LOADEST, dtype, n, d, C.byref(h)) == 0
    plan = object.__new__(GPPlan)
    plan.lib, plan._h = lib, h
    return plan


def test_window_panel_rows_against_a_brute_force_scan():
    lib = _lib.load()
    plan = _host_plan(lib)
    try:
        q = lib.dgp_posterior_window_variances_workspace_bytes
        for m, nq, reach in ((100, 100, 30), (1000, 971, 30), (3000, 2329, 672), (3000, 3000, 3000), (700, 100, 1)):
            M = -(-m // 128) * 128
            sizes = {R: int(q(plan._h, m, nq, reach, R)) for R in range(128, M + 129, 128)}
            assert all(sizes[R] == window_stream_bytes(200, m, 3, nq, reach, 8, R) for R in sizes), (m, nq, reach)
            assert all(sizes[R + 128] > sizes[R] for R in range(128, M, 128)) and sizes[M + 128] == sizes[M]  # capped at M rows
            for budget in (sizes[128], sizes[128] + 1, sizes[M] - 1, sizes[M], 10 * sizes[M], (sizes[128] + sizes[M]) // 2,
                           sizes[min(M, 384)], sizes[min(M, 384)] - 1):
                if budget < sizes[128]:  # (M = 128: the refusal, below)
                    continue
                brute = max(R for R in range(128, M + 1, 128) if sizes[R] <= budget)
                assert plan.window_panel_rows(m, nq, reach, budget) == brute, (m, nq, reach, budget)
            with pytest.raises(ValueError, match=rf"needs a work area of {sizes[128]} bytes.*128 rows.*max_bytes = {sizes[128] - 1}$"):
                plan.window_panel_rows(m, nq, reach, sizes[128] - 1)
        # the band grows quadratically in R: the second difference of the size is 2 x 128 x 128 elements
        s = [int(q(plan._h, 3000, 3000, 30, R)) for R in (128, 256, 384)]
        assert s[2] - 2 * s[1] + s[0] == 8 * 2 * 128 * 128
        with pytest.raises(ValueError, match="bad size"):
            plan.window_panel_rows(0, 10, 5, 1 << 30)
    finally:
        lib.dgp_plan_destroy(plan._h)
        plan._h = None


def test_abi_is_declared_bound_and_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    names = {"dgp_posterior_cov_block", "dgp_posterior_cov_block_workspace_bytes", "dgp_window_variances",
             "dgp_window_variances_workspace_bytes", "dgp_posterior_window_variances", "dgp_posterior_window_variances_workspace_bytes"}
    assert names <= set(_lib.EXT2_SIGNATURES) and not names & set(_lib.SIGNATURES) and not names & set(_lib.EXT_SIGNATURES)
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    ext2 = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "dgp_hip_ext2.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(dgp_[a-z_0-9]+)\s*\(", ext2))
    for name in names:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.EXT2_SIGNATURES[name][1] and fn.restype == _lib.EXT2_SIGNATURES[name][0]
    one = C.c_void_p(256)  # never dereferenced: every call below returns before any launch
    th = (C.c_double * 16)()
    err = lib.dgp_last_error

    # ---- dgp_window_variances: stateless
    wq, wv = lib.dgp_window_variances_workspace_bytes, lib.dgp_window_variances
    assert wq(385, 385, 1) == 8 * (3 * 512 + 3 * 512) + 256 and wq(385, 100, 3) == 8 * 3 * (3 * 512 + 3 * 128) + 256
    assert wq(0, 1, 1) == 0 and wq(1, 0, 1) == 0 and wq(1, 1, 0) == 0 and wq((1 << 20) + 1, 1, 1) == 0 and wq(1, 1, 1025) == 0
    ok = (_lib.F64, 1, one, 100, 1, one, one, None, one, one, 50, one, 0, one, one, None)  # (no work area: refused at the latest there)

    def call_wv(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return wv(*a)

    for i in (2, 5, 6, 8, 9, 13, 14):  # cov, mu, scale2 (mode 1), lo, hi, mean_out, var_out
        assert call_wv(**{f"a{i}": None}) == _lib.E_ARG and b"null" in err(), i
    assert call_wv(a1=0, a6=None) == _lib.E_WORKSPACE  # mode 0 needs no scale2: the next check is the work area (below)
    assert call_wv(a0=2) == _lib.E_ARG and b"dtype" in err()
    assert call_wv(a1=2) == _lib.E_ARG and b"mode" in err()
    for kw in (dict(a3=0), dict(a10=0), dict(a4=0), dict(a4=1025), dict(a3=(1 << 20) + 1)):
        assert call_wv(**kw) == _lib.E_ARG and b"size" in err(), kw
    assert call_wv(a11=None) == _lib.E_WORKSPACE and call_wv(a12=wq(100, 50, 1) - 1) == _lib.E_WORKSPACE and b"workspace" in err()
    assert call_wv(a11=C.c_void_p(260), a12=1 << 30) == _lib.E_ARG and b"aligned" in err()

    # ---- the plan entries
    bq, bk = lib.dgp_posterior_cov_block_workspace_bytes, lib.dgp_posterior_cov_block
    pq, pw = lib.dgp_posterior_window_variances_workspace_bytes, lib.dgp_posterior_window_variances
    assert bq(None, 385, 0, 128, 0) == 0 and pq(None, 385, 385, 30, 128) == 0
    assert bk(None, th, one, 385, 0, 128, 0, one, 1 << 30, one, None) == _lib.E_ARG and b"null plan" in err()
    assert pw(None, th, one, 385, one, one, None, one, one, 385, 0, 30, 128, one, 1 << 30, one, one, None) == _lib.E_ARG
    h = C.c_void_p()
    assert lib.dgp_plan_create(_lib.MODEL_LOADEST, _lib.F64, 150, 2, C.byref(h)) == 0
    try:
        assert bq(h, 385, 0, 128, 0) == bq(h, 385, 256, 512, 128) > 0
        for block in ((0, 128, 64), (64, 128, 0), (0, 100, 0), (128, 128, 0), (256, 128, 0), (128, 256, 256), (0, 640, 0), (-128, 128, -128)):
            assert bq(h, 385, *block) == 0, block
            assert bk(h, th, one, 385, *block, one, 1 << 30, one, None) == _lib.E_ARG and b"bad block" in err(), block
        assert bq(h, 0, 0, 128, 0) == 0
        for i in (1, 2, 9):  # theta, Xs, out
            a = [h, th, one, 385, 0, 128, 0, one, 1 << 30, one, None]
            a[i] = None
            assert bk(*a) == _lib.E_ARG and b"null" in err(), i
        assert bk(h, th, one, 385, 0, 128, 0, one, 1 << 30, one, None) == _lib.E_STATE and b"factorisation" in err()

        assert pq(h, 385, 385, 30, 128) == window_stream_bytes(150, 385, 2, 385, 30, 8, 128)
        assert pq(h, 385, 385, 30, 1024) == pq(h, 385, 385, 30, 512)  # M = 512: the panel is capped at M
        for bad in (dict(m=0), dict(q=0), dict(reach=0), dict(reach=(1 << 20) + 1), dict(R=0), dict(R=64), dict(R=200), dict(R=-128)):
            s = {**dict(m=385, q=385, reach=30, R=128), **bad}
            assert pq(h, s["m"], s["q"], s["reach"], s["R"]) == 0, bad
        okp = (h, th, one, 385, one, one, None, one, one, 385, 1, 30, 128, one, 1 << 30, one, one, None)

        def call_pw(**kw):
            a = list(okp)
            for i, v in kw.items():
                a[int(i[1:])] = v
            return pw(*a)

        for i in (1, 2, 4, 5, 7, 8, 15, 16):  # theta, Xs, mu, scale2 (mode 1), lo, hi, mean_out, var_out
            assert call_pw(**{f"a{i}": None}) == _lib.E_ARG and b"null" in err(), i
        assert call_pw(a10=2) == _lib.E_ARG and b"mode" in err()
        assert call_pw(a3=0) == _lib.E_ARG and call_pw(a9=0) == _lib.E_ARG and b"size" in err()
        for reach in (0, -5, (1 << 20) + 1):
            assert call_pw(a11=reach) == _lib.E_ARG and b"reach" in err()
        for rows in (0, 64, 129, -128):
            assert call_pw(a12=rows) == _lib.E_ARG and b"panel_rows" in err()
        assert call_pw() == _lib.E_STATE and b"factorisation" in err()  # nothing factorised yet
        assert call_pw(a10=0, a5=None) == _lib.E_STATE  # mode 0 needs no scale2
    finally:
        lib.dgp_plan_destroy(h)
