"""The streamed exceedance path (``streamed=True`` of ``exceedance`` / ``duration_curve`` / ``LoadestGP.exceedance(kind="flux")``)
on CPU, with the device plan replaced by the oracle-backed double of tests/exceedance_stream_helpers.py: the host logic of
the two paths gives the same statistics (1e-12: both doubles answer from the same oracle posterior, the streamed one takes
its mean from ``predict_mean`` and a symmetric covariance, the dense one the ``posterior_cov`` buffer's lower triangle),
selection is never automatic, the byte budget picks the panel by ``backend.stream_panel_rows``, and the new C entry refuses
bad arguments before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib, backend
from discontinuum_amd import exceedance as ex
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.rating_gp import RatingGP
from tests.exceedance_stream_helpers import StreamOraclePlan, stream_bytes
from tests.flux_helpers import daily_loadest, daily_rating


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(StreamOraclePlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)
    StreamOraclePlan.streamed_calls = []
    StreamOraclePlan.dense_calls = []


_MODELS = {}


def _loadest():
    if "loadest" not in _MODELS:
        cov_obs, target, daily = daily_loadest(seed=0, end="2014-01-01")
        model = LoadestGP()
        model.fit(cov_obs, target, iterations=10)
        _MODELS["loadest"] = (model, daily)
    return _MODELS["loadest"]


def _rating():
    if "rating" not in _MODELS:
        cov_obs, target, unc, daily = daily_rating(end="2013-07-01")
        model = RatingGP()
        model.fit(cov_obs, target, target_unc=unc, iterations=10)
        _MODELS["rating"] = (model, daily)
    return _MODELS["rating"]


def _same(a, b, names=("mean", "se", "lower", "upper")):
    for k in names:
        x, y = np.asarray(a[k].values, dtype=np.float64), np.asarray(b[k].values, dtype=np.float64)
        assert x.shape == y.shape and np.all(np.abs(x - y) <= 1e-12 * np.maximum(1.0, np.abs(y))), (k, float(np.abs(x - y).max()))


@pytest.mark.parametrize("above,fraction", [(True, False), (False, False), (True, True), (False, True)])
def test_streamed_exceedance_equals_the_dense_host_path(above, fraction):
    model, daily = _loadest()
    kw = dict(threshold=[0.9, 1.3], freq="YE", above=above, fraction=fraction, pred_noise=True, return_cov=True)
    dense, dcov = model.exceedance(daily, **kw)
    assert not StreamOraclePlan.streamed_calls and len(StreamOraclePlan.dense_calls) == 1
    streamed, scov = model.exceedance(daily, streamed=True, **kw)
    assert len(StreamOraclePlan.streamed_calls) == 1 and len(StreamOraclePlan.dense_calls) == 1
    _same(streamed, dense)
    assert np.array_equal(streamed["n_points"].values, dense["n_points"].values)
    assert np.abs(scov - dcov).max() <= 1e-12 * max(1.0, np.abs(dcov).max())


def test_streamed_flux_exceedance_equals_the_dense_host_path():
    model, daily = _loadest()
    dense = model.exceedance(daily, threshold=[300.0, 900.0], kind="flux")
    streamed = model.exceedance(daily, threshold=[300.0, 900.0], kind="flux", streamed=True)
    assert len(StreamOraclePlan.streamed_calls) == 1 and len(StreamOraclePlan.dense_calls) == 1
    _same(streamed, dense)


@pytest.mark.parametrize("above", [True, False])
def test_streamed_duration_curve_equals_the_dense_host_path(above):
    model, daily = _rating()
    dense = model.duration_curve(daily, above=above)
    streamed = model.duration_curve(daily, above=above, streamed=True)
    assert [c["levels"] for c in StreamOraclePlan.streamed_calls] == [21] and len(StreamOraclePlan.dense_calls) == 1
    _same(streamed, dense)
    assert np.array_equal(streamed["level"].values, dense["level"].values)


def test_more_than_64_levels_go_in_several_streamed_calls():
    model, daily = _rating()
    levels = np.linspace(1.5, 30.0, 70)
    dense = ex.duration_curve(model, daily, levels=levels)
    streamed = ex.duration_curve(model, daily, levels=levels, streamed=True)
    assert [c["levels"] for c in StreamOraclePlan.streamed_calls] == [64, 6]
    _same(streamed, dense)


def test_the_default_path_makes_no_streamed_call_and_over_budget_still_raises():
    model, daily = _loadest()
    model.exceedance(daily, threshold=1.0)
    model.duration_curve(daily, levels=[1.0])
    assert not StreamOraclePlan.streamed_calls and len(StreamOraclePlan.dense_calls) == 2
    with pytest.raises(ValueError, match=r"footprint of \d+ bytes.*max_bytes = 1000000; pass streamed=True"):
        model.exceedance(daily, threshold=1.0, max_bytes=1_000_000)
    with pytest.raises(ValueError, match=r"footprint of \d+ bytes.*max_bytes = 1000000; pass streamed=True"):
        model.duration_curve(daily, levels=[1.0], max_bytes=1_000_000)
    assert not StreamOraclePlan.streamed_calls and len(StreamOraclePlan.dense_calls) == 2  # selection is never automatic


def test_streamed_budget_picks_the_panel_and_a_budget_below_128_rows_raises():
    model, daily = _loadest()
    m, n, d = len(daily.coords["time"].values), model.dm.X.shape[0], model.dm.X.shape[1]
    M = -(-m // 128) * 128
    assert M >= 512
    size = lambda R: stream_bytes(n, m, d, 2, 1, 8, R)  # noqa: E731  (two years, one level, float64)
    step = size(256) - size(128)
    assert step == 8 * 128 * M and size(384) - size(256) == step and size(M + 128) == size(M)
    dense = model.exceedance(daily, threshold=1.0)
    for budget, rows in ((size(128), 128), (size(128) + step - 1, 128), (size(256), 256), (size(384) + 5, 384), (size(M), M),
                         (size(M) + 10 * step, M)):
        StreamOraclePlan.streamed_calls = []
        got = model.exceedance(daily, threshold=1.0, streamed=True, max_bytes=budget)
        call, = StreamOraclePlan.streamed_calls
        assert call["panel_rows"] == rows and call["bytes"] <= budget and call["max_bytes"] == budget, (budget, call)
        _same(got, dense)
    StreamOraclePlan.streamed_calls = []
    with pytest.raises(ValueError, match=rf"work area of {size(128)} bytes.*128 rows.*max_bytes = {size(128) - 1}"):
        model.exceedance(daily, threshold=1.0, streamed=True, max_bytes=size(128) - 1)
    assert not StreamOraclePlan.streamed_calls


def test_stream_panel_rows_is_the_documented_function():
    f = backend.stream_panel_rows
    assert f(1000, 100, 1280, 1000) == 128 and f(1000, 100, 1280, 1099) == 128 and f(1000, 100, 1280, 1100) == 256
    assert f(1000, 100, 1280, 1000 + 9 * 100) == 1280 and f(1000, 100, 1280, 10 ** 12) == 1280
    assert f(1000, 0, 128, 1000) == 128  # one block: nothing to grow
    for need, step, M, budget in ((12345, 777, 128 * 40, 30000), (5, 3, 128 * 7, 11), (10 ** 9, 10 ** 6, 128 * 1100, 16 * 2 ** 30)):
        R = f(need, step, M, budget)
        assert R % 128 == 0 and 128 <= R <= M and need + (R // 128 - 1) * step <= budget
        assert R == M or need + (R // 128) * step > budget  # the next panel size would not fit
    with pytest.raises(ValueError, match=r"1001 bytes.*max_bytes = 1000"):
        f(1001, 100, 1280, 1000)


# ------------------------------------------------------------------------------------------------ the C entry, no device
def test_abi_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    q = lib.dgp_posterior_exceedance_moments_workspace_bytes
    f = lib.dgp_posterior_exceedance_moments
    assert q(None, 100, 2, 1, 128) == 0
    one = C.c_void_p(256)  # never dereferenced: every call below returns before any launch
    th = (C.c_double * 8)()
    assert f(None, th, one, 100, one, one, 1, one, one, 2, None, 128, one, 1 << 20, one, one, None) == -1
    h = C.c_void_p()
    assert lib.dgp_plan_create(_lib.MODEL_LOADEST, _lib.F64, 200, 3, C.byref(h)) == 0
    try:
        assert q(h, 100, 2, 1, 128) > 0 and q(h, 100, 2, 1, 256) == q(h, 100, 2, 1, 128)  # M = 128: the panel is capped at M
        assert q(h, 300, 2, 1, 256) - q(h, 300, 2, 1, 128) == 8 * 128 * 384
        for m, P, L, R in ((100, 2, 1, 128), (300, 2, 1, 256), (1000, 31, 21, 768), (1000, 1, 64, 4096)):
            assert q(h, m, P, L, R) == stream_bytes(200, m, 3, P, L, 8, R), (m, P, L, R)  # the host's formula
        for bad_rows in (0, -128, 64, 200):
            assert q(h, 100, 2, 1, bad_rows) == 0
        assert q(h, 0, 2, 1, 128) == 0 and q(h, 100, 0, 1, 128) == 0 and q(h, 100, 2, 0, 128) == 0 and q(h, 100, 2, 65, 128) == 0
        ok = (h, th, one, 100, one, one, 1, one, one, 2, None, 128, one, 1 << 30, one, one, None)

        def call(**kw):
            a = list(ok)
            for i, v in kw.items():
                a[int(i[1:])] = v
            return f(*a)

        for i in (1, 2, 4, 5, 7, 8, 14, 15):  # theta, Xs, mu, thresh, w, group, mean_out, cov_out
            assert call(**{f"a{i}": None}) == -1, i
        for L in (0, 65, -1):
            assert call(a6=L) == -1
        for rows in (0, 64, 129, -128):
            assert call(a11=rows) == -1
        assert call(a3=0) == -1 and call(a9=0) == -1
        assert call() == -4 and b"factorisation" in lib.dgp_last_error()  # DGP_E_STATE: nothing factorised yet
    finally:
        lib.dgp_plan_destroy(h)
