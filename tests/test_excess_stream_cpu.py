"""The streamed threshold excess (``streamed=True`` of ``excess`` / ``excess_load``) on CPU, with the device plan replaced by an
oracle-backed double that records what it is handed: the streamed branch reaches ``posterior_excess_moments`` once per 64
levels with the mapped mean, s^2, ln tau and ``above`` passed through and never forms the dense covariance, the default path is
what it was, selection is never automatic, linear targets are refused on both paths, ``stream_panel_rows`` names the pass, and
the two new C entries are bound through ``EXT2_SIGNATURES`` and refuse bad arguments before any launch."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from discontinuum_amd import _lib, backend
from discontinuum_amd import excess as xs
from discontinuum_amd.engines.base import ModelConfig
from discontinuum_amd.engines.hip import MarginalHIP
from discontinuum_amd.loadest_gp import LoadestGP
from discontinuum_amd.loads import flux_weights, period_groups, target_transform
from discontinuum_amd.rating_gp import RatingGP
from oracle import gp_oracle as orc
from tests.excess_helpers import ExcessOraclePlan, dense_excess_moments
from tests.excess_stream_helpers import excess_stream_bytes
from tests.flux_helpers import daily_loadest, daily_rating


class StreamSpyPlan(ExcessOraclePlan):
    """Records the calls of the dense pair (``posterior_cov``, ``excess_moments``) and of ``posterior_excess_moments``, which it
    answers by the dense reference on the oracle's symmetric posterior covariance."""

    streamed: list = []
    dense: list = []
    cov_calls: list = []

    def posterior_cov(self, theta, Xs):
        StreamSpyPlan.cov_calls.append(int(Xs.shape[0]))
        return super().posterior_cov(theta, Xs)

    def excess_moments(self, cov, m, mu, scale2, thresh, w, groups, ngroups, above=True, extra_var=None):
        StreamSpyPlan.dense.append(dict(m=m, levels=int(torch.as_tensor(thresh).shape[0]), above=above))
        return super().excess_moments(cov, m, mu, scale2, thresh, w, groups, ngroups, above, extra_var)

    def posterior_excess_moments(self, theta, Xs, mu, scale2, thresh, w, groups, ngroups, above=True, extra_var=None,
                                 panel_rows=None, max_bytes=None):
        host = lambda v: None if v is None else torch.as_tensor(v).detach().cpu().double().numpy().copy()  # noqa: E731
        StreamSpyPlan.streamed.append(dict(m=int(Xs.shape[0]), mu=host(mu), scale2=float(scale2), thresh=host(thresh), w=host(w),
                                           groups=host(groups), ngroups=ngroups, above=above, extra_var=host(extra_var),
                                           panel_rows=panel_rows, max_bytes=max_bytes))
        th, r, noise = self._state
        _kmean, cov = orc.posterior(self.model, self.X, r, noise, th, Xs.double(), full_cov=True)
        Cs = cov.numpy()
        mean, pc, total = dense_excess_moments(0.5 * (Cs + Cs.T), host(mu), float(scale2), host(thresh), host(w), host(groups), ngroups,
                                               above, host(extra_var))
        return torch.tensor(mean), torch.tensor(pc), torch.tensor(total)


@pytest.fixture(autouse=True)
def cpu_engine(monkeypatch):
    monkeypatch.setattr(MarginalHIP, "_plan_factory", staticmethod(StreamSpyPlan))
    monkeypatch.setattr(MarginalHIP, "device", "cpu")
    torch.manual_seed(0)
    StreamSpyPlan.streamed, StreamSpyPlan.dense, StreamSpyPlan.cov_calls = [], [], []


_MODELS = {}
SPAN = dict(start="2012-06-01", end="2013-06-01")  # one year of days in two calendar years: m = 365, two periods


def _loadest(transform="log"):
    key = ("loadest", transform)
    if key not in _MODELS:
        cov_obs, target, daily = daily_loadest(n_obs=40, **SPAN)
        model = LoadestGP() if transform == "log" else LoadestGP(model_config=ModelConfig(transform=transform))
        model.fit(cov_obs, target, iterations=10)
        _MODELS[key] = (model, daily)
    return _MODELS[key]


def _rating():
    if "rating" not in _MODELS:
        cov_obs, target, unc, daily = daily_rating(n_obs=30, **SPAN)
        model = RatingGP()
        model.fit(cov_obs, target, target_unc=unc, iterations=10)
        _MODELS["rating"] = (model, daily)
    return _MODELS["rating"]


def _same(a, b, names=("mean", "se", "lower", "upper", "total", "share")):
    """1e-10 relative: both doubles answer from the same oracle posterior, which repeats to about 1e-10 (the streamed one takes
    a symmetrised covariance and the mean of ``predict_mean``, the dense one the ``posterior_cov`` buffer's lower triangle)."""
    for k in names:
        x, y = np.asarray(a[k].values, dtype=np.float64), np.asarray(b[k].values, dtype=np.float64)
        assert x.shape == y.shape and np.allclose(x, y, rtol=1e-10, atol=0), (k, float(np.abs(x - y).max()))


# ------------------------------------------------------------------------------------------------ the host product
@pytest.mark.parametrize("above", [True, False])
def test_streamed_excess_hands_the_mapped_mean_and_never_forms_the_covariance(above):
    model, daily = _loadest()
    m = len(daily.coords["time"].values)
    tau = [0.9, 1.2]
    dense, dcov = model.excess(daily, threshold=tau, above=above, return_cov=True)
    assert not StreamSpyPlan.streamed and len(StreamSpyPlan.dense) == 1 and StreamSpyPlan.cov_calls == [m]  # the default path
    ds, scov = model.excess(daily, threshold=tau, above=above, return_cov=True, streamed=True, max_bytes=123_456_789)
    assert len(StreamSpyPlan.streamed) == 1 and len(StreamSpyPlan.dense) == 1 and StreamSpyPlan.cov_calls == [m]  # no posterior_cov
    call = StreamSpyPlan.streamed[-1]
    _mode, s, t = target_transform(model.dm)
    x = torch.tensor(model.dm.Xnew(daily), dtype=torch.float64)
    latent = (model._plan.predict_mean(model._factor_theta, x) + model.model.prior_mean(x)).detach().numpy()
    assert np.allclose(call["mu"], s * latent + t, rtol=1e-8, atol=0) and call["scale2"] == s * s
    assert np.array_equal(call["thresh"], np.log(np.broadcast_to(np.array(tau)[:, None], (2, m))))
    assert call["above"] is above and call["extra_var"] is None and call["panel_rows"] is None and call["max_bytes"] == 123_456_789
    _o, groups, labels, _n, _d = period_groups(daily.coords["time"].values, np.ones(m), "YE")
    assert np.array_equal(call["groups"], groups) and call["ngroups"] == len(labels) == 2 and np.array_equal(call["w"], np.ones(m))
    assert set(ds) == set(dense) and ds.attrs == dense.attrs and scov.shape == (2, 2, 2)
    _same(ds, dense)
    assert np.allclose(scov, dcov, rtol=1e-9, atol=0) and np.array_equal(ds["n_points"].values, dense["n_points"].values)


def test_streamed_excess_load_and_rating_deficit_volume():
    model, daily = _loadest()
    wf = flux_weights(daily, {"units": "mg/l"})
    limit = float(np.median(wf)) * 1.1
    dense = model.excess_load(daily, limit=limit)
    streamed = model.excess_load(daily, limit=limit, streamed=True)
    call = StreamSpyPlan.streamed[-1]
    assert np.array_equal(call["thresh"], np.log(limit / wf)[None, :]) and np.array_equal(call["w"], wf) and call["above"] is True
    assert streamed["mean"].attrs["units"] == "kilograms"
    _same(streamed, dense)
    rating, rdaily = _rating()
    m = len(rdaily.coords["time"].values)
    seconds = np.full(m, 86400.0)
    low = 2.0
    dense = rating.excess(rdaily, threshold=low, weights=seconds, above=False)
    n_cov = len(StreamSpyPlan.cov_calls)
    streamed = rating.excess(rdaily, threshold=low, weights=seconds, above=False, streamed=True)
    assert StreamSpyPlan.streamed[-1]["above"] is False and len(StreamSpyPlan.cov_calls) == n_cov
    _same(streamed, dense)
    # predictive noise goes into the variances (model space), as on the dense path: a larger deficit
    noisy = rating.excess(rdaily, threshold=low, weights=seconds, above=False, streamed=True, pred_noise=True)
    extra = StreamSpyPlan.streamed[-1]["extra_var"]
    assert extra is not None and extra.shape == (m,) and np.all(extra > 0) and np.all(noisy["mean"].values > streamed["mean"].values)
    _same(noisy, rating.excess(rdaily, threshold=low, weights=seconds, above=False, pred_noise=True))


def test_more_than_64_levels_go_in_several_streamed_calls():
    model, daily = _rating()
    levels = np.linspace(1.5, 30.0, 70)
    ds = model.excess(daily, threshold=levels, streamed=True)
    assert [c["thresh"].shape[0] for c in StreamSpyPlan.streamed] == [64, 6] and not StreamSpyPlan.cov_calls and not StreamSpyPlan.dense
    assert ds["mean"].values.shape == (70, 2) and np.array_equal(StreamSpyPlan.streamed[1]["thresh"][:, 0], np.log(levels[64:]))
    assert np.all(np.diff(ds["mean"].values, axis=0) <= 0)


def test_selection_is_never_automatic_and_linear_targets_are_refused_on_both_paths():
    model, daily = _loadest()
    with pytest.raises(NotImplementedError, match=r"footprint of \d+ bytes.*max_bytes = 1000000.*no streamed form") as e:
        model.excess(daily, threshold=1.0, max_bytes=1_000_000)
    assert "streamed=True" in str(e.value)
    with pytest.raises(NotImplementedError, match=r"footprint of \d+ bytes.*streamed=True"):
        model.excess_load(daily, criterion=1.0, max_bytes=1_000_000)
    assert not StreamSpyPlan.streamed and not StreamSpyPlan.dense and not StreamSpyPlan.cov_calls
    linear, daily = _loadest("standard")
    for streamed in (False, True):
        with pytest.raises(NotImplementedError, match="log targets only"):
            linear.excess(daily, threshold=1.0, streamed=streamed)
        with pytest.raises(NotImplementedError, match="log targets only"):
            linear.excess_load(daily, limit=10.0, streamed=streamed)
        with pytest.raises(NotImplementedError, match="log targets only"):
            xs.excess_sums(linear, torch.zeros(3, 3, dtype=torch.float64), np.zeros((1, 3)), np.ones(3), np.zeros(3, np.int32), 1,
                           streamed=streamed)
    assert not StreamSpyPlan.streamed and not StreamSpyPlan.dense and not StreamSpyPlan.cov_calls


def test_stream_panel_rows_names_the_pass():
    f = backend.stream_panel_rows
    assert f(1000, 100, 1280, 1100, "the streamed excess pass") == 256 == f(1000, 100, 1280, 1100)
    with pytest.raises(ValueError, match=r"^the streamed excess pass needs a work area of 1001 bytes.*128 rows.*max_bytes = 1000$"):
        f(1001, 100, 1280, 1000, "the streamed excess pass")
    with pytest.raises(ValueError, match=r"^the streamed exceedance pass needs a work area of 1001 bytes with the smallest panel "
                                         r"\(128 rows\), which exceeds max_bytes = 1000$"):
        f(1001, 100, 1280, 1000)


# ------------------------------------------------------------------------------------------------ the C entries, no device
def test_abi_is_declared_bound_and_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    names = {"dgp_posterior_excess_moments_workspace_bytes", "dgp_posterior_excess_moments"}
    assert names <= set(_lib.EXT2_SIGNATURES) and not names & set(_lib.SIGNATURES) and not names & set(_lib.EXT_SIGNATURES)
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    ext2 = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "dgp_hip_ext2.h")).read(), flags=re.S)
    assert names <= set(re.findall(r"\b(dgp_[a-z_0-9]+)\s*\(", ext2))
    main = open(os.path.join(inc, "dgp_hip.h")).read()
    assert main.count('#include "dgp_hip_ext2.h"') == 1 and main.index('#include "dgp_hip_ext2.h"') < main.rindex("}")
    for name in names:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.EXT2_SIGNATURES[name][1] and fn.restype == _lib.EXT2_SIGNATURES[name][0]
    q = lib.dgp_posterior_excess_moments_workspace_bytes
    f = lib.dgp_posterior_excess_moments
    assert q(None, 100, 2, 1, 128) == 0
    one = C.c_void_p(256)  # never dereferenced: every call below returns before any launch
    th = (C.c_double * 8)()
    assert f(None, th, one, 100, one, one, one, 1, one, one, 2, None, 1, 128, one, 1 << 20, one, one, one, None) == -1
    h = C.c_void_p()
    assert lib.dgp_plan_create(_lib.MODEL_LOADEST, _lib.F64, 200, 3, C.byref(h)) == 0
    try:
        assert q(h, 100, 2, 1, 128) > 0 and q(h, 100, 2, 1, 256) == q(h, 100, 2, 1, 128)  # M = 128: the panel is capped at M
        assert q(h, 300, 2, 1, 256) - q(h, 300, 2, 1, 128) == 8 * 128 * 384
        for m, P, L, R in ((100, 2, 1, 128), (300, 2, 1, 256), (1000, 31, 21, 768), (1000, 1, 64, 4096), (700, 3, 9, 256)):
            assert q(h, m, P, L, R) == excess_stream_bytes(200, m, 3, P, L, 8, R), (m, P, L, R)  # the host's formula
        for bad_rows in (0, -128, 64, 200):
            assert q(h, 100, 2, 1, bad_rows) == 0
        assert q(h, 0, 2, 1, 128) == 0 and q(h, 100, 0, 1, 128) == 0 and q(h, 100, 2, 0, 128) == 0 and q(h, 100, 2, 65, 128) == 0
        ok = (h, th, one, 100, one, one, one, 1, one, one, 2, None, 1, 128, one, 1 << 30, one, one, one, None)

        def call(**kw):
            a = list(ok)
            for i, v in kw.items():
                a[int(i[1:])] = v
            return f(*a)

        for i in (1, 2, 4, 5, 6, 8, 9, 16, 17, 18):  # theta, Xs, mu, scale2, thresh, w, group, mean_out, cov_out, total_out
            assert call(**{f"a{i}": None}) == -1 and b"null" in lib.dgp_last_error(), i
        for L in (0, 65, -1):
            assert call(a7=L) == -1 and b"size" in lib.dgp_last_error()
        for rows in (0, 64, 129, -128):
            assert call(a13=rows) == -1 and b"panel_rows" in lib.dgp_last_error()
        for above in (-1, 2):
            assert call(a12=above) == -1 and b"above" in lib.dgp_last_error()
        assert call(a3=0) == -1 and call(a10=0) == -1
        assert call() == -4 and b"factorisation" in lib.dgp_last_error()  # DGP_E_STATE: nothing factorised yet
    finally:
        lib.dgp_plan_destroy(h)
