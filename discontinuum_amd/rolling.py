"""Exact rolling-window statistics of a fitted model's posterior: n-day means with their uncertainty, and the windows the
exceedance products count on -- the 30-day geometric mean of a bacteria record, 4-day and 30-day average chronic criteria,
7-day mean flows of a stage record.

The reference can only roll draws: ``sim = model.sample(daily, n)``, a rolling mean of every draw, its spread.  A rolling
mean in MODEL space is a linear functional of the latent f ~ N(mu, C): with W the (q, m) banded row-stochastic window
matrix,

    W f ~ N(W mu, W C W^T),

exactly Gaussian -- for a log target this is the rolling GEOMETRIC mean, exp(s (W f)_i + t).  The banded product W C W^T
is one ``dgp_window_moments`` pass over the covariance ``dgp_posterior_cov`` writes, and its result has that covariance's
layout, so ``dgp_exceedance_moments`` counts the days on which the rolling mean exceeds a criterion straight from it.  The
ARITHMETIC n-day mean of a log target is a sum of lognormals: its mean and standard error are exact (mode 1 of the pass),
its interval is the approximate rule ``loads.intervals`` uses for period sums.
"""
from __future__ import annotations

import numpy as np
import pandas as pd
import torch
from scipy.stats import norm

from .backend import MODE_LINEAR, MODE_LOG
from .loads import DEFAULT_MAX_BYTES, _site_bytes, _target_attrs, intervals, target_transform
from .xr_compat import Dataset


def _window_ns(window) -> int:
    """A pandas-style offset ("30D", "96h") or a ``numpy.timedelta64`` -> nanoseconds (> 0)."""
    try:
        ns = int(pd.Timedelta(window).value)
    except (ValueError, TypeError) as e:
        raise ValueError(f"window must be a fixed offset such as '30D' or a numpy.timedelta64, not {window!r}") from e
    if ns <= 0:
        raise ValueError(f"window must be positive, not {window!r}")
    return ns


def time_windows(time, window, align="right", min_periods=None, valid=None):
    """Index windows over a record by TIME, so that gaps and irregular records are handled.

    ``window``: a pandas-style offset ("30D", "7D", "96h") or a ``numpy.timedelta64``; ``align="right"``: window i covers
    (t_i - window, t_i], the trailing window regulators use; ``"center"``: [t_i - window / 2, t_i + window / 2).  Points with
    a non-finite time -- or marked False in ``valid`` (a missing covariate) -- are dropped.  ``min_periods``: the point
    count a window needs to qualify; None means the largest count any window of the record holds (30 for a gap-free daily
    record and "30D": leading partial windows and windows over gaps are excluded).
    -> (order, lo, hi, keep): ``order`` sorts the kept points by time (stable); window i of the sorted points is
    ``lo[i] <= j < hi[i]`` (int32, both non-decreasing); ``keep`` marks the outputs that qualify."""
    if align not in ("right", "center"):
        raise ValueError(f"align must be 'right' or 'center', not {align!r}")
    W = _window_ns(window)
    t = np.asarray(time).reshape(-1).astype("datetime64[ns]")
    ok = ~np.isnat(t)
    if valid is not None:
        ok &= np.asarray(valid, dtype=bool).reshape(-1)
    idx = np.nonzero(ok)[0]
    if idx.size == 0:
        raise ValueError("no point has a finite time and covariates")
    ti = t[idx].astype(np.int64)
    srt = np.argsort(ti, kind="stable")
    order, ts = idx[srt], ti[srt]
    if align == "right":
        lo, hi = np.searchsorted(ts, ts - W, side="right"), np.searchsorted(ts, ts, side="right")
    else:  # in half-nanoseconds, so that an odd window splits exactly
        lo, hi = np.searchsorted(2 * ts, 2 * ts - W, side="left"), np.searchsorted(2 * ts, 2 * ts + W, side="left")
    count = hi - lo
    need = int(count.max()) if min_periods is None else int(min_periods)
    if need < 1:
        raise ValueError("min_periods must be at least 1")
    return order, lo.astype(np.int32), hi.astype(np.int32), count >= need


def window_bytes(m, q):
    """Device bytes a windowed product adds to the dense footprint for one site: the (Q, Q) float64 result and the pass's
    work area of M Q + 2 M + 2 Q doubles (M, Q the padded sizes)."""
    M, Q = -(-m // 128) * 128, -(-q // 128) * 128
    return 8 * (M * Q + Q * Q) + 8 * (2 * M + 2 * Q)


def record_windows(model, covariates, window, align="right", min_periods=None):
    """The windows of a covariates record: -> (Xnew (m, d) tensor of the kept points in time order, their times (m,),
    lo, hi (q,) of the QUALIFYING outputs only, and ``out`` (q,): the sorted-point index each output sits on)."""
    time = np.asarray(covariates.coords["time"].values).reshape(-1)
    Xall = np.asarray(model.dm.Xnew(covariates))
    order, lo, hi, keep = time_windows(time, window, align, min_periods, valid=np.all(np.isfinite(Xall), axis=1))
    out = np.nonzero(keep)[0]
    if out.size == 0:
        raise ValueError(f"no window of the record holds min_periods = {min_periods} points")
    Xnew = torch.tensor(Xall[order], dtype=model.dtype)
    return Xnew, time[order].astype("datetime64[ns]"), np.ascontiguousarray(lo[out]), np.ascontiguousarray(hi[out]), out


def check_window_budget(model, m, q, extra_bytes, max_bytes, what, streamable=False):
    """``ValueError`` naming the bytes when the dense footprint plus the windowed product's own exceeds ``max_bytes``;
    ``streamable``: the product has a streamed form, and the text ends by naming it."""
    esz = torch.empty((), dtype=model.dtype).element_size()
    need = _site_bytes(model.dm.X.shape[0], m, esz) + window_bytes(m, q) + int(extra_bytes)
    if need > max_bytes:
        raise ValueError(f"{what} needs the dense posterior covariance and its windowed product: a footprint of {need} bytes for "
                         f"m = {m} points and {q} windows exceeds max_bytes = {max_bytes}" + ("; pass streamed=True" if streamable else ""))


def streamed_window_variances(model, Xnew, lo, hi, mode=MODE_LINEAR, s=1.0, t=0.0, max_bytes: int = DEFAULT_MAX_BYTES):
    """The streamed core of ``rolling_mean`` and ``exceedance_probability(window=)``: the latent mean from ``predict_mean``
    (as ``exceedance.count_moments``' streamed branch takes it), then ONE ``posterior_window_variances``, whose work area --
    with the tallest band panel that fits -- ``max_bytes`` bounds.  ``mode`` = MODE_LOG maps the mean by s mu + t first.
    -> numpy (mean (q,), var (q,))."""
    model._eval_ready(Xnew)
    with torch.no_grad():
        mu = (model._plan.predict_mean(model._factor_theta, Xnew) + model.model.prior_mean(Xnew)).contiguous()
        lo_t, hi_t = torch.from_numpy(np.ascontiguousarray(lo)), torch.from_numpy(np.ascontiguousarray(hi))
        if mode == MODE_LOG:
            mean_d, var_d = model._plan.posterior_window_variances(model._factor_theta, Xnew, (s * mu + t).contiguous(), lo_t, hi_t,
                                                                   mode=MODE_LOG, scale2=s * s, max_bytes=max_bytes)
        else:
            mean_d, var_d = model._plan.posterior_window_variances(model._factor_theta, Xnew, mu, lo_t, hi_t, mode=MODE_LINEAR,
                                                                   max_bytes=max_bytes)
    return mean_d.double().cpu().numpy(), var_d.double().cpu().numpy()


def rolling_mean(model, covariates, window, statistic=None, align="right", min_periods=None, ci=0.95, return_cov=False,
                 max_bytes: int = DEFAULT_MAX_BYTES, streamed=False):
    """``MarginalHIP.rolling_mean``: the rolling-window mean of the target over the record ``covariates`` with its exact
    uncertainty, from one ``posterior_cov`` and one ``window_moments``.

    ``statistic=None`` picks the model-space mean: ``"geometric_mean"`` for a log target -- exp(s (W mu)_i + t), with the
    EXACT ``ci`` interval through the monotone map and the lognormal's ``se`` as ``predict`` reports it -- and ``"mean"``
    for a linear one.  ``statistic="mean"`` on a log target is the ARITHMETIC n-day mean: mean and se exact (mode 1 of the
    pass), ``lower`` / ``upper`` APPROXIMATE (``loads.intervals``' lognormal with the same two moments; the attrs say so).
    ``window``, ``align``, ``min_periods``: see ``time_windows``.
    -> Dataset on the qualifying outputs' ``time`` with ``mean``, ``se``, ``lower``, ``upper`` and ``n_points``; with
    ``return_cov`` also the (q, q) covariance -- of the model-space means for the model-space statistic, of the data-space
    means for the arithmetic one.  A record over ``max_bytes`` raises ``ValueError`` naming the bytes.
    ``streamed=True`` (never chosen automatically): the same Dataset, to rounding, without the dense covariance -- the latent
    mean from ``predict_mean`` and one ``posterior_window_variances``, which produces only the band of the covariance the
    windows reach and whose work area ``max_bytes`` bounds instead -- for records of any length.  The covariance BETWEEN the
    outputs needs the dense path: ``return_cov=True`` is refused."""
    if streamed and return_cov:
        raise ValueError("the covariance between outputs needs the dense path: the streamed pass computes the variance of every "
                         "rolling mean alone; drop streamed=True or return_cov=True")
    mode, s, t = target_transform(model.dm)
    if statistic is None:
        statistic = "geometric_mean" if mode == MODE_LOG else "mean"
    if statistic not in ("mean", "geometric_mean"):
        raise ValueError(f"statistic must be 'mean' or 'geometric_mean', not {statistic!r}")
    if statistic == "geometric_mean" and mode != MODE_LOG:
        raise ValueError("the geometric mean is the model-space mean of a log target; this target is linear: use statistic='mean'")
    Xnew, times, lo, hi, out = record_windows(model, covariates, window, align, min_periods)
    Xnew = Xnew.to(model.device).contiguous()
    m, q = Xnew.shape[0], len(out)
    pass_mode = MODE_LOG if (mode == MODE_LOG and statistic == "mean") else MODE_LINEAR
    if streamed:
        wm, var = streamed_window_variances(model, Xnew, lo, hi, pass_mode, s, t, max_bytes)
        var = np.clip(var, 0.0, None)
        S = None
    else:
        check_window_budget(model, m, q, 0, max_bytes, "a rolling mean", streamable=True)
        model._eval_ready(Xnew)
        with torch.no_grad():
            kmean, cov = model._plan.posterior_cov(model._factor_theta, Xnew)
            mu = (kmean + model.model.prior_mean(Xnew)).contiguous()
            lo_t, hi_t = torch.from_numpy(lo), torch.from_numpy(hi)
            if pass_mode == MODE_LOG:
                mean_d, cov_d = model._plan.window_moments(cov, m, (s * mu + t).contiguous(), lo_t, hi_t, mode=MODE_LOG, scale2=s * s)
            else:
                mean_d, cov_d = model._plan.window_moments(cov, m, mu, lo_t, hi_t, mode=MODE_LINEAR)
        wm = mean_d.double().cpu().numpy()
        S = cov_d.double().cpu().numpy()[:q, :q]
        S = np.tril(S) + np.tril(S, -1).T
        var = np.clip(np.diagonal(S), 0.0, None)
    attrs = dict(_target_attrs(model.dm), statistic=statistic, window=str(window), align=align)
    z_lo, z_hi = norm.ppf((1 - ci) / 2), norm.ppf(1 - (1 - ci) / 2)
    if pass_mode == MODE_LOG:
        mean, se = wm, np.sqrt(var)
        lower, upper = intervals(MODE_LOG, mean, var, ci)
        interval = "approximate (lognormal with the exact mean and variance)"
    elif mode == MODE_LOG:
        sd = np.sqrt(var)
        mean = np.exp(s * wm + t)
        lower, upper = np.exp(s * (wm + z_lo * sd) + t), np.exp(s * (wm + z_hi * sd) + t)
        se = np.asarray(model.dm.error_pipeline.inverse_transform(var).values, dtype=np.float64).reshape(-1)
        interval = "exact"
    else:
        sd = np.sqrt(var)
        mean = s * wm + t
        lower, upper = mean + abs(s) * z_lo * sd, mean + abs(s) * z_hi * sd
        se = np.asarray(model.dm.error_pipeline.inverse_transform(var).values, dtype=np.float64).reshape(-1)
        interval = "exact"
    attrs["interval"] = interval
    ds = Dataset(
        {
            "mean": ("time", mean, attrs),
            "se": ("time", se, attrs),
            "lower": ("time", lower, dict(attrs, ci=ci)),
            "upper": ("time", upper, dict(attrs, ci=ci)),
            "n_points": ("time", (hi - lo).astype(np.int64)),
        },
        coords={"time": times[out]},
        attrs=attrs,
    )
    return (ds, S) if return_cov else ds


__all__ = ["time_windows", "rolling_mean", "record_windows", "window_bytes", "check_window_budget", "streamed_window_variances"]
