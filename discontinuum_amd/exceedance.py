"""Exact threshold-exceedance statistics of a fitted model's posterior: days per period above a criterion, duration
curves, pointwise exceedance probabilities -- each with its uncertainty.

The reference can only count by Monte Carlo: ``sim = model.sample(daily, n)``, ``(sim > threshold)``, a sum per period and
the spread of the counts over the draws.  Over the latent posterior f ~ N(mu, C) (model space) the moments of the count
N_g = sum_{i in g} w_i 1[f_i > u_i] have a closed form,

    z_i = (mu_i - u_i) / sigma_i,  sigma_i^2 = C_ii (+ predictive noise),  rho_ij = C_ij / (sigma_i sigma_j),
    E[N_g] = sum_{i in g} w_i Phi(z_i),
    Cov(N_g, N_h) = sum_{i in g} sum_{j in h} w_i w_j (Phi2(z_i, z_j; rho_ij) - Phi(z_i) Phi(z_j)),

with Phi2 the bivariate normal distribution function, computed on the device by ``dgp_exceedance_moments`` straight from
the covariance ``dgp_posterior_cov`` writes: no factorisation, no draws, no sampling noise.  ``streamed=True`` takes
``dgp_posterior_exceedance_moments`` instead, which produces that covariance a panel of rows at a time from the held
factorisation and never stores it: the same numbers (to rounding) at any record length.  The target transforms of the
project are monotone (log + standardise, or standardise), so a data-space threshold tau maps EXACTLY to the model-space
u = (ln tau - t) / s or (tau - t) / s (s, t the target scaler's ``scale_`` and ``mean_``): unlike the loads, nothing
lognormal is approximated.  The pipelines' clip of the data-space value is not part of the statistics.
"""
from __future__ import annotations

import numpy as np
import torch
from scipy.stats import beta, norm

from .backend import MODE_LOG
from .loads import DEFAULT_MAX_BYTES, _kept, _site_bytes, _target_attrs, flux_weights, period_groups, target_transform
from .xr_compat import DataArray, Dataset

MAX_LEVELS = 64  # levels of one ``dgp_exceedance_moments`` call; longer lists go in several


def model_space_threshold(dm, tau):
    """Data-space thresholds -> model space through the fitted target pipeline: (ln tau - t) / s for log targets (tau <= 0
    -> -inf: always exceeded), (tau - t) / s for standard ones.  A non-finite threshold raises ``ValueError``."""
    mode, s, t = target_transform(dm)
    tau = np.asarray(tau, dtype=np.float64)
    if not np.all(np.isfinite(tau)):
        raise ValueError("thresholds must be finite")
    if mode == MODE_LOG:
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(tau > 0, (np.log(np.where(tau > 0, tau, 1.0)) - t) / s, -np.inf)
    return (tau - t) / s


def count_intervals(mean, var, total, ci=0.95):
    """Approximate central ``ci`` intervals of a count N in [0, total] from its exact mean and variance: the quantiles of
    a beta distribution for N / total with the same two moments, times ``total``.  Where the variance is 0 (or the mean
    sits at 0 or ``total``) both ends are the mean itself."""
    lo_q, hi_q = (1 - ci) / 2, 1 - (1 - ci) / 2
    mean, var = np.asarray(mean, dtype=np.float64), np.clip(np.asarray(var, dtype=np.float64), 0.0, None)
    total = np.broadcast_to(np.asarray(total, dtype=np.float64), mean.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        f, v = mean / total, var / total ** 2
        room = f * (1 - f)
        ok = (total > 0) & (v > 0) & (room > 0)
        k = np.where(ok, np.maximum(room / np.where(ok, v, 1.0) - 1.0, 1e-8), 1.0)  # (v = room: a 0 / total coin)
        fa, fb = np.where(ok, f * k, 1.0), np.where(ok, (1 - f) * k, 1.0)
        lower, upper = total * beta.ppf(lo_q, fa, fb), total * beta.ppf(hi_q, fa, fb)
    return np.where(ok, lower, mean), np.where(ok, upper, mean)


def _work_bytes(m, P, L):
    """Bytes of ``dgp_exceedance_moments``' work area for one site: 2 M (L + 1) + M P min(L, 8) + P doubles."""
    M = -(-m // 128) * 128
    return 8 * (2 * M * (L + 1) + M * P * min(L, 8) + P)


def count_moments(model, Xnew, u, w, groups, ngroups, pred_noise=False, max_bytes: int = DEFAULT_MAX_BYTES, streamed=False,
                  windows=None):
    """The device core: design rows ``Xnew`` (m, d), model-space thresholds ``u`` (L, m), weights ``w`` (m,), int32 group
    ids (non-decreasing, -1 = excluded) -> numpy (mean (L, P), cov (L, P, P)) from ONE ``posterior_cov`` and one
    ``exceedance_moments`` per 64 levels, taken the way ``loads.point_moments`` takes its dense branch.  A record whose
    dense footprint -- ``loads._site_bytes`` plus the moment pass's own work area (``_work_bytes``) -- exceeds
    ``max_bytes`` raises ``ValueError``.  ``streamed=True`` (never chosen automatically): the latent mean from
    ``predict_mean`` like ``point_moments``' streamed branch, then one ``posterior_exceedance_moments`` per 64 levels, whose
    work area -- with the largest covariance panel that fits -- ``max_bytes`` bounds instead.

    ``windows=(lo, hi)`` (int32, (q,) each: ``rolling.time_windows``): the counts are of the ROLLING MEANS over the windows
    ``lo[i] <= j < hi[i]`` of the points -- one ``window_moments`` between ``posterior_cov`` and ``exceedance_moments``;
    ``u``, ``w`` and ``groups`` are then per OUTPUT (q).  See ``_windowed_count_moments``."""
    if windows is not None:
        return _windowed_count_moments(model, Xnew, u, w, groups, ngroups, windows, pred_noise, max_bytes, streamed)
    Xnew = Xnew.to(model.device).contiguous()
    m = Xnew.shape[0]
    u = np.ascontiguousarray(np.asarray(u, dtype=np.float64).reshape(-1, m))
    means, covs = [], []
    if streamed:
        model._eval_ready(Xnew)
        with torch.no_grad():
            mu = (model._plan.predict_mean(model._factor_theta, Xnew) + model.model.prior_mean(Xnew)).contiguous()
            extra = model.likelihood.predictive_noise(m, Xnew.device, model.dtype) if pred_noise else None
            for l0 in range(0, u.shape[0], MAX_LEVELS):
                mean_d, cov_d = model._plan.posterior_exceedance_moments(
                    model._factor_theta, Xnew, mu, torch.from_numpy(u[l0:l0 + MAX_LEVELS]), w, groups, ngroups, extra_var=extra,
                    max_bytes=max_bytes)
                means.append(mean_d.cpu().numpy())
                covs.append(cov_d.cpu().numpy())
        return np.concatenate(means), np.concatenate(covs)
    esz = torch.empty((), dtype=model.dtype).element_size()
    need = _site_bytes(model.dm.X.shape[0], m, esz) + _work_bytes(m, ngroups, min(u.shape[0], MAX_LEVELS))
    if need > max_bytes:
        raise ValueError(f"exceedance statistics need the dense posterior covariance: a footprint of {need} bytes for "
                         f"m = {m} points exceeds max_bytes = {max_bytes}; pass streamed=True")
    model._eval_ready(Xnew)
    with torch.no_grad():
        kmean, cov = model._plan.posterior_cov(model._factor_theta, Xnew)
        mu = (kmean + model.model.prior_mean(Xnew)).contiguous()
        extra = model.likelihood.predictive_noise(m, Xnew.device, model.dtype) if pred_noise else None
        for l0 in range(0, u.shape[0], MAX_LEVELS):
            mean_d, cov_d = model._plan.exceedance_moments(cov, m, mu, torch.from_numpy(u[l0:l0 + MAX_LEVELS]), w, groups,
                                                           ngroups, extra_var=extra)
            means.append(mean_d.cpu().numpy())
            covs.append(cov_d.cpu().numpy())
    return np.concatenate(means), np.concatenate(covs)


WINDOW_REFUSALS = {
    "streamed": "a window needs the dense posterior covariance: the streamed pass produces it a panel of rows at a time, and a "
                "window reaches across panels (a streamed form needs a row halo); drop streamed=True",
    "pred_noise": "pred_noise=True has no meaning for a rolling mean: the noise of an averaged hypothetical observation is not "
                  "defined here",
    "flux": "kind='flux' with a window is not implemented: a rolling mean of daily loads is a weighted sum of lognormals, not "
            "a Gaussian in model space",
    "statistic": "exceedance of the arithmetic rolling mean of a log target is not implemented: that mean is a sum of "
                 "lognormals, not a Gaussian; use the model-space statistic (the geometric mean)",
}


def _check_window_request(model, statistic, pred_noise, streamed):
    """The refusals of a windowed count, each saying why; -> nothing."""
    if streamed:
        raise NotImplementedError(WINDOW_REFUSALS["streamed"])
    if pred_noise:
        raise ValueError(WINDOW_REFUSALS["pred_noise"])
    mode, _s, _t = target_transform(model.dm)
    model_space = "geometric_mean" if mode == MODE_LOG else "mean"
    if statistic is not None and statistic not in ("mean", "geometric_mean"):
        raise ValueError(f"statistic must be 'mean' or 'geometric_mean', not {statistic!r}")
    if statistic == "mean" and mode == MODE_LOG:
        raise NotImplementedError(WINDOW_REFUSALS["statistic"])
    if statistic is not None and statistic != model_space:
        raise ValueError(f"the model-space statistic of this target is {model_space!r}, not {statistic!r}")


def _windowed_count_moments(model, Xnew, u, w, groups, ngroups, windows, pred_noise, max_bytes, streamed):
    """``count_moments`` of rolling means: ``Xnew`` (m, d) the points in time order, ``windows=(lo, hi)`` the q outputs'
    index windows, ``u`` (L, q), ``w`` (q,) and ``groups`` (q,; -1 = excluded) per output.  One ``posterior_cov``, one
    ``window_moments`` (mode 0: W mu and W C W^T in the covariance's own layout), then ``exceedance_moments`` on that.  The
    dense footprint grows by the (Q, Q) result and the pass's work area (``rolling.window_bytes``)."""
    from .rolling import check_window_budget

    if streamed:
        raise NotImplementedError(WINDOW_REFUSALS["streamed"])
    if pred_noise:
        raise ValueError(WINDOW_REFUSALS["pred_noise"])
    lo, hi = (np.ascontiguousarray(np.asarray(v, dtype=np.int32)) for v in windows)
    Xnew = Xnew.to(model.device).contiguous()
    m, q = Xnew.shape[0], len(lo)
    u = np.ascontiguousarray(np.asarray(u, dtype=np.float64).reshape(-1, q))
    check_window_budget(model, m, q, _work_bytes(q, ngroups, min(u.shape[0], MAX_LEVELS)), max_bytes,
                        "exceedance statistics of a rolling mean")
    means, covs = [], []
    model._eval_ready(Xnew)
    with torch.no_grad():
        kmean, cov = model._plan.posterior_cov(model._factor_theta, Xnew)
        mu = (kmean + model.model.prior_mean(Xnew)).contiguous()
        wmean, S = model._plan.window_moments(cov, m, mu, torch.from_numpy(lo), torch.from_numpy(hi))
        for l0 in range(0, u.shape[0], MAX_LEVELS):
            mean_d, cov_d = model._plan.exceedance_moments(S, q, wmean, torch.from_numpy(u[l0:l0 + MAX_LEVELS]), w, groups, ngroups)
            means.append(mean_d.cpu().numpy())
            covs.append(cov_d.cpu().numpy())
    return np.concatenate(means), np.concatenate(covs)


def _output_groups(times, keep, freq):
    """Period ids of the outputs in TIME order: an output belongs to the period of its own time stamp, one that does not
    qualify gets -1.  -> (groups int32, labels, n_points): the periods run from the first to the last qualifying output."""
    order, groups, labels, n_points, _dropped = period_groups(times, np.where(keep, 1.0, np.nan), freq)
    g = np.empty(len(times), dtype=np.int32)
    g[order] = groups
    return g, labels, n_points


def _finish(mean, cov, total, above, fraction, ci):
    """Complement / fraction on the host, then se and intervals: -> (mean, se, lower, upper, cov), each per level."""
    total = np.asarray(total, dtype=np.float64)
    if not above:
        mean = total[None, :] - mean  # the covariance of W - N is that of N
    var = np.clip(np.diagonal(cov, axis1=1, axis2=2), 0.0, None)
    lower, upper = count_intervals(mean, var, total[None, :], ci)
    se = np.sqrt(var)
    if fraction:
        with np.errstate(divide="ignore", invalid="ignore"):
            mean, se, lower, upper = (a / total[None, :] for a in (mean, se, lower, upper))
            cov = cov / (total[:, None] * total[None, :])[None]
    return mean, se, lower, upper, cov


def exceedance(model, covariates, threshold=None, threshold_series=None, freq="YE", above=True, fraction=False, ci=0.95,
               pred_noise=False, return_cov=False, max_bytes: int = DEFAULT_MAX_BYTES, streamed=False, window=None,
               align="right", min_periods=None, statistic=None):
    """``MarginalHIP.exceedance``: per period of ``freq`` the expected number of points of ``covariates`` at which the
    target exceeds a threshold -- days per year above a criterion, for a daily record -- with its exact standard error.

    ``threshold``: a number or a 1-D list of L data-space levels; ``threshold_series``: a per-point threshold, (m,) or
    (L, m), for criteria that vary by day; exactly one of the two.  ``above=False``: the points NOT above (mean ->
    sum w - mean, same covariance); ``fraction=True``: divided by the period's sum of weights; ``pred_noise=True`` adds
    the likelihood's predictive noise to the variances (never to the covariances).  Points with a non-finite time are
    dropped like ``aggregate`` drops them.
    -> Dataset on (``level``, ``time``) with ``mean``, ``se``, ``lower`` / ``upper`` and ``n_points`` (per period);
    ``lower`` / ``upper`` are APPROXIMATE ``ci`` intervals -- the quantiles of a beta distribution for N / sum w matched
    to the exact mean and variance (the mean itself where the variance is 0) --, mean and se are exact.  With
    ``return_cov`` also the (L, P, P) covariance between the periods, level by level.  A record whose dense footprint
    exceeds ``max_bytes`` raises ``ValueError``; ``streamed=True`` never forms the m x m covariance (``count_moments``).

    ``window`` ("30D", "7D", a ``numpy.timedelta64``; with ``align`` and ``min_periods``: ``rolling.time_windows``): the
    days on which the ROLLING mean of the target over that window -- the model-space mean: the geometric mean for a log
    target -- exceeds the threshold, which is how criteria on an averaging period are written.  An output belongs to the
    period of its own time stamp, the threshold is the one of its own day, outputs whose window does not qualify are left
    out and ``n_points`` counts the rest.  Refused with a window: ``streamed=True``, ``pred_noise=True``, the arithmetic
    ``statistic="mean"`` of a log target.  ``window=None`` (default) is the daily product, unchanged."""
    return _exceedance(model, covariates, threshold, threshold_series, freq=freq, above=above, fraction=fraction, ci=ci,
                       pred_noise=pred_noise, return_cov=return_cov, max_bytes=max_bytes, streamed=streamed, window=window,
                       align=align, min_periods=min_periods, statistic=statistic)


def _exceedance(model, covariates, threshold=None, threshold_series=None, *, weights=None, level_labels=None, freq="YE",
                above=True, fraction=False, ci=0.95, pred_noise=False, return_cov=False, max_bytes: int = DEFAULT_MAX_BYTES,
                streamed=False, window=None, align="right", min_periods=None, statistic=None):
    """The body of ``exceedance`` with what ``flux_exceedance`` adds: per-point ``weights`` of the count (default 1; a
    point with a non-finite weight is dropped like ``aggregate`` drops it) and ``level_labels`` for the ``level``
    coordinate of a per-point series.  With ``window`` the points are the record in time order, the outputs sit on them
    and the groups come from ``_output_groups``."""
    if (threshold is None) == (threshold_series is None):
        raise ValueError("give exactly one of threshold and threshold_series")
    time = np.asarray(covariates.coords["time"].values).reshape(-1)
    m_all = len(time)
    windows = None
    if window is not None:
        from .rolling import time_windows

        if weights is not None:
            raise NotImplementedError(WINDOW_REFUSALS["flux"])
        _check_window_request(model, statistic, pred_noise, streamed)
        w_all = np.ones(m_all)
        Xall = np.asarray(model.dm.Xnew(covariates))
        order, lo, hi, keep = time_windows(time, window, align, min_periods, valid=np.all(np.isfinite(Xall), axis=1))
        if not keep.any():
            raise ValueError(f"no window of the record holds min_periods = {min_periods} points")
        groups, labels, n_points = _output_groups(time[order], keep, freq)
        windows = (lo, hi)
    else:
        w_all = np.ones(m_all) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        order, groups, labels, n_points, _dropped = _kept(*period_groups(time, w_all, freq))
    if threshold is not None:
        levels = np.atleast_1d(np.asarray(threshold, dtype=np.float64))
        if levels.ndim != 1 or levels.size == 0:
            raise ValueError("threshold must be a number or a 1-D list of levels")
        series = np.broadcast_to(levels[:, None], (levels.size, m_all))
    else:
        series = np.asarray(threshold_series, dtype=np.float64)
        series = series[None, :] if series.ndim == 1 else series
        if series.ndim != 2 or series.shape[1] != m_all or series.shape[0] == 0:
            raise ValueError(f"threshold_series must have shape ({m_all},) or (L, {m_all})")
        levels = np.arange(series.shape[0])
    if level_labels is not None:
        levels = np.asarray(level_labels)
    u = model_space_threshold(model.dm, series[:, order])
    w = w_all[order]
    Xnew = torch.tensor(model.dm.Xnew(covariates), dtype=model.dtype)[torch.as_tensor(order)]
    if windows is None:
        mean, cov = count_moments(model, Xnew, u, w, groups, len(labels), pred_noise=pred_noise, max_bytes=max_bytes, streamed=streamed)
        total = np.bincount(groups, weights=w, minlength=len(labels))
    else:
        mean, cov = count_moments(model, Xnew, u, w, groups, len(labels), pred_noise=pred_noise, max_bytes=max_bytes, streamed=streamed,
                                  windows=windows)
        total = np.bincount(groups[groups >= 0], weights=w[groups >= 0], minlength=len(labels))
    mean, se, lower, upper, cov = _finish(mean, cov, total, above, fraction, ci)
    attrs = dict(_target_attrs(model.dm), above=bool(above), fraction=bool(fraction))
    if windows is not None:
        attrs.update(window=str(window), align=align, statistic="geometric_mean" if target_transform(model.dm)[0] == MODE_LOG else "mean")
    dims = ("level", "time")
    ds = Dataset(
        {
            "mean": (dims, mean, attrs),
            "se": (dims, se, attrs),
            "lower": (dims, lower, dict(attrs, ci=ci)),
            "upper": (dims, upper, dict(attrs, ci=ci)),
            "n_points": ("time", n_points),
        },
        coords={"level": levels, "time": labels},
        attrs=dict(attrs, freq=freq),
    )
    return (ds, cov) if return_cov else ds


def flux_exceedance(model, covariates, limit, **kwargs):
    """``LoadestGP.exceedance(kind="flux")``: days on which the daily LOAD exceeds ``limit`` (kg per day; a number or a
    list): the per-day concentration threshold tau_i = limit / w_i with w_i the flux weights of ``annual_flux``; a day
    with w_i <= 0 (or a missing flow) is excluded.  ``streamed`` and the other keywords go to ``_exceedance``."""
    wf = flux_weights(covariates, _target_attrs(model.dm))
    limits = np.atleast_1d(np.asarray(limit, dtype=np.float64))
    if limits.ndim != 1 or not np.all(np.isfinite(limits)):
        raise ValueError("the load limit must be a finite number or a 1-D list of them")
    live = wf > 0
    series = limits[:, None] / np.where(live, wf, 1.0)[None, :]
    return _exceedance(model, covariates, threshold_series=series, weights=np.where(live, 1.0, np.nan), level_labels=limits,
                       **kwargs)


def _latent_predict(model, covariates, pred_noise):
    """Model-space (mu, var) at the points of ``covariates`` from the plan's prediction, as numpy."""
    Xnew = torch.tensor(model.dm.Xnew(covariates), dtype=model.dtype)
    mu, var = model._model_space_predict(Xnew)  # (its variance carries the predictive noise)
    if not pred_noise:
        with torch.no_grad():
            var = var - model.likelihood.predictive_noise(Xnew.shape[0], var.device, model.dtype)
    return mu.double().cpu().numpy(), var.double().cpu().numpy()


def _data_space(model, f):
    """Model-space values -> data space through the target transform alone (exp(s f + t) or s f + t; no clip)."""
    mode, s, t = target_transform(model.dm)
    return np.exp(s * f + t) if mode == MODE_LOG else s * f + t


def _windowed_duration_curve(model, covariates, levels, above, ci, pred_noise, max_bytes, streamed, window, align, min_periods,
                             statistic):
    """``duration_curve`` of the rolling mean: the qualifying outputs as ONE group.  Default ``levels``: the 21 quantiles of
    the data-space rolling posterior mean (W mu, mapped) over those outputs."""
    from .rolling import time_windows

    _check_window_request(model, statistic, pred_noise, streamed)
    time = np.asarray(covariates.coords["time"].values).reshape(-1)
    Xall = np.asarray(model.dm.Xnew(covariates))
    order, lo, hi, keep = time_windows(time, window, align, min_periods, valid=np.all(np.isfinite(Xall), axis=1))
    if not keep.any():
        raise ValueError(f"no window of the record holds min_periods = {min_periods} points")
    if levels is None:
        mu, _var = _latent_predict(model, covariates, False)
        cs = np.concatenate([[0.0], np.cumsum(mu[order])])
        wm = (cs[hi[keep]] - cs[lo[keep]]) / (hi[keep] - lo[keep])
        levels = np.quantile(_data_space(model, wm), np.linspace(0.02, 0.98, 21))
    levels = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if levels.ndim != 1 or levels.size == 0:
        raise ValueError("levels must be a 1-D list of data-space levels")
    q, n = len(lo), int(keep.sum())
    u = np.broadcast_to(model_space_threshold(model.dm, levels)[:, None], (levels.size, q))
    Xnew = torch.tensor(Xall[order], dtype=model.dtype)
    mean, cov = count_moments(model, Xnew, u, np.ones(q), np.where(keep, 0, -1).astype(np.int32), 1, max_bytes=max_bytes,
                              windows=(lo, hi))
    mean, se, lower, upper, _cov = _finish(mean, cov, np.array([float(n)]), above, True, ci)
    attrs = dict(_target_attrs(model.dm), above=bool(above), n_points=n, window=str(window), align=align,
                 statistic="geometric_mean" if target_transform(model.dm)[0] == MODE_LOG else "mean")
    return Dataset(
        {
            "mean": ("level", mean[:, 0], attrs),
            "se": ("level", se[:, 0], attrs),
            "lower": ("level", lower[:, 0], dict(attrs, ci=ci)),
            "upper": ("level", upper[:, 0], dict(attrs, ci=ci)),
        },
        coords={"level": levels},
        attrs=attrs,
    )


def duration_curve(model, covariates, levels=None, above=True, ci=0.95, pred_noise=False, max_bytes: int = DEFAULT_MAX_BYTES,
                   streamed=False, window=None, align="right", min_periods=None, statistic=None):
    """``MarginalHIP.duration_curve``: the fraction of the record -- all points of ``covariates`` as ONE group -- on which
    the target exceeds each of ``levels`` (data space), with the exact standard error of that fraction and approximate
    ``ci`` intervals (``count_intervals``); for a rating model over a stage record, the flow-duration curve.  Default
    ``levels``: the 21 quantiles 2 %, 6.8 %, ... 98 % of the data-space posterior mean over the record.
    ``streamed=True``: without the m x m covariance, for records of any length (``count_moments``).
    -> Dataset on ``level`` with ``mean``, ``se``, ``lower``, ``upper``; ``n_points`` among its attributes.
    ``window`` (with ``align``, ``min_periods``): the duration curve of the ROLLING mean over that window instead -- the
    fraction of the qualifying outputs on which it exceeds each level (``exceedance`` explains the keyword and its
    refusals)."""
    if window is not None:
        return _windowed_duration_curve(model, covariates, levels, above, ci, pred_noise, max_bytes, streamed, window, align,
                                        min_periods, statistic)
    Xall = np.asarray(model.dm.Xnew(covariates))
    keep = np.nonzero(np.all(np.isfinite(Xall), axis=1))[0]
    if levels is None:
        mu, _var = _latent_predict(model, covariates, pred_noise)
        data_mean = np.asarray(model.dm.y_t(mu[keep]).values, dtype=np.float64).reshape(-1)
        levels = np.quantile(data_mean, np.linspace(0.02, 0.98, 21))
    levels = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if levels.ndim != 1 or levels.size == 0:
        raise ValueError("levels must be a 1-D list of data-space levels")
    m = len(keep)
    u = np.broadcast_to(model_space_threshold(model.dm, levels)[:, None], (levels.size, m))
    Xnew = torch.tensor(Xall[keep], dtype=model.dtype)
    mean, cov = count_moments(model, Xnew, u, np.ones(m), np.zeros(m, dtype=np.int32), 1, pred_noise=pred_noise,
                              max_bytes=max_bytes, streamed=streamed)
    mean, se, lower, upper, _cov = _finish(mean, cov, np.array([float(m)]), above, True, ci)
    attrs = dict(_target_attrs(model.dm), above=bool(above), n_points=m)
    return Dataset(
        {
            "mean": ("level", mean[:, 0], attrs),
            "se": ("level", se[:, 0], attrs),
            "lower": ("level", lower[:, 0], dict(attrs, ci=ci)),
            "upper": ("level", upper[:, 0], dict(attrs, ci=ci)),
        },
        coords={"level": levels},
        attrs=attrs,
    )


def _windowed_exceedance_probability(model, covariates, threshold, above, pred_noise, window, align, min_periods, max_bytes,
                                     streamed=False):
    """``exceedance_probability`` of the rolling mean: Phi(((W mu)_i - u_i) / sqrt(S_ii)) from the diagonal of S = W C W^T,
    on the qualifying outputs' ``time`` coordinate; a per-point threshold is read at the output's own time stamp.
    ``streamed``: (W mu, diag S) from ``rolling.streamed_window_variances`` instead of the dense pair."""
    from .rolling import check_window_budget, streamed_window_variances, time_windows

    if pred_noise:
        raise ValueError(WINDOW_REFUSALS["pred_noise"])
    time = np.asarray(covariates.coords["time"].values).reshape(-1)
    m_all = len(time)
    Xall = np.asarray(model.dm.Xnew(covariates))
    order, lo, hi, keep = time_windows(time, window, align, min_periods, valid=np.all(np.isfinite(Xall), axis=1))
    out = np.nonzero(keep)[0]
    if out.size == 0:
        raise ValueError(f"no window of the record holds min_periods = {min_periods} points")
    tau = np.broadcast_to(np.asarray(threshold, dtype=np.float64), (m_all,))[order][out]
    u = model_space_threshold(model.dm, tau)
    Xnew = torch.tensor(Xall[order], dtype=model.dtype).to(model.device).contiguous()
    m, q = Xnew.shape[0], len(out)
    if streamed:
        wm, var = streamed_window_variances(model, Xnew, lo[out], hi[out], max_bytes=max_bytes)
    else:
        check_window_budget(model, m, q, 0, max_bytes, "the exceedance probability of a rolling mean", streamable=True)
        model._eval_ready(Xnew)
        with torch.no_grad():
            kmean, cov = model._plan.posterior_cov(model._factor_theta, Xnew)
            mu = (kmean + model.model.prior_mean(Xnew)).contiguous()
            wmean, S = model._plan.window_moments(cov, m, mu, torch.from_numpy(np.ascontiguousarray(lo[out])),
                                                  torch.from_numpy(np.ascontiguousarray(hi[out])))
            wm = wmean.double().cpu().numpy()
            var = torch.diagonal(S)[:q].double().cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(var > 0, (wm - u) / np.sqrt(np.where(var > 0, var, 1.0)), np.where(wm > u, np.inf, -np.inf))
    z = np.where(np.isinf(u), np.where(u < 0, np.inf, -np.inf), z)
    p = norm.cdf(z if above else -z)
    attrs = dict(_target_attrs(model.dm), long_name="Exceedance probability" if above else "Non-exceedance probability",
                 units="1", window=str(window), align=align)
    return DataArray(p, coords={"time": time[order][out].astype("datetime64[ns]")}, dims=["time"], attrs=attrs)


def exceedance_probability(model, covariates, threshold, above=True, pred_noise=False, window=None, align="right",
                           min_periods=None, max_bytes: int = DEFAULT_MAX_BYTES, streamed=False):
    """``MarginalHIP.exceedance_probability``: the pointwise probability Phi((mu_i - u_i) / sigma_i) that the target
    exceeds ``threshold`` (a data-space number, or one value per point) at each point of ``covariates`` -- host-side, from
    the plan's existing prediction.  A point with zero variance gives 1 or 0 (a tie counts as not exceeded).
    -> DataArray on the covariates' coordinate.  ``window`` (with ``align``, ``min_periods``): the probability that the ROLLING
    mean over that window exceeds it, from the diagonal of the windowed covariance, on the qualifying outputs' ``time``.
    ``streamed=True`` (with ``window`` only; never chosen automatically): that diagonal from the streamed band pass of
    ``rolling_mean(streamed=True)``, without the dense covariance; ``max_bytes`` then bounds its work area."""
    if streamed and window is None:
        raise ValueError("streamed=True applies to the rolling mean: give window=; the pointwise probability needs no covariance")
    if window is not None:
        return _windowed_exceedance_probability(model, covariates, threshold, above, pred_noise, window, align, min_periods, max_bytes,
                                                streamed)
    mu, var = _latent_predict(model, covariates, pred_noise)
    tau = np.broadcast_to(np.asarray(threshold, dtype=np.float64), mu.shape)
    u = model_space_threshold(model.dm, tau)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(var > 0, (mu - u) / np.sqrt(np.where(var > 0, var, 1.0)), np.where(mu > u, np.inf, -np.inf))
    z = np.where(np.isinf(u), np.where(u < 0, np.inf, -np.inf), z)
    p = norm.cdf(z if above else -z)
    attrs = dict(_target_attrs(model.dm), long_name="Exceedance probability" if above else "Non-exceedance probability",
                 units="1")
    return DataArray(p, coords=dict(covariates.coords), dims=list(covariates.coords), attrs=attrs)


__all__ = ["exceedance", "flux_exceedance", "duration_curve", "exceedance_probability", "count_moments", "count_intervals",
           "model_space_threshold", "MAX_LEVELS"]
