"""Exact excess and deficit over a threshold, per period, with uncertainty: BY HOW MUCH a criterion is overshot -- the mass
carried above an allowable load (the load reduction a TMDL asks for), the flood volume above bankfull discharge, or, with
the sign turned, the deficit volume below a low-flow threshold.

The reference can only sample, clip and sum: ``sim = model.sample(daily, n)``, ``np.clip(sim - tau, 0, None)``, a sum per
period and the spread over the draws.  For a log target c_i = exp(s f_i + t) over the latent posterior f ~ N(mu, C) the
moments of E_g = sum_{i in g} w_i (c_i - tau_i)^+ have a closed form: with m_i = s mu_i + t, v_i = s^2 C_ii (+ predictive
noise), sigma_i = sqrt(v_i), c_ij = s^2 C_ij, M_i = m_i + v_i / 2 and a_i = ln tau_i,

    E (c_i - tau_i)^+ = exp(M_i) Phi((m_i + v_i - a_i) / sigma_i) - tau_i Phi((m_i - a_i) / sigma_i),
    E e_i e_j = exp(M_i + M_j + c_ij) P11 - tau_j exp(M_i) P10 - tau_i exp(M_j) P01 + tau_i tau_j P00,
    P_tu = Phi2((m_i + t v_i + u c_ij - a_i) / sigma_i, (m_j + u v_j + t c_ij - a_j) / sigma_j; rho_ij),

(the opposite orthants for the deficit), computed on the device by ``dgp_excess_moments`` straight from the covariance
``dgp_posterior_cov`` writes: no factorisation, no draws, no sampling noise.  It reads the latent posterior covariance
alone, so Laplace and EP censored fits take the same path.  The pipelines' clip of the data-space value is not part of the
statistics.  Linear targets are refused.  A record whose dense footprint exceeds ``max_bytes`` -- sixteen months of a
15-minute stage record already do -- is refused too unless ``streamed=True`` is passed: ``dgp_posterior_excess_moments`` then
produces the covariance a panel of rows at a time from the held factorisation and never stores it whole, and ``max_bytes``
bounds its work area instead.  The streamed form is never chosen automatically: short panels cost time."""
from __future__ import annotations

import numpy as np
import torch
from scipy.stats import gamma

from .backend import MODE_LOG
from .exceedance import MAX_LEVELS
from .loads import DEFAULT_MAX_BYTES, _kept, _site_bytes, _target_attrs, flux_weights, period_groups, target_transform
from .xr_compat import Dataset

LINEAR_REFUSAL = ("the excess over a threshold is implemented for log targets only: for a linear target the pair function is "
                  "that of a clipped Gaussian, not of a clipped lognormal")


def log_threshold(tau):
    """Data-space thresholds -> a = ln tau (tau <= 0 -> -inf: the excess is the value itself, the deficit 0).  A non-finite
    threshold raises ``ValueError``."""
    tau = np.asarray(tau, dtype=np.float64)
    if not np.all(np.isfinite(tau)):
        raise ValueError("thresholds must be finite")
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(tau > 0, np.log(np.where(tau > 0, tau, 1.0)), -np.inf)


def excess_intervals(mean, var, ci=0.95):
    """Approximate central ``ci`` intervals of a non-negative sum from its exact mean and variance: the quantiles of a
    gamma distribution with the same two moments.  Where the variance is 0 (or the mean is not positive and finite) both
    ends are the mean itself."""
    lo_q, hi_q = (1 - ci) / 2, 1 - (1 - ci) / 2
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ok = np.isfinite(mean) & np.isfinite(var) & (mean > 0) & (var > 0)
        shape = np.where(ok, mean * mean / np.where(ok, var, 1.0), 1.0)
        scale = np.where(ok, var / np.where(ok, mean, 1.0), 1.0)
        lower, upper = gamma.ppf(lo_q, shape, scale=scale), gamma.ppf(hi_q, shape, scale=scale)
    return np.where(ok, lower, mean), np.where(ok, upper, mean)


def _work_bytes(m, P, L):
    """Bytes of ``dgp_excess_moments``' work area for one site: M (3 + 6 L + P min(L, 2)) + P doubles."""
    M = -(-m // 128) * 128
    return 8 * (M * (3 + 6 * L + P * min(L, 2)) + P)


def excess_sums(model, Xnew, a, w, groups, ngroups, above=True, pred_noise=False, max_bytes: int = DEFAULT_MAX_BYTES,
                streamed=False):
    """The device core: design rows ``Xnew`` (m, d), thresholds ``a`` = ln tau (L, m), weights ``w`` (m,), int32 group ids
    (non-decreasing, -1 = excluded) -> numpy (mean (L, P), cov (L, P, P), total (P,)) from ONE ``posterior_cov`` and one
    ``excess_moments`` per 64 levels.  ``NotImplementedError`` for a linear target, and for a record whose dense footprint --
    ``loads._site_bytes`` plus the pass's own work area -- exceeds ``max_bytes``.  ``streamed=True`` (never chosen
    automatically): the latent mean from ``predict_mean`` like ``exceedance.count_moments``' streamed branch, then one
    ``posterior_excess_moments`` per 64 levels, whose work area -- with the largest covariance panel that fits -- ``max_bytes``
    bounds instead (``ValueError`` naming the bytes when 128 panel rows do not fit)."""
    mode, s, t = target_transform(model.dm)
    if mode != MODE_LOG:
        raise NotImplementedError(LINEAR_REFUSAL)
    Xnew = Xnew.to(model.device).contiguous()
    m = Xnew.shape[0]
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, m))
    means, covs, total = [], [], None
    if streamed:
        model._eval_ready(Xnew)
        with torch.no_grad():
            latent = model._plan.predict_mean(model._factor_theta, Xnew) + model.model.prior_mean(Xnew)
            mapped = (s * latent + t).contiguous()
            extra = model.likelihood.predictive_noise(m, Xnew.device, model.dtype) if pred_noise else None
            for l0 in range(0, a.shape[0], MAX_LEVELS):
                mean_d, cov_d, total_d = model._plan.posterior_excess_moments(
                    model._factor_theta, Xnew, mapped, s * s, torch.from_numpy(a[l0:l0 + MAX_LEVELS]), w, groups, ngroups,
                    above=above, extra_var=extra, max_bytes=max_bytes)
                means.append(mean_d.cpu().numpy())
                covs.append(cov_d.cpu().numpy())
                total = total_d.cpu().numpy()
        return np.concatenate(means), np.concatenate(covs), total
    esz = torch.empty((), dtype=model.dtype).element_size()
    need = _site_bytes(model.dm.X.shape[0], m, esz) + _work_bytes(m, ngroups, min(a.shape[0], MAX_LEVELS))
    if need > max_bytes:
        raise NotImplementedError(f"the excess over a threshold needs the dense posterior covariance: a footprint of {need} bytes "
                                  f"for m = {m} points exceeds max_bytes = {max_bytes}; no streamed form is chosen "
                                  "automatically: pass streamed=True")
    model._eval_ready(Xnew)
    with torch.no_grad():
        kmean, cov = model._plan.posterior_cov(model._factor_theta, Xnew)
        mapped = (s * (kmean + model.model.prior_mean(Xnew)) + t).contiguous()
        extra = model.likelihood.predictive_noise(m, Xnew.device, model.dtype) if pred_noise else None
        for l0 in range(0, a.shape[0], MAX_LEVELS):
            mean_d, cov_d, total_d = model._plan.excess_moments(cov, m, mapped, s * s, torch.from_numpy(a[l0:l0 + MAX_LEVELS]), w,
                                                                groups, ngroups, above=above, extra_var=extra)
            means.append(mean_d.cpu().numpy())
            covs.append(cov_d.cpu().numpy())
            total = total_d.cpu().numpy()
    return np.concatenate(means), np.concatenate(covs), total


def excess(model, covariates, threshold=None, threshold_series=None, weights=None, freq="YE", above=True, ci=0.95,
           pred_noise=False, return_cov=False, max_bytes: int = DEFAULT_MAX_BYTES, level_labels=None, attrs=None, streamed=False):
    """``MarginalHIP.excess``: per period of ``freq`` the expected sum over the points of ``covariates`` of the target's
    excess over a threshold, sum_i w_i (c_i - tau_i)^+ -- ``above=False``: of its deficit sum_i w_i (tau_i - c_i)^+ -- with
    its exact standard error.

    ``threshold``: a number or a 1-D list of L data-space levels; ``threshold_series``: a per-point threshold, (m,) or
    (L, m); exactly one of the two; a threshold <= 0 is never undershot (a = -inf).  ``weights``: (m,), default 1 -- seconds
    per step turn a discharge into a volume, flux weights a concentration into a mass; a point with a non-finite weight or
    time is dropped like ``aggregate`` drops it.  ``pred_noise=True`` adds the likelihood's predictive noise to the
    variances (never to the covariances).
    -> Dataset on (``level``, ``time``) with ``mean``, ``se``, ``lower`` / ``upper``, ``total`` (per period: the expected
    sum w_i c_i), ``share`` = mean / total -- a RATIO OF EXPECTATIONS, not the expectation of a ratio -- and ``n_points``.
    Mean and se are exact; ``lower`` / ``upper`` are APPROXIMATE ``ci`` intervals: the quantiles of a gamma distribution
    matched to the exact mean and variance (the mean itself where the variance is 0).  With ``return_cov`` also the
    (L, P, P) covariance between the periods, level by level.  ``NotImplementedError``: a linear (non-log) target, and a
    record whose dense footprint exceeds ``max_bytes`` unless ``streamed=True`` (never chosen automatically): the covariance
    is then produced a panel of rows at a time (``excess_sums``) and ``max_bytes`` bounds that pass's work area."""
    if (threshold is None) == (threshold_series is None):
        raise ValueError("give exactly one of threshold and threshold_series")
    if target_transform(model.dm)[0] != MODE_LOG:
        raise NotImplementedError(LINEAR_REFUSAL)
    time = np.asarray(covariates.coords["time"].values).reshape(-1)
    m_all = len(time)
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
    a = log_threshold(series[:, order])
    Xnew = torch.tensor(model.dm.Xnew(covariates), dtype=model.dtype)[torch.as_tensor(order)]
    mean, cov, total = excess_sums(model, Xnew, a, w_all[order], groups, len(labels), above=above, pred_noise=pred_noise,
                                   max_bytes=max_bytes, streamed=streamed)
    var = np.clip(np.diagonal(cov, axis1=1, axis2=2), 0.0, None)
    lower, upper = excess_intervals(mean, var, ci)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = mean / total[None, :]
    attrs = dict(_target_attrs(model.dm) if attrs is None else attrs, above=bool(above))
    dims = ("level", "time")
    ds = Dataset(
        {
            "mean": (dims, mean, attrs),
            "se": (dims, np.sqrt(var), attrs),
            "lower": (dims, lower, dict(attrs, ci=ci)),
            "upper": (dims, upper, dict(attrs, ci=ci)),
            "total": ("time", total, attrs),
            "share": (dims, share, dict(attrs, units="1", long_name="Ratio of expectations: mean / total")),
            "n_points": ("time", n_points),
        },
        coords={"level": levels, "time": labels},
        attrs=dict(attrs, freq=freq),
    )
    return (ds, cov) if return_cov else ds


def _levels_or_series(value, m, name):
    """A number, a 1-D list of levels or a per-day series (m,) / (L, m) -> (series (L, m), level labels or None)."""
    v = np.asarray(value, dtype=np.float64)
    if not np.all(np.isfinite(v)):
        raise ValueError(f"{name} must be finite")
    if v.ndim == 2 and v.shape[1] == m and v.shape[0] > 0:
        return v, None
    if v.ndim == 1 and v.shape[0] == m and m > 0 and not isinstance(value, (list, tuple)):
        return v[None, :], None
    v = np.atleast_1d(v)
    if v.ndim != 1 or v.size == 0:
        raise ValueError(f"{name} must be a number, a 1-D list of levels or a per-day series of shape ({m},) or (L, {m})")
    return np.broadcast_to(v[:, None], (v.size, m)), v


def excess_load(model, covariates, criterion=None, limit=None, **kwargs):
    """``LoadestGP.excess_load``: the MASS per period carried above an allowable load (``above=False``: the mass by which
    the load stays below it), in kilograms.  Exactly one of
    ``criterion``: a concentration (mg/l); the allowable load of a day is criterion x flow, so tau_i = criterion;
    ``limit``: a load in kg per day; tau_i = limit_i / w_i with w_i the flux weights of ``annual_flux``, as in
    ``flux_exceedance``.
    Each a number, a list of levels, or a per-day series ((m,) array, or (L, m)).  The weights are the flux weights; a day
    with w_i <= 0 (or a missing flow) is excluded.  ``streamed`` and the other keywords go to ``excess``."""
    if (criterion is None) == (limit is None):
        raise ValueError("give exactly one of criterion and limit")
    attrs = _target_attrs(model.dm)
    wf = flux_weights(covariates, attrs)
    live = wf > 0
    series, labels = _levels_or_series(criterion if limit is None else limit, len(wf), "criterion" if limit is None else "limit")
    if limit is not None:
        series = series / np.where(live, wf, 1.0)[None, :]
    attrs = dict(attrs, units="kilograms", standard_name="flux")
    return excess(model, covariates, threshold_series=series, weights=np.where(live, wf, np.nan), level_labels=labels,
                  attrs=attrs, **kwargs)


__all__ = ["excess", "excess_load", "excess_sums", "excess_intervals", "log_threshold"]
