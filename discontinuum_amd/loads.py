"""Exact period sums (annual / monthly loads) of a fitted model's posterior, with their uncertainty.

The reference gets annual loads by Monte Carlo: ``sim = model.sample(daily, n)`` (the full m x m posterior covariance, its
jittered Cholesky factor, n draws), ``concentration_to_flux(sim, flow)`` and ``flux.resample(time="YE").sum()``
(``src/loadest_gp/utils.py:14-103``).  For the two target transforms of the project the moments of a period sum
L_g = sum_{i in g} w_i c_i have a closed form over the latent posterior f ~ N(mu, C) (model space), with s, t the target
scaler's ``scale_`` and ``mean_``:

    log      (c = exp(s f + t)):  a_i = w_i exp(s mu_i + t + s^2 C_ii / 2),   E[L_g] = sum_{i in g} a_i,
                                  Cov(L_g, L_h) = sum_{i in g, j in h} a_i a_j expm1(s^2 C_ij)
    standard (c = s f + t):       E[L_g] = sum_{i in g} w_i (s mu_i + t),  Cov(L_g, L_h) = s^2 sum w_i w_j C_ij

computed on the device by ``dgp_period_moments`` straight from the covariance ``dgp_posterior_cov`` writes: no
factorisation, no draws, no sampling noise.  The pipelines' clip of the data-space value (at 1e-6 for the log transform,
at 0 for the standard one) is not part of these moments; it only matters where the posterior puts mass below the clip.
"""
from __future__ import annotations

import re
import warnings

import numpy as np
import pandas as pd
import torch
from scipy.stats import norm

from . import pipeline as _pl
from .backend import MODE_LINEAR, MODE_LOG
from .gp.lowering import lower
from .xr_compat import Dataset

DEFAULT_MAX_BYTES = 16 * 2 ** 30  # device bytes per batch of sites in aggregate_many (posterior covariances + plan)


# ---------------------------------------------------------------------------------------------------- grouping
def _period_freq(freq: str) -> str:
    """Resample alias -> period alias: "YE" -> "Y", "YE-SEP" -> "Y-SEP", "QE" -> "Q", "ME" -> "M"."""
    return re.sub(r"^([YQM])E(?=$|-)", r"\1", freq)


def period_groups(time, weights, freq: str = "YE"):
    """Group the points by calendar period like ``resample(time=freq).sum()``.

    -> (order, groups, labels, n_points, n_dropped): ``order`` sorts the points by period (stable), ``groups`` are the
    int32 period ids of the sorted points (non-decreasing; -1 for a point whose weight or time is not finite -- the
    resampled sum skips NaN), ``labels`` the period-end dates (every period from the first to the last, empty ones
    included), ``n_points`` the points per period and ``n_dropped`` the points left out."""
    t = pd.DatetimeIndex(np.asarray(time).reshape(-1).astype("datetime64[ns]"))
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.shape[0] != len(t):
        raise ValueError(f"{w.shape[0]} weights for {len(t)} points")
    valid = np.isfinite(w) & ~t.isna()
    if not valid.any():
        raise ValueError("no point has a finite weight and time")
    pfreq = _period_freq(freq)
    ordinal = np.zeros(len(t), dtype=np.int64)
    ordinal[valid] = t[valid].to_period(pfreq).asi8
    first, last = ordinal[valid].min(), ordinal[valid].max()
    ids = np.where(valid, ordinal - first, -1)
    order = np.argsort(np.where(valid, ids, -1), kind="stable")
    groups = ids[order].astype(np.int32)
    P = int(last - first + 1)
    labels = pd.period_range(start=pd.Period(ordinal=int(first), freq=pfreq), periods=P, freq=pfreq)
    labels = labels.to_timestamp(how="end").normalize().to_numpy().astype("datetime64[ns]")
    n_points = np.bincount(groups[groups >= 0], minlength=P)
    return order, groups, labels, n_points, int((~valid).sum())


def _kept(order, groups, labels, n_points, dropped):
    """``period_groups`` without the excluded points: their covariates may be missing too (a NaN flow is both the
    weight and a model input), so they are not evaluated at all."""
    keep = groups >= 0
    return order[keep], groups[keep], labels, n_points, dropped


def target_transform(dm):
    """(mode, s, t) of a fitted target pipeline: ``log`` + ``scaler`` steps -> log mode, ``StandardPipeline`` -> linear
    mode; anything else raises ``NotImplementedError``."""
    pipe = dm.target_pipeline
    steps = dict(getattr(pipe, "steps", []))
    names = [name for name, _ in getattr(pipe, "steps", [])]
    scaler = steps.get("scaler")
    if not isinstance(scaler, _pl.StandardScaler):
        raise NotImplementedError(f"period moments need a standardised target, not {type(pipe).__name__}")
    s = float(np.asarray(scaler.scale_).reshape(-1)[0]) if scaler.with_std else 1.0
    t = float(np.asarray(scaler.mean_).reshape(-1)[0]) if scaler.with_mean else 0.0
    if names == ["metadata", "clip", "log", "scaler"]:
        return MODE_LOG, s, t
    if isinstance(pipe, _pl.StandardPipeline):
        return MODE_LINEAR, s, t
    raise NotImplementedError(f"period moments are exact for the log and standard transforms only, not {type(pipe).__name__}")


INTERVALS = ("lognormal", "three-moment")


def _check_interval(interval):
    if interval not in INTERVALS:
        raise ValueError(f"interval must be one of {INTERVALS}, not {interval!r}")
    return interval


def three_moment_fit(skew):
    """The shifted lognormal X = shift + scale exp(sigma Z) with a given skewness gamma > 0, in units of the standard
    deviation: omega = exp(sigma^2) solves (omega + 2) sqrt(omega - 1) = gamma, in closed form
    omega = A + 1 / A - 1, A = cbrt(1 + gamma^2 / 2 + sqrt(gamma^2 + gamma^4 / 4)) (the two cube roots of Cardano's formula
    multiply to 1).  Evaluated through u = omega - 1 = (A - 1)^2 / A with A - 1 from expm1 / log1p, which keeps full relative
    precision as gamma -> 0 (u ~ gamma^2 / 9).  -> (u, sigma, scale / sd); mean = shift + scale sqrt(omega)."""
    g = np.asarray(skew, dtype=np.float64)
    g2 = g * g
    d = np.expm1(np.log1p(0.5 * g2 + np.sqrt(g2 + 0.25 * g2 * g2)) / 3.0)
    u = d * d / (1.0 + d)
    with np.errstate(divide="ignore", invalid="ignore"):
        return u, np.sqrt(np.log1p(u)), 1.0 / np.sqrt(u * (1.0 + u))


SKEW_NORMAL_BELOW = 1e-8  # a skewness below this takes the normal interval, the fit's limit


def three_moment_intervals(mean, var, skew, ci=0.95):
    """Central ``ci`` intervals of the shifted lognormal with the given mean, variance and skewness (``three_moment_fit``):
    lower / upper = shift + scale exp(-/+ z sigma), written as mean + scale (expm1(-/+ z sigma) - expm1(sigma^2 / 2)) so that
    the normal limit is reached continuously.  A skewness below ``SKEW_NORMAL_BELOW`` gives the normal interval; a lower end
    below 0 (a negative shift) is clipped to 0.  -> (lower, upper, number of clipped lower ends)."""
    lo_q, hi_q = (1 - ci) / 2, 1 - (1 - ci) / 2
    mean, var = np.asarray(mean, dtype=np.float64), np.clip(np.asarray(var, dtype=np.float64), 0.0, None)
    skew = np.nan_to_num(np.asarray(skew, dtype=np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    se = np.sqrt(var)
    fitted = skew >= SKEW_NORMAL_BELOW
    u, sigma, rel = three_moment_fit(np.where(fitted, skew, 1.0))
    scale, centre = rel * se, np.expm1(0.5 * sigma * sigma)
    lower = np.where(fitted, mean + scale * (np.expm1(norm.ppf(lo_q) * sigma) - centre), mean + norm.ppf(lo_q) * se)
    upper = np.where(fitted, mean + scale * (np.expm1(norm.ppf(hi_q) * sigma) - centre), mean + norm.ppf(hi_q) * se)
    clipped = lower < 0.0
    return np.where(clipped, 0.0, lower), upper, int(np.count_nonzero(clipped))


def intervals(mode, mean, var, ci=0.95, interval="lognormal", skew=None):
    """Approximate central ``ci`` intervals from exact moments.  ``interval="lognormal"``: a lognormal with the same mean and
    variance (Fenton-Wilkinson) for log-mode sums of lognormals, the normal for linear-mode sums.  ``"three-moment"``: for
    log-mode sums the shifted lognormal with the same mean, variance and skewness ``skew``
    (``three_moment_intervals``); linear-mode sums are Gaussian and keep the normal interval."""
    _check_interval(interval)
    if interval == "three-moment" and mode != MODE_LINEAR:
        if skew is None:
            raise ValueError('interval="three-moment" needs the skewness')
        lower, upper, _clipped = three_moment_intervals(mean, var, skew, ci)
        return lower, upper
    lo_q, hi_q = (1 - ci) / 2, 1 - (1 - ci) / 2
    mean, var = np.asarray(mean, dtype=np.float64), np.clip(np.asarray(var, dtype=np.float64), 0.0, None)
    if mode == MODE_LINEAR:
        se = np.sqrt(var)
        return mean + norm.ppf(lo_q) * se, mean + norm.ppf(hi_q) * se
    with np.errstate(divide="ignore", invalid="ignore"):
        sig2 = np.log1p(var / mean ** 2)
        mu_ln = np.log(mean) - sig2 / 2
        lower = np.exp(mu_ln + norm.ppf(lo_q) * np.sqrt(sig2))
        upper = np.exp(mu_ln + norm.ppf(hi_q) * np.sqrt(sig2))
    pos = mean > 0
    return np.where(pos, lower, mean), np.where(pos, upper, mean)


def _dataset(mode, mean, cov, labels, n_points, attrs, ci, freq=None, cov_hyper=None, interval="lognormal", k3=None):
    """-> the result Dataset; its own attrs also carry the period ``freq`` (``period_change`` reads it).  ``cov_hyper``: the
    first-order contribution of the hyperparameters' uncertainty (``hyperparameters=True``), which adds ``se_hyper``,
    ``se_total`` and ``lower_total`` / ``upper_total`` (the two-moment interval rule at the summed variance, whatever
    ``interval`` is).  ``interval="three-moment"``: ``k3`` holds the periods' exact third central moments (None for a linear
    target: skewness 0); the Dataset gains ``skewness``, ``lower`` / ``upper`` come from ``three_moment_intervals`` and the
    attrs carry ``interval`` and ``clipped_lower``, the number of lower ends clipped to 0."""
    var = np.clip(np.diagonal(cov), 0.0, None)
    extra = {}
    if interval == "three-moment":
        with np.errstate(divide="ignore", invalid="ignore"):
            skew = np.zeros_like(var) if k3 is None else np.where(var > 0, np.asarray(k3, dtype=np.float64) / var ** 1.5, 0.0)
        if mode == MODE_LINEAR:
            (lower, upper), clipped = intervals(mode, mean, var, ci), 0
        else:
            lower, upper, clipped = three_moment_intervals(mean, var, skew, ci)
        extra = {"interval": interval, "clipped_lower": clipped}
    else:
        lower, upper = intervals(mode, mean, var, ci)
    attrs = dict(attrs)
    data = {
        "mean": ("time", mean, attrs),
        "se": ("time", np.sqrt(var), attrs),
        "lower": ("time", lower, dict(attrs, ci=ci)),
        "upper": ("time", upper, dict(attrs, ci=ci)),
        "n_points": ("time", n_points),
    }
    if interval == "three-moment":
        data["skewness"] = ("time", skew)
    if cov_hyper is not None:
        var_h = np.clip(np.diagonal(cov_hyper), 0.0, None)
        lower_t, upper_t = intervals(mode, mean, var + var_h, ci)
        note = dict(attrs, order="first (delta method)")
        data.update({"se_hyper": ("time", np.sqrt(var_h), note), "se_total": ("time", np.sqrt(var + var_h), note),
                     "lower_total": ("time", lower_t, dict(note, ci=ci)), "upper_total": ("time", upper_t, dict(note, ci=ci))})
    return Dataset(data, coords={"time": labels}, attrs=dict(attrs if freq is None else dict(attrs, freq=freq), **extra))


def _target_attrs(dm):
    meta = dict(getattr(dm.target_pipeline, "steps", [])).get("metadata")
    return dict(getattr(meta, "attrs_", {}) or {})


# ---------------------------------------------------------------------------------------------------- one site
def aggregate(model, covariates, weights, freq="YE", ci=0.95, pred_noise=False, return_cov=False, attrs=None,
              max_bytes: int = DEFAULT_MAX_BYTES, hyperparameters=False, prior=True, interval="lognormal"):
    """``MarginalHIP.aggregate``: exact mean / covariance of sum_{i in period} w_i c_i over the points of
    ``covariates`` (c = the model's target in data space).  A site whose dense footprint (``_site_bytes``) fits
    ``max_bytes`` takes one ``dgp_posterior_cov`` + one ``dgp_period_moments``; a larger one the streamed
    ``dgp_posterior_period_moments``, which never forms the m x m covariance.

    ``hyperparameters=True`` also propagates the hyperparameters' uncertainty to FIRST ORDER (delta method): with G the
    exact Jacobian of the period means with respect to the raw parameters (``hyperpar.period_hyper_covariance``, from one
    ``dgp_predict_sensitivity``) and Sigma_raw the exact inverse Fisher information (``prior``: with the priors' curvature),
    cov_hyper = G Sigma_raw G^T.  It adds ``se_hyper``, ``se_total`` = sqrt(se^2 + se_hyper^2) and ``lower_total`` /
    ``upper_total``; with ``return_cov`` the result is (ds, cov, cov_hyper).  It works on the dense and the streamed path
    alike (the Jacobian needs no m x m buffer).  Second-order terms are not included; ``flow_normalized``, ``exceedance`` and
    the ``*_many`` wrappers do not propagate.  ``False`` returns exactly the variables it always did.

    ``interval``: ``"lognormal"`` (the default) fits ``lower`` / ``upper`` to the two exact moments (Fenton-Wilkinson).
    ``"three-moment"`` also computes every period's exact third central moment (one ``dgp_period_third_moments`` on the dense
    covariance), adds ``skewness`` and takes ``lower`` / ``upper`` from the shifted lognormal with the exact mean, variance and
    skewness (``three_moment_intervals``): the three moments are exact, the interval is still a fitted shape.  The dense
    footprint then includes the product's work area (2 M^2 doubles); a record that fits ``max_bytes`` for two moments but not
    for three raises ``ValueError``, one that would take the streamed path ``NotImplementedError``.  With
    ``hyperparameters=True`` ``lower`` / ``upper`` are the three-moment ones and ``lower_total`` / ``upper_total`` stay the
    two-moment intervals at the summed variance (the hyperparameters' effect on the skewness is not propagated)."""
    _check_interval(interval)
    order, groups, labels, n_points, _dropped = _kept(*period_groups(covariates.coords["time"].values, np.asarray(weights), freq))
    w = np.asarray(weights, dtype=np.float64).reshape(-1)[order]
    Xnew = torch.tensor(model.dm.Xnew(covariates), dtype=model.dtype)[torch.as_tensor(order)]
    return point_moments(model, Xnew, w, groups, labels, n_points, ci=ci, pred_noise=pred_noise, return_cov=return_cov,
                         attrs=attrs, max_bytes=max_bytes, freq=freq, hyperparameters=hyperparameters, prior=prior,
                         interval=interval)


def point_moments(model, Xnew, w, groups, labels, n_points, ci=0.95, pred_noise=False, return_cov=False, attrs=None,
                  max_bytes: int = DEFAULT_MAX_BYTES, freq=None, hyperparameters=False, prior=True, interval="lognormal"):
    """The moment core of ``aggregate`` on model-space inputs: design rows ``Xnew`` (m, d), weights ``w`` (m,), int32
    period ids ``groups`` (non-decreasing, -1 = excluded), period ``labels`` and ``n_points`` per period -- what
    ``aggregate`` builds from a covariates record and ``flow_normalized`` from its (day, flow) pairs."""
    _check_interval(interval)
    if hyperparameters and hasattr(model, "_refuse_censored"):
        model._refuse_censored("the hyperparameters' uncertainty of period sums (hyperparameters=True)")
    mode, s, t = target_transform(model.dm)
    Xnew = Xnew.to(model.device).contiguous()
    m = Xnew.shape[0]
    model._eval_ready(Xnew)
    esz = torch.empty((), dtype=model.dtype).element_size()
    third = interval == "three-moment" and mode == MODE_LOG  # (a linear target is Gaussian: skewness 0, nothing to compute)
    k3_d = None
    if third:
        _third_moment_budget(_site_bytes(model.dm.X.shape[0], m, esz), m, len(labels), max_bytes)
    with torch.no_grad():
        if _site_bytes(model.dm.X.shape[0], m, esz) <= max_bytes:
            kmean, cov = model._plan.posterior_cov(model._factor_theta, Xnew)
            mu = kmean + model.model.prior_mean(Xnew)
            extra = model.likelihood.predictive_noise(m, Xnew.device, model.dtype) if pred_noise else None
            mean_d, cov_d = model._plan.period_moments(cov, m, (s * mu + t).contiguous(), s * s, w, groups, len(labels),
                                                       mode, extra_var=extra)
            if third:
                k3_d = model._plan.period_third_moments(cov, m, (s * mu + t).contiguous(), s * s, w, groups, len(labels),
                                                        extra_var=extra)
        else:
            mu = model._plan.predict_mean(model._factor_theta, Xnew) + model.model.prior_mean(Xnew)
            extra = model.likelihood.predictive_noise(m, Xnew.device, model.dtype) if pred_noise else None
            mean_d, cov_d = model._plan.posterior_period_moments(model._factor_theta, Xnew, (s * mu + t).contiguous(), s * s, w,
                                                                 groups, len(labels), mode, extra_var=extra)
        if hyperparameters:  # the per-point factors a_i of the period Jacobian need the pointwise variance on both paths
            _kmean, kvar = model._plan.predict(model._factor_theta, Xnew)
            var = kvar.double() + (extra.double() if extra is not None else 0.0)
            mapped = (s * mu + t).double()
            a_pt = torch.as_tensor(w, dtype=torch.float64, device=Xnew.device)
            if mode == MODE_LOG:
                a_pt = a_pt * torch.exp(mapped + 0.5 * s * s * var)
            a_pt = a_pt.cpu().numpy()
    mean, pcov = mean_d.cpu().numpy(), cov_d.cpu().numpy()
    cov_hyper = None
    if hyperparameters:
        from .hyperpar import period_hyper_covariance

        cov_hyper, _G = period_hyper_covariance(model, Xnew, a_pt, groups, len(labels), mode, s, prior=prior, pred_noise=pred_noise)
    ds = _dataset(mode, mean, pcov, labels, n_points, _target_attrs(model.dm) if attrs is None else attrs, ci, freq, cov_hyper,
                  interval=interval, k3=None if k3_d is None else k3_d.cpu().numpy())
    if return_cov:
        return (ds, pcov, cov_hyper) if hyperparameters else (ds, pcov)
    return ds


# ---------------------------------------------------------------------------------------------------- many sites
def _site_bytes(n, m, esz):
    """Device bytes of the dense path for one site: the (M, M) covariance, the prediction's cross terms, the plan."""
    N, M = -(-n // 128) * 128, -(-m // 128) * 128
    return esz * (M * M + 2 * N * M + 3 * N * N) + 8 * M * 8


def _third_moment_bytes(m, P):
    """Device bytes of ``dgp_period_third_moments``' work area for one site (``dgp_period_third_moments_workspace_bytes``, area
    by area, each rounded up to 256 bytes): a, the row totals, the points' periods, the periods' and the 64-row blocks' column
    ranges, the per-(tile, row) partials, and the two M x M double matrices."""
    M, up = -(-m // 128) * 128, lambda b: -(-b // 256) * 256
    nb = M // 64
    return 2 * up(8 * M) + up(4 * M) + up(8 * P) + up(8 * nb) + up(8 * 64 * (nb * (nb + 1) // 2)) + 2 * up(8 * M * M)


def _third_moment_budget(dense_bytes, m, P, max_bytes):
    """The footprint check of ``interval="three-moment"`` for one site whose two-moment dense path needs ``dense_bytes``."""
    if dense_bytes > max_bytes:
        raise NotImplementedError(f'interval="three-moment" needs the dense m x m covariance: this record ({dense_bytes} bytes '
                                  f"dense, max_bytes = {max_bytes}) takes the streamed dgp_posterior_period_moments, for "
                                  "which no third-moment pass exists")
    need = dense_bytes + _third_moment_bytes(m, P)
    if need > max_bytes:
        raise ValueError(f'interval="three-moment" needs {need} bytes on the device ({dense_bytes} for the dense two-moment '
                         f"path + {need - dense_bytes} for the third-moment work area), max_bytes = {max_bytes}")


def _streamed_bytes(n, m, P, d, esz):
    """Device bytes of the streamed path for one site: the plan, the prediction's work area (coordinates, cross Gram, V,
    vectors, partial sums) and the moment pass's M P + 2 M + P doubles -- nothing of order M^2."""
    N, M = -(-n // 128) * 128, -(-m // 128) * 128
    return esz * (3 * N * N + 2 * N * M + (d + 3 + 64) * M) + 8 * (M * P + 2 * M + P) + 8 * M * 8


def _batches(idx, nbytes, sizes, max_bytes):
    """Consecutive batches of the sites ``idx`` whose footprint ``len(batch) x nbytes(max n, max m)`` stays under
    ``max_bytes``; a site over budget on its own runs alone."""
    batches, cur, n_max, m_max = [], [], 0, 0
    for b in idx:
        n, m = sizes[b]
        n2, m2 = max(n_max, n), max(m_max, m)
        if cur and (len(cur) + 1) * nbytes(n2, m2) > max_bytes:
            batches.append(cur)
            cur, n2, m2 = [], n, m
        cur.append(b)
        n_max, m_max = n2, m2
    if cur:
        batches.append(cur)
    return batches


def aggregate_many(models, covariates_list, weights_list, freq="YE", ci=0.95, pred_noise=False, return_cov=False,
                   max_bytes: int = DEFAULT_MAX_BYTES, attrs_list=None, interval="lognormal"):
    """``aggregate`` for many fitted sites (different n and m allowed) like ``multisite_fit.predict_many``: per batch of
    sites ONE batched plan, one batched ``dgp_factorize``, one batched ``dgp_posterior_cov`` and one
    ``dgp_period_moments`` launch (gridDim.z = sites); pad points carry group -1.  Sites are cut into consecutive
    batches whose device footprint -- B x (M^2 + 2 N M + 3 N^2) elements for the covariances, the cross terms and the
    plan -- stays under ``max_bytes`` (default 16 GiB; one site at m = 11 323 already needs 1 GB for its covariance).
    Sites whose dense footprint alone exceeds ``max_bytes`` take the streamed ``dgp_posterior_period_moments`` instead,
    in batches of their own cut by the streamed footprint (``_streamed_bytes``: nothing of order M^2).  A batch in which a
    model carries censoring (``fit(censored=)`` / ``fit_many(censored=)``) builds its cache with the batched
    ``laplace_factorize`` (``multisite_fit.censored_cache_build``): the Laplace posterior, not the limits taken for samples.
    ``interval="three-moment"`` (see ``aggregate``): one batched ``dgp_period_third_moments`` per dense batch, whose footprint
    then counts the product's work area; a site that would go the streamed way raises ``NotImplementedError``."""
    from .backend import GPPlan
    from . import _lib

    _check_interval(interval)
    if not (len(models) == len(covariates_list) == len(weights_list)) or not models:
        raise ValueError("aggregate_many needs one covariates object and one weight vector per model")
    for mdl in models:
        if not mdl.is_fitted:
            raise RuntimeError("The model hasn't been fitted yet, call .fit().")
    dtype, device = models[0].dtype, torch.device(models[0].device)
    esz = torch.empty((), dtype=dtype).element_size()
    sites = []
    with torch.no_grad():
        for b, (mdl, cov, wts) in enumerate(zip(models, covariates_list, weights_list)):
            mdl.model.eval()
            mdl.likelihood.eval()
            mode, s, t = target_transform(mdl.dm)
            order, groups, labels, n_points, _ = _kept(*period_groups(cov.coords["time"].values, np.asarray(wts), freq))
            w = np.asarray(wts, dtype=np.float64).reshape(-1)[order]
            x = torch.tensor(mdl.dm.X, dtype=dtype)
            xn = torch.tensor(mdl.dm.Xnew(cov), dtype=dtype)[torch.as_tensor(order)]
            if hasattr(mdl.model, "prepare_eval"):
                mdl.model.prepare_eval(x, xn)
            name, theta_fn = lower(mdl.model.covar_module, x.shape[1])
            sites.append(dict(mode=mode, s=s, t=t, groups=groups, labels=labels, n_points=n_points, w=w, x=x, xn=xn,
                              y=torch.tensor(mdl.model_space_targets() if hasattr(mdl, "model_space_targets") else mdl.dm.y,
                                             dtype=dtype), name=(name, x.shape[1]),
                              theta=theta_fn().detach().to(torch.float64), prior=mdl.model.prior_mean(x).detach().to(dtype),
                              noise=mdl.likelihood.train_noise(torch.device("cpu"), dtype).detach().reshape(-1),
                              xmean=mdl.model.prior_mean(xn).detach().to(dtype),
                              extra=(mdl.likelihood.predictive_noise(xn.shape[0], torch.device("cpu"), dtype)
                                     if pred_noise else None)))
    if len({st["name"] for st in sites}) != 1 or len({st["mode"] for st in sites}) != 1:
        raise ValueError("aggregate_many needs sites of one model family, one input dimension and one target transform")
    # sites whose dense footprint fits the budget keep the dense batches; the others go the streamed way in batches of
    # their own, cut by the streamed footprint
    sizes = [(st["x"].shape[0], st["xn"].shape[0]) for st in sites]
    dense = [b for b, (n, m) in enumerate(sizes) if _site_bytes(n, m, esz) <= max_bytes]
    rest = [b for b in range(len(sites)) if b not in set(dense)]
    P_all, d_all = max(len(st["labels"]) for st in sites), sites[0]["name"][1]
    third = interval == "three-moment" and sites[0]["mode"] == MODE_LOG
    if third:
        for n, m in sizes:
            _third_moment_budget(_site_bytes(n, m, esz), m, P_all, max_bytes)
    dense_bytes = (lambda n, m: _site_bytes(n, m, esz) + _third_moment_bytes(m, P_all)) if third else (lambda n, m: _site_bytes(n, m, esz))
    batches = [(idx, False) for idx in _batches(dense, dense_bytes, sizes, max_bytes)]
    batches += [(idx, True) for idx in _batches(rest, lambda n, m: _streamed_bytes(n, m, P_all, d_all, esz), sizes, max_bytes)]

    results = [None] * len(sites)
    for idx, streamed in batches:
        group = [sites[b] for b in idx]
        B = len(group)
        (name, d), mode = group[0]["name"], group[0]["mode"]
        sizes, msizes = [st["x"].shape[0] for st in group], [st["xn"].shape[0] for st in group]
        n, mm = max(sizes), max(msizes)
        plan = GPPlan(name, n, d, dtype=dtype, device=device, lookahead=1 if B > 1 else 2, batch=B)
        if B > 1:
            plan.set_site_sizes(sizes)

        def slots(ts, width, fill=0.0, dt=dtype):
            out = torch.full((B, width) + tuple(ts[0].shape[1:]), fill, dtype=dt)
            for k, v in enumerate(ts):
                out[k, : v.shape[0]] = torch.as_tensor(v, dtype=dt)
            return out

        X = slots([st["x"] for st in group], n).to(device).contiguous()
        R = slots([st["y"] - st["prior"] for st in group], n).to(device).contiguous()
        Nz = slots([st["noise"] for st in group], n, 1.0).to(device).contiguous()
        Xs = torch.stack([torch.cat([st["xn"], st["xn"][-1:].expand(mm - st["xn"].shape[0], -1)]) for st in group])
        Xs = Xs.to(device).contiguous()
        theta = torch.stack([st["theta"] for st in group])
        single = B == 1
        one = (lambda v: v[0].contiguous()) if single else (lambda v: v)
        with torch.no_grad():
            plan.set_inputs(one(X))
            if any(getattr(models[b], "_censor", None) is not None for b in idx):  # the Laplace posterior, not the limits as samples
                from .multisite_fit import censored_cache_build

                out = censored_cache_build(plan, [models[b] for b in idx], theta, [st["y"] for st in group],
                                           [st["prior"] for st in group], [st["noise"] for st in group], sizes, n)
            else:
                out = plan.factorize(one(theta), one(R), one(Nz))
            info = out.reshape(B, -1)[:, _lib.OUT_INFO].cpu()
            if bool((info != 0).any()):
                bad = int(torch.nonzero(info)[0])
                raise RuntimeError(f"site {idx[bad]}: matrix not positive definite (Cholesky pivot {int(info[bad])})")
            if streamed:
                kmean, cov = plan.predict_mean(one(theta), one(Xs)), None
            else:
                kmean, cov = plan.posterior_cov(one(theta), one(Xs))
            mu = kmean.reshape(B, mm) + slots([st["xmean"] for st in group], mm).to(device)
            sv = torch.tensor([st["s"] for st in group], dtype=dtype, device=device)
            tv = torch.tensor([st["t"] for st in group], dtype=dtype, device=device)
            mapped = (sv[:, None] * mu + tv[:, None]).contiguous()
            W = slots([st["w"] for st in group], mm, dt=torch.float64)
            G = slots([st["groups"] for st in group], mm, -1, dt=torch.int32)
            EV = slots([st["extra"] for st in group], mm).to(device).contiguous() if pred_noise else None
            P = max(len(st["labels"]) for st in group)
            if streamed:
                mean_d, cov_d = plan.posterior_period_moments(one(theta), one(Xs), one(mapped), (sv.double() ** 2).cpu(), one(W),
                                                              one(G), P, mode, extra_var=one(EV) if EV is not None else None)
            else:
                mean_d, cov_d = plan.period_moments(cov, mm, one(mapped), (sv.double() ** 2).cpu(), one(W), one(G), P, mode,
                                                    extra_var=one(EV) if EV is not None else None)
            k3_h = None
            if third:
                k3_h = plan.period_third_moments(cov, mm, one(mapped), (sv.double() ** 2).cpu(), one(W), one(G), P,
                                                 extra_var=one(EV) if EV is not None else None).reshape(B, P).cpu().numpy()
        mean_h, cov_h = mean_d.reshape(B, P).cpu().numpy(), cov_d.reshape(B, P, P).cpu().numpy()
        del plan, cov
        for k, b in enumerate(idx):
            st = sites[b]
            p = len(st["labels"])
            attrs = _target_attrs(models[b].dm) if attrs_list is None else attrs_list[b]
            ds = _dataset(mode, mean_h[k, :p], cov_h[k, :p, :p], st["labels"], st["n_points"], attrs, ci, freq, interval=interval,
                          k3=None if k3_h is None else k3_h[k, :p])
            results[b] = (ds, cov_h[k, :p, :p].copy()) if return_cov else ds
    return results


# ---------------------------------------------------------------------------------------------------- loads
def flux_weights(covariates, concentration_attrs):
    """w_i = Q_i dt 1e-3 (flow in m^3/s, dt in s, mg/l -> kg) for a regular time grid, with ``concentration_to_flux``'s
    unit warnings; an irregular grid raises ``ValueError``."""
    time = np.asarray(covariates.coords["time"].values).astype("datetime64[ns]")
    dt = np.unique(np.diff(time).astype("timedelta64[ns]").astype(np.int64)) / 1e9
    if len(dt) != 1:
        raise ValueError("annual_flux needs a regular time grid (one constant time step)")
    flow = covariates["flow"]
    _unit_warnings(flow, concentration_attrs, stacklevel=4)
    return np.asarray(flow.values, dtype=np.float64).reshape(-1) * dt[0] * 1e-3


def _unit_warnings(flow, concentration_attrs, stacklevel):
    if getattr(flow, "attrs", {}).get("units") != "cubic meters per second":
        warnings.warn("Check that flow is 'cubic meters per second'. Set flow.units = 'cubic meters per second' to silence.",
                      UserWarning, stacklevel=stacklevel)
    if "mg/l" not in str(concentration_attrs.get("units", "")):
        warnings.warn("Check that concentration is in 'mg/l'. Set concentration.units = 'mg/l' to silence.",
                      UserWarning, stacklevel=stacklevel)


def _flux_attrs(model):
    attrs = _target_attrs(model.dm)
    attrs["units"] = "kilograms"
    attrs["standard_name"] = "flux"
    return attrs


def annual_flux(model, covariates, freq="YE", ci=0.95, pred_noise=False, return_cov=False, max_bytes: int = DEFAULT_MAX_BYTES,
                hyperparameters=False, prior=True, interval="lognormal"):
    """``LoadestGP.annual_flux``: exact period loads (kg) and their uncertainty.  ``hyperparameters=True``: also the
    first-order (delta method) contribution of the hyperparameters' uncertainty, see ``aggregate``.
    ``interval="three-moment"``: the exact skewness of every load and intervals fitted to three moments, see ``aggregate``."""
    _check_interval(interval)
    w = flux_weights(covariates, _target_attrs(model.dm))
    return aggregate(model, covariates, w, freq=freq, ci=ci, pred_noise=pred_noise, return_cov=return_cov,
                     attrs=_flux_attrs(model), max_bytes=max_bytes, hyperparameters=hyperparameters, prior=prior,
                     interval=interval)


# ---------------------------------------------------------------------------------------------------- flow normalization
DAY_NS = 86_400 * 10 ** 9


def day_keys(time):
    """Calendar key 0..364 of each day on a 365-day year: 29 Feb folds onto 28 Feb, the later days of a leap year shift
    back by one."""
    t = pd.DatetimeIndex(np.asarray(time).reshape(-1).astype("datetime64[ns]"))
    doy = t.dayofyear.to_numpy() - 1
    return np.where(t.is_leap_year & (doy >= 59), doy - 1, doy).astype(np.int64)


def flow_normalized_points(daily, kind="flux", freq="YE", flow_window=None):
    """The point set of flow-normalized (FN) period values: day t contributes (t, q) for every q in S(key(t)), the finite
    flows on all days with t's calendar key (inside ``flow_window`` = an inclusive (start, end) pair of date-likes, if
    given); days with an empty set are dropped.  Weights: ``kind="flux"`` q 86400 1e-3 / |S| (kg per mg/l), a day's
    average load; ``"concentration"`` 1 / (|S| D_p), D_p the contributing days of the period, a period mean.
    -> dict of point arrays ``time``, ``flow``, ``key``, ``set_size``, ``weight``, ``group`` (int32, non-decreasing) and
    per period ``labels`` and ``n_points`` (contributing days); ``daily`` must be on a daily grid (else ``ValueError``)."""
    if kind not in ("flux", "concentration"):
        raise ValueError(f"kind must be 'flux' or 'concentration', not {kind!r}")
    time = np.asarray(daily.coords["time"].values).reshape(-1).astype("datetime64[ns]")
    if len(time) < 2 or np.any(np.diff(time).astype(np.int64) != DAY_NS):
        raise ValueError("flow normalization needs a daily grid (one point per day, no gaps)")
    flow = np.asarray(daily["flow"].values, dtype=np.float64).reshape(-1)
    keys = day_keys(time)
    pool = np.isfinite(flow)
    if flow_window is not None:
        lo, hi = (np.datetime64(pd.Timestamp(v).to_datetime64(), "ns") for v in flow_window)
        pool &= (time >= lo) & (time <= hi)
    if not pool.any():
        raise ValueError("no finite flow to normalize with (check flow_window)")
    srt = np.argsort(keys[pool], kind="stable")
    pool_q = flow[pool][srt]
    count = np.bincount(keys[pool], minlength=365)
    start = np.cumsum(count) - count
    order, dgroups, labels, _n, _d = period_groups(time, np.ones(len(time)), freq)
    live = count[keys[order]] > 0
    days, groups = order[live], dgroups[live]
    size = count[keys[days]]
    n_points = np.bincount(groups, minlength=len(labels))
    day_of = np.repeat(np.arange(len(days)), size)                       # point -> contributing day
    within = np.arange(day_of.shape[0]) - np.repeat(np.cumsum(size) - size, size)
    q = pool_q[start[keys[days]][day_of] + within]
    g = groups[day_of].astype(np.int32)
    ns = size[day_of].astype(np.float64)
    w = q * 86400 * 1e-3 / ns if kind == "flux" else 1.0 / (ns * n_points[g])
    return {"time": time[days][day_of], "flow": q, "key": keys[days][day_of], "set_size": size[day_of], "weight": w,
            "group": g, "labels": labels, "n_points": n_points}


def flow_normalized(model, daily, kind="flux", freq="YE", flow_window=None, ci=0.95, pred_noise=False, return_cov=False,
                    max_bytes: int = DEFAULT_MAX_BYTES):
    """Flow-normalized (FN) period flux (kg, ``kind="flux"``) or mean concentration (``"concentration"``) -- WRTDS's FN
    values, with exact moments:  FN(p) = sum_{t in p} 1/|S(t)| sum_{q in S(t)} c(t, q) w(q), S(t) the flows seen on t's
    calendar day over the record (or over ``flow_window``: loads under a base period's flows, the counterfactual of the
    reference's ``time_substitution``, src/discontinuum/utils.py:36-67).  The points are those of
    ``flow_normalized_points`` -- about 365 Y^2 for Y years, which the streamed path takes once the dense one exceeds
    ``max_bytes``.  The model's design must be exactly (time, flow).  -> ``annual_flux``'s layout (+ the (P, P)
    covariance with ``return_cov``), the period change of which ``period_change`` gives."""
    if not model.is_fitted:
        raise RuntimeError("The model hasn't been fitted yet, call .fit().")
    names = tuple(model.dm.covariate_pipelines)
    if names != ("time", "flow"):
        raise ValueError(f"flow normalization needs a model of exactly (time, flow), not {names}")
    pts = flow_normalized_points(daily, kind=kind, freq=freq, flow_window=flow_window)
    if kind == "flux":
        _unit_warnings(daily["flow"], _target_attrs(model.dm), stacklevel=4)
        attrs = _flux_attrs(model)
    else:
        attrs = _target_attrs(model.dm)
    attrs["long_name"] = f"Flow-normalized {attrs.get('long_name', kind)}".strip()
    points = Dataset({"flow": ("time", pts["flow"])}, coords={"time": pts["time"]})
    Xnew = torch.tensor(model.dm.Xnew(points), dtype=model.dtype)
    return point_moments(model, Xnew, pts["weight"], pts["group"], pts["labels"], pts["n_points"], ci=ci,
                         pred_noise=pred_noise, return_cov=return_cov, attrs=attrs, max_bytes=max_bytes, freq=freq)


def period_change(ds, cov, start, end, ci=0.95, freq=None):
    """Change between two periods of an ``aggregate`` / ``annual_flux`` / ``flow_normalized`` result and its (P, P)
    covariance: ``start`` / ``end`` are date-likes, each selecting the period that contains it ("1995" = 1 Jan 1995) at the
    result's own frequency (its ``freq`` attribute, or ``freq``).  -> dict(start, end (period labels), change =
    mean[end] - mean[start], se = sqrt(C_ee + C_ss - 2 C_se), lower, upper (normal ``ci`` interval))."""
    freq = freq or dict(getattr(ds, "attrs", None) or {}).get("freq")
    if freq is None:
        raise ValueError("period_change needs the period frequency: pass freq= (aggregate / annual_flux / flow_normalized "
                         "results carry it)")
    pfreq = _period_freq(freq)
    labels = pd.DatetimeIndex(np.asarray(ds.coords["time"].values).reshape(-1).astype("datetime64[ns]"))
    periods = labels.to_period(pfreq)
    mean, cov = np.asarray(ds["mean"].values, dtype=np.float64), np.asarray(cov, dtype=np.float64)
    if cov.shape != (len(labels), len(labels)):
        raise ValueError(f"cov must be ({len(labels)}, {len(labels)})")

    def index(x):
        p = pd.Timestamp(x).to_period(pfreq)
        hit = np.nonzero(periods == p)[0]
        if not len(hit):
            raise ValueError(f"{pd.Timestamp(x).date()} lies in none of the periods {periods[0]} .. {periods[-1]}")
        return int(hit[0])

    s, e = index(start), index(end)
    change = mean[e] - mean[s]
    se = float(np.sqrt(max(cov[e, e] + cov[s, s] - 2.0 * cov[s, e], 0.0)))
    z = norm.ppf(1 - (1 - ci) / 2)
    return {"start": labels[s].to_datetime64(), "end": labels[e].to_datetime64(), "change": float(change), "se": se,
            "lower": float(change - z * se), "upper": float(change + z * se)}


def annual_flux_many(models, covariates_list, freq="YE", ci=0.95, pred_noise=False, return_cov=False,
                     max_bytes: int = DEFAULT_MAX_BYTES, interval="lognormal"):
    """``annual_flux`` for many sites through ``aggregate_many`` (batched device work, byte-budgeted batches);
    ``interval="three-moment"``: one batched ``dgp_period_third_moments`` per dense batch."""
    _check_interval(interval)
    weights = [flux_weights(cov, _target_attrs(m.dm)) for m, cov in zip(models, covariates_list)]
    return aggregate_many(models, covariates_list, weights, freq=freq, ci=ci, pred_noise=pred_noise, return_cov=return_cov,
                          max_bytes=max_bytes, attrs_list=[_flux_attrs(m) for m in models], interval=interval)


__all__ = ["aggregate", "aggregate_many", "annual_flux", "annual_flux_many", "period_groups", "target_transform",
           "intervals", "three_moment_fit", "three_moment_intervals", "point_moments", "day_keys", "flow_normalized_points", "flow_normalized", "period_change",
           "DEFAULT_MAX_BYTES"]
