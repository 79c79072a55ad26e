"""Exact leave-one-out / leave-group-out cross-validation of a fitted model, without refitting.

WRTDS / LOADEST practice publishes no load without held-out residuals and the flux bias statistic.  With gpytorch every
fold is a new factorisation (the reference has no such check: its only use of the posterior is ``predict``,
``src/discontinuum/engines/gpytorch.py:599-626``).  The engine's factorisation already holds what is needed: with
T = L^-1, alpha = K^^-1 r and a held-out index set B (Rasmussen & Williams 5.4.2; the block form is the partitioned inverse)

    G_B = (K^^-1)_BB = T[:, B]^T T[:, B],   e_B = y_B - E[y_B | y_-B] = G_B^-1 alpha_B,   Cov[y_B | y_-B] = G_B^-1,
    log p(y_B | y_-B) = -1/2 alpha_B^T e_B + 1/2 log|G_B| - b/2 log 2 pi

which ``dgp_cross_validate`` evaluates on the device for all folds at once (``backend.GPPlan.cross_validate``).

What is held fixed: the hyperparameters, the parameters of the prior mean and the fitted data transforms keep their fitted
values and the prior mean is evaluated at all observations -- the standard GP cross-validation, not a refit per fold.  The
held-out variance is that of the OBSERVATION and uses each observation's *training* noise (it is on the diagonal of K^).
"""
from __future__ import annotations

import numpy as np
import torch
from scipy.stats import norm

from .gp.mll import NotPSDError
from .loads import period_groups, target_transform
from .backend import MODE_LOG
from .xr_compat import Dataset


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def cv_folds(time, scheme="loo"):
    """Fold ids for the observations at ``time``.  -> (groups, labels): ``groups`` (n,) int64 fold id per observation (in
    the observations' own order; -1 = never held out), ``labels`` one entry per fold id.  ``scheme``:

    * ``"loo"``: every observation is its own fold; the labels are the observations' times;
    * a resample alias as ``loads.period_groups`` takes them ("YE", "YE-SEP" for water years, "QE", "ME"): one fold per
      period that holds at least one observation, labelled with the period-end date;
    * an int k: k contiguous blocks in time order whose sizes differ by at most one, labelled 0 .. k-1;
    * ``("random", k, seed)``: k folds dealt round-robin over a seeded permutation, labelled 0 .. k-1;
    * an explicit integer array (n,) of fold ids >= 0 (-1: never held out), labelled 0 .. max id."""
    t = np.asarray(time).reshape(-1)
    n = t.shape[0]
    if n < 1:
        raise ValueError("no observations")
    if isinstance(scheme, str):
        if scheme.lower() == "loo":
            return np.arange(n, dtype=np.int64), t.copy()
        order, sorted_ids, labels, n_points, dropped = period_groups(t, np.ones(n), scheme)
        if dropped:
            raise ValueError(f"{dropped} observations have no valid time")
        ids = np.empty(n, dtype=np.int64)
        ids[order] = sorted_ids
        used = n_points > 0
        remap = np.cumsum(used) - 1
        return remap[ids].astype(np.int64), labels[used]
    if _is_int(scheme):
        k = int(scheme)
        if not 1 <= k <= n:
            raise ValueError(f"k = {k} folds for {n} observations")
        groups = np.empty(n, dtype=np.int64)
        rank = np.argsort(t, kind="stable")
        for f, block in enumerate(np.array_split(rank, k)):
            groups[block] = f
        return groups, np.arange(k)
    if isinstance(scheme, tuple) and len(scheme) == 3 and scheme[0] == "random":
        k, seed = int(scheme[1]), scheme[2]
        if not 1 <= k <= n:
            raise ValueError(f"k = {k} folds for {n} observations")
        groups = np.empty(n, dtype=np.int64)
        groups[np.random.default_rng(seed).permutation(n)] = np.arange(n) % k
        return groups, np.arange(k)
    arr = np.asarray(scheme)
    if arr.dtype.kind not in "iu" or arr.shape != (n,):
        raise ValueError(f"unknown fold scheme {scheme!r}: expected 'loo', a resample alias, an int, ('random', k, seed) or "
                         f"an integer array of shape ({n},)")
    arr = arr.astype(np.int64)
    if arr.min() < -1 or arr.max() < 0:
        raise ValueError("fold ids must be >= 0 (-1: never held out) and at least one observation must be held out")
    return arr, np.arange(int(arr.max()) + 1)


def _scheme_name(folds):
    if isinstance(folds, str):
        return folds
    if _is_int(folds):
        return f"{int(folds)}-block"
    if isinstance(folds, tuple):
        return "-".join(str(v) for v in folds)
    return "explicit"


def model_space(model, groups):
    """(y, mu, var, lpd) in model space for the fold ids ``groups`` (n,): the observations, their held-out predictive mean
    and variance (NaN / NaN where the observation is never held out) and the per-fold joint log density, as numpy arrays."""
    if hasattr(model.model, "prepare_eval"):
        model._factor_key = None  # a model with data-dependent clamps is factorised afresh
    model._eval_ready()  # no test points: the clamps see the training rows only
    with torch.no_grad():
        resid, var, lpd, info = model._plan.cross_validate(torch.as_tensor(np.asarray(groups), dtype=torch.int64))
        y = model._train_y.detach().to("cpu", torch.float64).numpy()
    resid, var = resid.detach().cpu().numpy(), var.detach().cpu().numpy()
    lpd, info = lpd.detach().cpu().numpy(), info.detach().cpu().numpy()
    if (info != 0).any():
        g = int(np.nonzero(info)[0][0])
        raise NotPSDError(f"cross-validation: the held-out block of fold {g} is not positive definite (pivot {int(info[g])})")
    held = np.asarray(groups) >= 0
    mu = np.where(held, y - resid, np.nan)
    var = np.where(held, var, np.nan)
    return y, mu, var, lpd


CAVITY_HINT = ('; pass laplace="cavity" for the cross-validation by Laplace cavity folds, which is approximate (the pseudo-data of '
               "the rows that stay are held at the full-data mode)")


def _wants_cavity(model, laplace, what):
    """Validate the ``laplace`` keyword of ``what``; -> whether the call takes the cavity path.  A censored fit is refused
    unless the caller asks for the approximation by name; on a fit without censoring ``"cavity"`` is the plain path."""
    if laplace not in (None, "cavity"):
        raise ValueError(f'laplace must be None or "cavity", got {laplace!r}')
    if getattr(model, "_censor", None) is None:
        return False
    if getattr(model._censor, "approximation", "laplace") == "ep":
        raise NotImplementedError(
            f'{what} is not available for a fit with approximation="ep": the cavity folds hold the pseudo-data at a Laplace MODE, '
            "which would be computed at hyperparameters trained for the EP posterior (the cross-validation of an EP fit, from the "
            "cavities dgp_ep_* returns, does not exist yet)")
    if laplace is None:
        model._refuse_censored(what, hint=CAVITY_HINT)
    return True


def cavity_space(model, groups, shift=0.0):
    """The planes of ``GPPlan.laplace_cross_validate`` for the fold ids ``groups`` of a censored fit, in model space, as a
    dict of numpy arrays (``mu`` and ``var`` NaN where the observation is never held out), plus ``y``, ``side`` and ``upper``
    (NaN off the bracketed rows) as the fit ran on them."""
    if hasattr(model.model, "prepare_eval"):
        model._factor_key = None
    model._eval_ready()
    groups = np.asarray(groups)
    with torch.no_grad():
        spec = model._prior()
        cs = spec.censored
        res = model._plan.laplace_cross_validate(model._factor_theta, model._train_y, spec.mean.contiguous(), spec.noise.contiguous(),
                                                 cs.side, cs.f, torch.as_tensor(groups, dtype=torch.int64), upper=cs.upper,
                                                 shift=float(shift))
    out = {k: v.detach().cpu().numpy() for k, v in res.items()}
    info = out.pop("info")
    if (info != 0).any():
        g = int(np.nonzero(info)[0][0])
        raise NotPSDError(f"cross-validation: the held-out block of fold {g} is not positive definite (pivot {int(info[g])})")
    held = groups >= 0
    out["mu"] = np.where(held, out["mu"], np.nan)
    out["var"] = np.where(held, out["var"], np.nan)
    out["y"] = model._train_y.detach().to("cpu", torch.float64).numpy()
    out["side"] = cs.side.detach().cpu().numpy().astype(np.int64)
    n = out["y"].shape[0]
    out["upper"] = np.full(n, np.nan) if cs.upper is None else np.where(out["side"] == 2, cs.upper.detach().cpu().numpy(), np.nan)
    return out


def _cross_validate_cavity(model, folds, ci, return_folds):
    """``cross_validate`` of a fit with censored observations: see there."""
    target = model.dm.data.target
    time = np.asarray(target.coords["time"].values)
    groups, labels = cv_folds(time, folds)
    try:
        mode, s, _t = target_transform(model.dm)
    except NotImplementedError:
        mode, s = None, 0.0
    shift = s if mode == MODE_LOG else 0.0  # the tilt of the lognormal mean (flux_bias); 0: the tilt plane is not needed
    cav = cavity_space(model, groups, shift)
    y, mu, var, side = cav["y"], cav["mu"], cav["var"], cav["side"]
    held = groups >= 0
    plain = held & (side == 0)
    sd = np.sqrt(var)
    q = norm.ppf(1 - (1 - ci) / 2)
    z = np.where(side == 0, (y - mu) / sd, np.nan)
    observed = np.asarray(target.values, dtype=np.float64).reshape(-1)
    upper_host = getattr(model, "_upper_host", None)
    observed_upper = np.full(observed.shape, np.nan)
    if upper_host is not None:
        observed_upper = np.where(side == 2, np.asarray(upper_host, dtype=np.float64).reshape(-1), np.nan)
    predicted = model.dm.y_t(mu)
    attrs = dict(getattr(predicted, "attrs", {}) or {})
    lower = np.asarray(model.dm.y_t(mu - q * sd).values).reshape(-1)
    upper = np.asarray(model.dm.y_t(mu + q * sd).values).reshape(-1)
    se = np.asarray(model.dm.error_pipeline.inverse_transform(var).values).reshape(-1)
    inside = (observed >= lower) & (observed <= upper)
    counts = np.bincount(groups[held], minlength=len(labels))
    lpd = np.where(held, cav["lpd"], np.nan)
    ds = Dataset(
        {
            "observed": ("time", observed, attrs),
            "observed_upper": ("time", observed_upper, attrs),
            "censored": ("time", side),
            "predicted": ("time", np.asarray(predicted.values).reshape(-1), attrs),
            "se": ("time", se, attrs),
            "lower": ("time", lower, dict(attrs, ci=ci)),
            "upper": ("time", upper, dict(attrs, ci=ci)),
            "z": ("time", z),
            "mu": ("time", mu),
            "var": ("time", var),
            "fold": ("time", groups),
            "lpd": ("time", lpd),
            "pit_lower": ("time", np.where(held, cav["pit_lower"], np.nan)),
            "pit_upper": ("time", np.where(held, cav["pit_upper"], np.nan)),
            "dlp": ("time", np.where(held, cav["dlp"], np.nan)),
            "tilt": ("time", np.where(held, cav["tilt"], np.nan)),
        },
        coords={"time": time},
        attrs={
            "elpd": float(lpd[held].sum()),
            "elpd_kind": "pointwise",
            "rmse": float(np.sqrt(np.mean((y - mu)[plain] ** 2))) if plain.any() else float("nan"),
            "coverage": float(inside[plain].mean()) if plain.any() else float("nan"),
            "n_censored": int((side != 0).sum()),
            "approximation": "laplace-cavity",
            "tilt_shift": float(shift),
            "n_folds": int((counts > 0).sum()),
            "scheme": _scheme_name(folds),
            "ci": ci,
        },
    )
    if not return_folds:
        return ds
    fold_lpd = np.bincount(groups[held], weights=lpd[held], minlength=len(labels))
    per_fold = Dataset({"lpd": ("fold", fold_lpd), "n_points": ("fold", counts)}, coords={"fold": labels})
    return ds, per_fold


def cross_validate(model, folds="loo", ci=0.95, return_folds=False, laplace=None):
    """Held-out predictions of every training observation of a fitted model (``cv_folds`` schemes), from the engine's own
    factorisation.  -> Dataset on the observations' ``time`` coordinate with ``observed``; ``predicted`` -- what
    ``predict`` would have returned for the observation had its fold been absent (through ``dm.y_t``; fitted transform
    and hyperparameters kept); ``se`` (through ``dm.error_pipeline.inverse_transform``, like ``predict``); ``lower`` /
    ``upper`` -- the exact central ``ci`` quantiles ``dm.y_t(mu -+ q sqrt(var))`` of the held-out observation (the target
    transforms are monotone; this is not the moment-matched ``loads.intervals``, which is meant for sums); ``z`` -- the
    model-space standardised residual; ``mu`` / ``var`` -- the model-space held-out mean and variance behind all of
    them; ``fold``.  Attributes: ``elpd`` (sum of the folds' joint log predictive densities,
    model space), ``rmse`` (model space), ``coverage`` (share of the held-out observations inside their interval),
    ``n_folds``, ``scheme``.  ``return_folds``: also a Dataset of per-fold ``lpd`` / ``n_points`` on a ``fold`` coordinate
    of the folds' labels.  See the module docstring for what is held fixed.

    A fit with CENSORED observations is refused (``NotImplementedError``) unless ``laplace="cavity"`` asks for the Laplace
    cavity folds by name (``GPPlan.laplace_cross_validate``; on a fit without censoring the keyword changes nothing): the
    fold's Gaussian sites are taken out of the Laplace posterior in closed form, no fold is refitted, and -- the
    approximation -- the pseudo-data of the rows that stay are held at the full-data mode.  The Dataset then also has
    ``observed_upper`` (NaN where there is none), ``censored`` (the codes -1 / 0 / +1 / 2), the pointwise ``lpd`` (the Gaussian
    density of an observed row, the probability of a censored row's bracket), ``pit_lower`` / ``pit_upper`` (the
    observation's probability integral transform, an interval for censored rows), ``dlp`` / ``tilt`` (what ``flux_bias``
    needs for the expected concentration inside a bracket); ``z`` is NaN on censored rows; ``elpd`` is the sum of the
    pointwise ``lpd`` (``elpd_kind="pointwise"``: the joint density of a fold with several censored rows is an orthant
    probability and is not attempted); ``rmse`` and ``coverage`` run over the observed held-out rows only; ``n_censored``;
    ``approximation="laplace-cavity"``.  ``return_folds``: the per-fold SUM of the pointwise ``lpd``."""
    if not 0.0 < ci < 1.0:
        raise ValueError("ci must be in (0, 1)")
    if _wants_cavity(model, laplace, "cross_validate"):
        return _cross_validate_cavity(model, folds, ci, return_folds)
    target = model.dm.data.target
    time = np.asarray(target.coords["time"].values)
    groups, labels = cv_folds(time, folds)
    y, mu, var, lpd = model_space(model, groups)
    held = groups >= 0
    sd = np.sqrt(var)
    q = norm.ppf(1 - (1 - ci) / 2)
    z = (y - mu) / sd
    observed = np.asarray(target.values, dtype=np.float64).reshape(-1)
    predicted = model.dm.y_t(mu)
    attrs = dict(getattr(predicted, "attrs", {}) or {})
    lower = np.asarray(model.dm.y_t(mu - q * sd).values).reshape(-1)
    upper = np.asarray(model.dm.y_t(mu + q * sd).values).reshape(-1)
    se = np.asarray(model.dm.error_pipeline.inverse_transform(var).values).reshape(-1)
    inside = (observed >= lower) & (observed <= upper)
    counts = np.bincount(groups[held], minlength=len(labels))
    ds = Dataset(
        {
            "observed": ("time", observed, attrs),
            "predicted": ("time", np.asarray(predicted.values).reshape(-1), attrs),
            "se": ("time", se, attrs),
            "lower": ("time", lower, dict(attrs, ci=ci)),
            "upper": ("time", upper, dict(attrs, ci=ci)),
            "z": ("time", z),
            "mu": ("time", mu),
            "var": ("time", var),
            "fold": ("time", groups),
        },
        coords={"time": time},
        attrs={
            "elpd": float(lpd.sum()),
            "rmse": float(np.sqrt(np.mean((y - mu)[held] ** 2))),
            "coverage": float(inside[held].mean()),
            "n_folds": int((counts > 0).sum()),
            "scheme": _scheme_name(folds),
            "ci": ci,
        },
    )
    if not return_folds:
        return ds
    per_fold = Dataset({"lpd": ("fold", lpd[: len(labels)]), "n_points": ("fold", counts)}, coords={"fold": labels})
    return ds, per_fold


def flux_bias(model, cv=None, folds="loo", laplace=None):
    """WRTDS's flux bias statistic on the sampled days, B = (sum P - sum O) / sum P: O_i the observed concentration x flow,
    P_i the cross-validated MEAN concentration x flow -- for the log transform the lognormal mean exp(s mu + t + s^2 var / 2),
    not the median ``cross_validate`` reports as ``predicted``.  Flow comes from the model's own training covariates.
    ``cv``: a Dataset ``cross_validate`` returned (default: ``cross_validate(model, folds)``); observations that are never
    held out are left out.

    ``laplace="cavity"``: a fit with censored observations (refused otherwise; ``cv``, when given, must then come from
    ``cross_validate(..., laplace="cavity")``).  P_i is the same on every held-out row; O_i of a censored row is the
    EXPECTATION of the concentration given the row's bracket under its own held-out predictive N(mu, var): for the log
    transform exp(s mu + t + s^2 var / 2 + tilt), tilt = log of the bracket's probability under N(mu + s var, var) minus that
    under N(mu, var); for a linear target s (mu + var dlp) + t with dlp = d log P / d mu."""
    cavity = _wants_cavity(model, laplace, "flux_bias")
    if cv is None:
        cv = cross_validate(model, folds, laplace=laplace)
    mu, var = (np.asarray(cv[k].values, dtype=np.float64).reshape(-1) for k in ("mu", "var"))
    held = np.asarray(cv["fold"].values).reshape(-1) >= 0
    mode, s, t = target_transform(model.dm)
    mean = np.exp(s * mu + t + 0.5 * s * s * var) if mode == MODE_LOG else s * mu + t
    flow = np.asarray(model.dm.data.covariates["flow"].values, dtype=np.float64).reshape(-1)
    observed = np.asarray(model.dm.data.target.values, dtype=np.float64).reshape(-1)
    if cavity:
        if cv.attrs.get("approximation") != "laplace-cavity":
            raise ValueError('flux_bias(laplace="cavity") needs the Dataset of cross_validate(..., laplace="cavity")')
        cens = np.asarray(cv["censored"].values).reshape(-1) != 0
        dlp, tilt = (np.asarray(cv[k].values, dtype=np.float64).reshape(-1) for k in ("dlp", "tilt"))
        if mode == MODE_LOG:
            if cv.attrs.get("tilt_shift") != s:
                raise ValueError("the cross-validation Dataset was computed for another target transform")
            expected = np.exp(s * mu + t + 0.5 * s * s * var + tilt)
        else:
            expected = s * (mu + var * dlp) + t
        observed = np.where(cens, expected, observed)
    P, O = float((mean * flow)[held].sum()), float((observed * flow)[held].sum())
    return (P - O) / P
