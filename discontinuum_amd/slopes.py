"""Exact posterior slopes: the derivatives of a fitted surface with respect to its covariates.

The derivative of a GP is a GP, so the slope of the fit has a closed-form posterior.  With D_0 = id, D_q = d / d x*_q acting on
the test point, T = L^-1 and alpha = K^^-1 r from the factorisation the engine holds, and V_a = T (D_a K)(X, x*)

    E[D_a f(x*) | y]           = (D_a K)(x*, X) alpha
    Cov[D_a f, D_b f | y](x*)  = D_a D'_b k(x, x')|_{x = x' = x*} - V_a[:, *]^T V_b[:, *]

which ``dgp_predict_slopes`` evaluates for the value and all requested columns in one pass (``backend.GPPlan.predict_slopes``).
Differencing two ``predict`` calls gives the same mean but no standard error: the two predictions are strongly correlated and
``predict`` returns no covariance between them.

Units.  Every shipped covariate pipeline is an optional ``log`` or decimal-year step followed by an affine map x = a u + b
(standardisation, unit scaling), and the target is s f + t in its transformed space (``loads.target_transform``).  A slope is
reported per unit of u -- ln Q for log covariates (d ln C / d ln Q: the concentration-discharge slope), years for time
(x 100 ~ percent per year for log targets), the raw unit otherwise (d ln Q / d stage) -- in units of the transformed target:
s a (D f + D m) with m the prior mean function (constant for loadest-gp, the power law for rating-gp).  Data-space slopes of
log targets are deliberately absent: they are not Gaussian.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch
from scipy.stats import norm

from . import _lib
from . import pipeline as _pl
from .backend import MODE_LOG, model_id
from .components import unpack_cov
from .loads import target_transform
from .xr_compat import Dataset


def covariate_chain(name, pipe):
    """(a, unit) of a fitted covariate pipeline: model-space x = a u + b with u = ln(raw) (unit ``"ln <name>"``), decimal
    years (``"year"``) or the raw value (``name``).  Clips are the identity inside their range.  Anything else -- a step
    that is neither of these, a second log, a step after the scaler -- raises ``NotImplementedError``."""
    unit, a, scaled = name, 1.0, False
    for step_name, step in getattr(pipe, "steps", None) or [(None, pipe)]:
        if isinstance(step, (_pl.MetadataManager, _pl.ClipTransformer)):
            continue
        if scaled or not isinstance(step, (_pl.LogTransformer, _pl.TimeTransformer, _pl.StandardScaler, _pl.UnitScaler)):
            raise NotImplementedError(f"slopes need a (log | decimal year) + affine pipeline for {name!r}; "
                                      f"step {step_name!r} ({type(step).__name__}) of {type(pipe).__name__} is neither")
        if isinstance(step, (_pl.LogTransformer, _pl.TimeTransformer)):
            if unit != name:
                raise NotImplementedError(f"slopes need at most one log / decimal-year step for {name!r}")
            unit = f"ln {name}" if isinstance(step, _pl.LogTransformer) else "year"
        elif isinstance(step, _pl.StandardScaler):
            a, scaled = (1.0 / float(np.asarray(step.scale_).reshape(-1)[0]) if step.with_std else 1.0), True
        else:
            a, scaled = 1.0 / float(step.max_ - step.min_), True
    return a, unit


def _columns(model, wrt):
    names = list(model.dm.covariate_pipelines)
    if wrt is None:
        wrt = names
    wrt = [wrt] if isinstance(wrt, str) else list(wrt)
    if not wrt:
        raise ValueError("wrt is empty")
    for name in wrt:
        if name not in names:
            raise ValueError(f"unknown covariate {name!r}; the model has {names}")
    if len(set(wrt)) != len(wrt):
        raise ValueError(f"wrt lists a covariate more than once: {wrt}")
    return wrt, [names.index(name) for name in wrt]


def prior_mean_slopes(model, x, cols):
    """d m / d x_c of the prior mean function at model-space points x (m, d), by autograd through ``prior_mean`` (its
    parameter clamps act on ``.data`` and do not touch the graph of x) -> (len(cols), m) float64 numpy."""
    xg = x.detach().clone().requires_grad_(True)
    with torch.enable_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # the power law reads min(stage) as a float for its clamp: no graph needed
        pm = model.model.prior_mean(xg)
        grad = torch.autograd.grad(pm.sum(), xg, allow_unused=True)[0] if pm.requires_grad else None
    if grad is None:
        return np.zeros((len(cols), x.shape[0]))
    return grad.detach().to("cpu", torch.float64).numpy().T[cols]


def model_space(model, Xnew, cols):
    """(mean (P, m), cov (P, P, m), prior-mean slopes (P - 1, m)) in model space, P = 1 + len(cols), as float64 numpy."""
    model._device_ready()
    plan = model._plan
    mid = model_id(plan.model)
    lib = _lib.load()
    for c in cols:
        if int(lib.dgp_model_input_differentiable(mid, int(plan.d), int(c))) != 1:
            raise ValueError(f"the covariance is not differentiable in covariate column {c} (Matern-1/2 factor): no slope exists")
    x = Xnew.to(model.device, model.dtype).contiguous()
    model._eval_ready(x)
    with torch.no_grad():
        mean, packed = plan.predict_slopes(model._factor_theta, x, cols)
    dprior = prior_mean_slopes(model, x, cols)
    mean = mean.detach().to("cpu", torch.float64).numpy()
    packed = packed.detach().to("cpu", torch.float64).numpy()
    return mean, unpack_cov(packed), dprior


def slope(model, covariates, wrt=None, ci=0.95, return_cov=False):
    """``MarginalHIP.slope``: see the module docstring.  -> Dataset on (``wrt``, the covariates' coordinate): ``mean``,
    ``se``, ``lower`` / ``upper`` (the exact central ``ci`` interval), ``prob_positive`` = Phi(mean / se).  ``return_cov``
    adds ``cov`` on (``wrt``, ``wrt_2``, coordinate), the covariance between the slopes, and ``cov_value`` on (``wrt``,
    coordinate), the covariance of each slope with the fitted value (transformed target units) at every point.  The unit each
    slope is per is in ``attrs["per"]`` of the dataset and of every variable."""
    if not 0.0 < ci < 1.0:
        raise ValueError("ci must be in (0, 1)")
    wrt, cols = _columns(model, wrt)
    chains = [covariate_chain(name, model.dm.covariate_pipelines[name]) for name in wrt]
    mode, s, _t = target_transform(model.dm)
    Xnew = torch.tensor(model.dm.Xnew(covariates), dtype=model.dtype)
    mean, cov, dprior = model_space(model, Xnew, cols)
    a = np.asarray([c[0] for c in chains])[:, None]
    per = [c[1] for c in chains]
    mean_s = s * a * (mean[1:] + dprior)
    cov_s = s * s * a[:, None, :] * a[None, :, :] * cov[1:, 1:]
    se = np.sqrt(np.clip(np.einsum("aam->am", cov_s), 0.0, None))
    z = norm.ppf(1 - (1 - ci) / 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        prob = norm.cdf(np.where(se > 0, mean_s / se, np.sign(mean_s) * np.inf))
    coord = next(iter(covariates.coords))
    dims = ("wrt", coord)
    attrs = {"per": per}
    data = {"mean": (dims, mean_s, attrs), "se": (dims, se, attrs),
            "lower": (dims, mean_s - z * se, {"ci": ci, **attrs}), "upper": (dims, mean_s + z * se, {"ci": ci, **attrs}),
            "prob_positive": (dims, prob)}
    coords = {"wrt": np.array(wrt, dtype=object), coord: np.asarray(covariates.coords[coord].values)}
    if return_cov:
        data["cov"] = (("wrt", "wrt_2", coord), cov_s, attrs)
        data["cov_value"] = (dims, s * s * a * cov[1:, 0], attrs)
        coords["wrt_2"] = np.array(wrt, dtype=object)
    return Dataset(data, coords=coords, attrs={"ci": ci, "space": "log" if mode == MODE_LOG else "linear", "scale": s,
                                               "per": per})


def rating_exponent(model, covariates, ci=0.95):
    """``RatingGP.rating_exponent``: the local rating exponent d ln Q / d ln h = h d ln Q / d stage on the covariates'
    coordinate -- ``mean``, ``se``, ``lower`` / ``upper``, ``prob_positive`` (the posterior probability of an increasing
    rating at that stage and time).  Needs the log target transform (ln Q)."""
    mode, _s, _t = target_transform(model.dm)
    if mode != MODE_LOG:
        raise NotImplementedError("the rating exponent d ln Q / d ln h needs the log target transform")
    ds = slope(model, covariates, wrt="stage", ci=ci)
    if ds.attrs["per"] != ["stage"]:
        raise NotImplementedError("the rating exponent needs a stage pipeline that is affine in the stage itself")
    h = np.asarray(covariates["stage"].values, dtype=np.float64).reshape(-1)
    coord = next(iter(covariates.coords))
    data = {k: ((coord,), h * np.asarray(ds[k].values)[0]) for k in ("mean", "se", "lower", "upper")}
    data["prob_positive"] = ((coord,), np.asarray(ds["prob_positive"].values)[0])
    return Dataset(data, coords={coord: np.asarray(covariates.coords[coord].values)}, attrs={"ci": ci, "quantity": "d ln Q / d ln h"})
