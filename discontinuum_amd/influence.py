"""Exact influence of the samples a fit already has on every period's load: case deletion without refitting.

``sample_value`` says what one more sample would be worth; this module says what the samples in hand were worth: which
samples, storms or years of sampling drive each annual load, which could have been skipped, which single observation moves a
year's load by 15 %.  It is the case-deletion diagnostic of regression and the delete-a-group jackknife of WRTDS practice; the
reference can only answer by refitting once per deletion.  At FIXED hyperparameters the answer is closed-form.  With
S = K^^-1, alpha = S r, beta = S K* and, for a fold F of training rows, G_F = S_FF = M M^T, u = M^-1 alpha_F and
z_j = M^-1 beta_{F,j}, deleting F changes the latent posterior at the m points of a record exactly by

    mu'_j = mu_j - z_j^T u,        C'_jl = C_jl + z_j^T z_l        (sigma'^2_j = sigma^2_j + |z_j|^2)

and the period sums L_g = sum_{j in g} w_j c_j of ``loads.aggregate`` (c = exp(s f + t) for log targets, s f + t else) by

    log:     dL[F][g] = sum_{j in g} a_j expm1(s dmu_Fj + s^2 dsigma^2_Fj / 2),   a_j = w_j exp(s mu_j + t + s^2 C_jj / 2)
    linear:  dL[F][g] = sum_{j in g} s w_j dmu_Fj,    dVar[F][g] = |sum_{j in g} s w_j z_j|^2 >= 0  (deleting data never helps)

for all folds at once in one ``dgp_deletion_influence`` call (``backend.GPPlan.deletion_influence``).

Sign convention: every change is the value WITHOUT the fold minus the value with it.  What is held fixed: the hyperparameters,
the parameters of the prior mean and the fitted data transforms -- as in ``validation``; refitting them per deletion, the
standard error after deletion for log targets (an m x m pass per fold), ``*_many`` wrappers and the distributed path are out
of scope.  ``se_jackknife`` is the delete-a-group jackknife standard error of each period's load over the folds, reported when
the non-empty folds partition all observations: a DIAGNOSTIC to read beside the model-based ``se`` of ``aggregate``, not a
replacement (it holds the hyperparameters fixed and treats the folds as exchangeable).
"""
from __future__ import annotations

import numpy as np
import torch

from .backend import MODE_LOG
from .loads import _kept, _target_attrs, period_groups, target_transform
from .validation import _scheme_name, cv_folds
from .xr_compat import Dataset

SIGN = "without the fold minus with it"


def jackknife_se(load_without, fold_size, n_obs):
    """Delete-a-group jackknife standard error per period from the loads without each fold, (F, P): over the k non-empty
    folds sqrt((k - 1) / k sum_f (L_(f) - mean_f L_(f))^2).  NaN unless the non-empty folds hold all ``n_obs`` observations
    (fold ids are one per observation, so they then partition them) and k >= 2."""
    lw = np.asarray(load_without, dtype=np.float64)
    used = np.asarray(fold_size) > 0
    k = int(used.sum())
    if k < 2 or int(np.asarray(fold_size).sum()) != int(n_obs):
        return np.full(lw.shape[1], np.nan)
    rows = lw[used]
    return np.sqrt((k - 1) / k * ((rows - rows.mean(axis=0)) ** 2).sum(axis=0))


def influence(model, covariates, weights, folds="loo", freq="YE", max_bytes=None):
    """``MarginalHIP.influence``: for every fold of training observations (``validation.cv_folds`` schemes: "loo", a resample
    alias "YE" / "YE-SEP" / "QE" / "ME", an int k, ``("random", k, seed)`` or explicit ids, -1 = in no fold) the exact change of
    every period sum sum_{i in period} weights_i target_i over the points of ``covariates`` had the fold not been sampled --
    one ``predict`` and one ``dgp_deletion_influence``, no refit.  Hyperparameters held fixed; see the module docstring.

    -> Dataset on (``fold``, ``period``): ``load_change`` (without minus with), ``relative_change`` (divided by the period's
    load), ``load_without``, ``load`` (period), ``fold_size`` (fold), ``max_shift`` (fold) = max_j |dmu_j| / sigma_j over the
    record, a DFFITS-style screen, ``info`` (fold; 0, or the failing pivot of the fold's block, whose rows are NaN),
    ``se_jackknife`` (period; NaN unless the non-empty folds partition the observations) and, for linear targets,
    ``var_change`` (>= 0) and ``se_without``.  ``max_bytes``: raise ``ValueError`` instead of using a larger work area."""
    time_all = np.asarray(covariates.coords["time"].values).reshape(-1).astype("datetime64[ns]")
    w_all = np.asarray(weights, dtype=np.float64).reshape(-1)
    order, periods, labels, n_points, _dropped = _kept(*period_groups(time_all, w_all, freq))
    m, P = len(order), len(labels)
    obs_time = np.asarray(model.dm.data.target.coords["time"].values)
    groups, fold_labels = cv_folds(obs_time, folds)
    n_obs = len(groups)
    fold_size = np.bincount(groups[groups >= 0], minlength=len(fold_labels))
    mode, s, t = target_transform(model.dm)
    Xnew = torch.tensor(model.dm.Xnew(covariates), dtype=model.dtype)[torch.as_tensor(order)].to(model.device).contiguous()
    model._eval_ready(Xnew)
    with torch.no_grad():
        kmean, kvar = model._plan.predict(model._factor_theta, Xnew)
        mapped = (s * (kmean + model.model.prior_mean(Xnew)) + t).double()
        var = kvar.double().clamp(min=0.0)
        w_t = torch.as_tensor(w_all[order], dtype=torch.float64, device=mapped.device)
        a = w_t * torch.exp(mapped + 0.5 * s * s * var) if mode == MODE_LOG else s * w_t
        point = (a if mode == MODE_LOG else w_t * mapped).cpu().numpy()
        inv_sd = torch.where(var > 0, 1.0 / torch.sqrt(var), torch.zeros_like(var))
        dload, dvar, shift, info = model._plan.deletion_influence(
            model._factor_theta, Xnew, torch.as_tensor(groups, dtype=torch.int64), a.contiguous(), s, periods, P, mode,
            inv_sd=inv_sd, max_bytes=max_bytes)
        var_now = None
        if dvar is not None:
            _mean, cov_d = model._plan.posterior_period_moments(model._factor_theta, Xnew, mapped.to(model.dtype).contiguous(),
                                                                s * s, w_all[order], periods, P, mode)
            var_now = np.clip(np.diagonal(cov_d.cpu().numpy()), 0.0, None)
    load = np.bincount(periods, weights=point, minlength=P).astype(np.float64)
    dload = dload.cpu().numpy()[: len(fold_labels)]
    info = info.cpu().numpy()[: len(fold_labels)]
    shift = shift.cpu().numpy()[: len(fold_labels)]
    without = load[None, :] + dload
    with np.errstate(divide="ignore", invalid="ignore"):
        relative = np.where(load[None, :] != 0, dload / load[None, :], np.nan)
    attrs = _target_attrs(model.dm)
    data = {
        "load_change": (("fold", "period"), dload, attrs),
        "relative_change": (("fold", "period"), relative),
        "load_without": (("fold", "period"), without, attrs),
        "load": ("period", load, attrs),
        "fold_size": ("fold", fold_size),
        "max_shift": ("fold", shift),
        "info": ("fold", info),
        "se_jackknife": ("period", jackknife_se(without, fold_size, n_obs), attrs),
        "n_points": ("period", n_points),
    }
    if dvar is not None:
        dvar = dvar.cpu().numpy()[: len(fold_labels)]
        data["var_change"] = (("fold", "period"), dvar, attrs)
        data["se_without"] = (("fold", "period"), np.sqrt(var_now[None, :] + dvar), attrs)
    return Dataset(data, coords={"fold": fold_labels, "period": labels},
                   attrs=dict(attrs, freq=freq, scheme=_scheme_name(folds), hyperparameters="held fixed", sign=SIGN))


__all__ = ["influence", "jackknife_se", "SIGN"]
