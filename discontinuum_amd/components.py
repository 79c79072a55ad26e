"""Exact posterior decomposition of a fitted model into the additive parts of its covariance.

Both shipped covariances are sums of named parts -- loadest-gp: seasonal + covariates + residual; rating-gp: shift_1 +
shift_2 (gated to low stages) + bend (gated to high stages) + base + periodic -- and a GP with an additive covariance is a
sum of independent GPs a priori, f = sum_c f_c.  Given the data the parts are jointly Gaussian: with T = L^-1 and
alpha = K^^-1 r from the factorisation the engine holds, K_c the Gram of part c and V_c = T K_c(X, X*)

    E[f_c(x*) | y]              = K_c(x*, X) alpha
    Cov[f_c(x*), f_c'(x*) | y]  = delta_cc' k_c(x*, x*) - V_c[:, *]^T V_c'[:, *]

which ``dgp_predict_terms`` evaluates for all parts in one pass (``backend.GPPlan.predict_terms``): one pair evaluation per
matrix entry, the prediction's GEMM at C times its width, one reduction.  The means sum to the latent mean of ``predict`` and
the C x C covariance at a point to its variance.  The cross-covariances matter: the parts are strongly anti-correlated a
posteriori (the data pin their sum, not each of them), so the standard error of a merged part -- the total shift of a rating,
"everything that varies in time" -- is not the root sum of squares of its members' standard errors.

Everything is reported in the units of the TRANSFORMED target (log concentration, log discharge, or the standardised
target): a part contributes s f_c with (s, t) the target scaler's scale and offset (``loads.target_transform``), and the
prior mean function is one more, deterministic, component ``"mean"`` = s m(x) + t.  The components' means add up to the
transformed prediction.  For log targets each part is a multiplicative ``factor`` exp(s f_c) of the prediction, lognormal with
exact quantiles.  Per-part period loads are deliberately absent: in log space the parts multiply, so no exact per-part load
exists.
"""
from __future__ import annotations

import numpy as np
import torch
from scipy.stats import norm

from .backend import MODE_LOG
from .loads import target_transform
from .xr_compat import Dataset

MEAN_COMPONENT = "mean"


def component_names(model):
    """Names of the covariance's additive parts in the device's order: the model class's ``component_names`` for the two
    fused covariances, ``term_0 ...`` for a generic (lowered composite) one."""
    count = int(model._plan.nterms)
    if str(model._plan.model).startswith("composite:"):
        return tuple(f"term_{c}" for c in range(count))
    names = tuple(getattr(model, "component_names", ()) or ())
    if len(names) != count:
        raise RuntimeError(f"{type(model).__name__}.component_names lists {len(names)} parts, the covariance has {count}")
    return names


def unpack_cov(packed):
    """(C (C + 1) / 2, m) packed lower triangles (entry (c, c'), c' <= c, at c (c + 1) / 2 + c') -> symmetric (C, C, m)."""
    packed = np.asarray(packed, dtype=np.float64)
    C = int((np.sqrt(8 * packed.shape[0] + 1) - 1) / 2 + 0.5)
    if C * (C + 1) // 2 != packed.shape[0]:
        raise ValueError(f"{packed.shape[0]} rows are no packed triangle")
    full = np.empty((C, C) + packed.shape[1:], dtype=np.float64)
    for c in range(C):
        for e in range(c + 1):
            full[c, e] = full[e, c] = packed[c * (c + 1) // 2 + e]
    return full


def merge_matrix(names, groups):
    """-> (merged names, G): G (len(merged), len(names)) of 0 / 1 maps the parts onto the merged components.  A group takes
    the place of its first member; parts no group lists stay separate.  Unknown, repeated or reserved names raise."""
    names = tuple(names)
    groups = dict(groups or {})
    owner = {}
    for g, members in groups.items():
        members = (members,) if isinstance(members, str) else tuple(members)
        if not members:
            raise ValueError(f"group {g!r} is empty")
        if g == MEAN_COMPONENT or (g in names and g not in members):
            raise ValueError(f"group name {g!r} is already a component")
        for name in members:
            if name not in names:
                raise ValueError(f"unknown component {name!r}; the model has {names}")
            if name in owner:
                raise ValueError(f"component {name!r} is listed more than once")
            owner[name] = g
    merged = []
    for name in names:
        label = owner.get(name, name)
        if label not in merged:
            merged.append(label)
    G = np.zeros((len(merged), len(names)))
    for c, name in enumerate(names):
        G[merged.index(owner.get(name, name)), c] = 1.0
    return tuple(merged), G


def model_space(model, Xnew):
    """(names, mean (C, m), cov (C, C, m), prior mean (m,)) of the parts at model-space points ``Xnew``, as float64 numpy."""
    x = Xnew.to(model.device, model.dtype).contiguous()
    model._eval_ready(x)
    with torch.no_grad():
        mean, packed = model._plan.predict_terms(model._factor_theta, x)
        prior = model.model.prior_mean(x)
    mean = mean.detach().to("cpu", torch.float64).numpy()
    packed = packed.detach().to("cpu", torch.float64).numpy()
    prior = np.broadcast_to(prior.detach().to("cpu", torch.float64).numpy().reshape(-1), (x.shape[0],))
    return component_names(model), mean, unpack_cov(packed), prior


def decompose(model, covariates, groups=None, ci=0.95, return_cov=False):
    """``MarginalHIP.decompose``: see the module docstring.  -> Dataset on (``component``, the covariates' coordinate):
    ``mean`` and ``se`` of every component in the units of the transformed target -- the parts of the covariance in the
    model's order (merged as ``groups`` says), then ``"mean"``, the prior mean function s m(x) + t with ``se`` 0.  Log
    targets also get ``factor`` = exp(mean) and ``factor_lower`` / ``factor_upper`` = exp(mean -+ z se), the exact central
    ``ci`` interval of the part's multiplicative contribution.  ``return_cov`` adds ``cov`` on (``component``,
    ``component_2``, coordinate): the covariance between the (merged) components at every point."""
    if not 0.0 < ci < 1.0:
        raise ValueError("ci must be in (0, 1)")
    mode, s, t = target_transform(model.dm)
    Xnew = torch.tensor(model.dm.Xnew(covariates), dtype=model.dtype)
    names, mean, cov, prior = model_space(model, Xnew)
    merged, G = merge_matrix(names, groups)
    mean = s * (G @ mean)
    cov = s * s * np.einsum("ac,cem,be->abm", G, cov, G)
    k, m = len(merged), mean.shape[1]
    labels = np.array(list(merged) + [MEAN_COMPONENT], dtype=object)
    mean_all = np.concatenate([mean, (s * prior + t)[None, :]], axis=0)
    var = np.clip(np.einsum("aam->am", cov), 0.0, None)
    se_all = np.concatenate([np.sqrt(var), np.zeros((1, m))], axis=0)
    coord = next(iter(covariates.coords))
    dims = ("component", coord)
    data = {"mean": (dims, mean_all), "se": (dims, se_all)}
    if mode == MODE_LOG:
        z = norm.ppf(1 - (1 - ci) / 2)
        data["factor"] = (dims, np.exp(mean_all))
        data["factor_lower"] = (dims, np.exp(mean_all - z * se_all), {"ci": ci})
        data["factor_upper"] = (dims, np.exp(mean_all + z * se_all), {"ci": ci})
    coords = {"component": labels, coord: np.asarray(covariates.coords[coord].values)}
    if return_cov:
        cov_all = np.zeros((k + 1, k + 1, m))
        cov_all[:k, :k] = cov
        data["cov"] = (("component", "component_2", coord), cov_all)
        coords["component_2"] = labels
    return Dataset(data, coords=coords, attrs={"ci": ci, "space": "log" if mode == MODE_LOG else "linear",
                                               "scale": s, "offset": t, "parts": list(names)})
