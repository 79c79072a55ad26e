"""How well the data determine the hyperparameters: their exact Fisher information from the factorisation the engine holds.

Every posterior product of this package is exact AT the fitted hyperparameters; this module says how well those are known.
For the Gaussian marginal likelihood y ~ N(m, K^) the expected information (Mardia & Marshall 1984) is

    F_ab = 1/2 tr(K^^-1 d_a K^ K^^-1 d_b K^)  +  d_a m^T K^^-1 d_b m

-- first derivatives only, positive semi-definite everywhere, and equal to the covariance of the score under the model.
Training stops on an iteration budget or on early stopping, not at a stationary point, where the observed Hessian is
indefinite; the expected information is not.

The device computes the covariance block over DIRECTIONS of K^ (``GPPlan.fisher`` / ``dgp_fisher``: the P constrained kernel
hyperparameters, then up to 8 diagonal directions for learned noise terms).  The host takes the Jacobians of the model's own
map  raw parameters -> (theta, prior mean m(X), noise diagonal)  by forward-mode differentiation, one pass per raw value,
and assembles

    F_raw = J_theta,d^T F_dev J_theta,d + J_m^T K^^-1 J_m

(K^^-1 J_m through the held factor, ``GPPlan.whiten``), adds the Hessian of -log prior in raw space when asked to, and inverts
on the identified subspace.  Units: the UN-normalised log-likelihood -- the objective the engine minimises is this divided by n.

PROPAGATION into predictions and loads (``raw_covariance``, ``prediction_jacobians``, ``predict_marginalized``,
``period_hyper_covariance``): with Sigma_raw the inverse above and J_mu = d E[f* | y, raw] / d raw the exact Jacobian of the
posterior mean at the prediction points (``GPPlan.predict_sensitivity`` / ``dgp_predict_sensitivity`` on the held
factorisation, mapped to raw space by the same forward-mode Jacobians), the delta method gives

    Var_total[f*] = Var[f* | raw^] + J_mu Sigma_raw J_mu^T.

The Jacobians and Sigma_raw are exact; the propagation is FIRST ORDER in Sigma_raw (second-order terms such as
1/2 tr(Hessian(sigma^2) Sigma_raw) are not included).
"""
from __future__ import annotations

from contextlib import contextmanager
from statistics import NormalDist

import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

from .backend import MODE_LOG
from .gp.mll import ExactMarginalLogLikelihood
from .xr_compat import Dataset

EIG_FLOOR = 1e-10  # a direction of the unit-diagonal scaling with an eigenvalue below this is reported as unidentified
MAX_DIAG = 8       # diagonal directions of ``dgp_fisher``


@contextmanager
def _substituted(engine, values):
    """Run the engine's modules with substituted parameter values, ``values`` = {id(parameter): tensor}: every slot that
    holds one of the parameters -- shared modules (the gate of the rating kernel, a likelihood the model also holds) are
    visited once -- reads the substitute until the block ends; the parameters themselves are put back whatever happens."""
    slots, seen = [], set()
    for root in (engine.model, engine.likelihood):
        for mod in root.modules():
            if id(mod) in seen:
                continue
            seen.add(id(mod))
            slots += [(mod, name, p) for name, p in mod._parameters.items() if p is not None and id(p) in values]
    try:
        for mod, name, p in slots:
            mod._parameters[name] = values[id(p)]
        yield
    finally:
        for mod, name, p in slots:
            mod._parameters[name] = p


def _host_map(engine, x=None, theta_fn=None):
    """(theta, prior mean m(X), noise diagonal) of the engine's model at its training rows: what one fit step is handed.
    ``x`` / ``theta_fn``: the model-space training rows on the device and the lowered theta builder, when the engine's own
    device state is not to be used (``multisite_fit.hyperparameter_uncertainty_many``)."""
    x = engine._train_x if x is None else x
    theta_fn = engine._theta_fn if theta_fn is None else theta_fn
    return theta_fn(), engine.model.prior_mean(x), engine.likelihood.train_noise(x.device, engine.dtype)


def leaves(engine):
    """[(name, parameter)]: every leaf of ``model.parameters()`` and ``likelihood.parameters()`` that requires grad, in
    ``named_parameters()`` order, the likelihood's own (when the model does not hold it) prefixed ``likelihood.``."""
    seen, out = set(), []
    for prefix, mod in (("", engine.model), ("likelihood.", engine.likelihood)):
        for name, p in mod.named_parameters():
            if p.requires_grad and id(p) not in seen:
                seen.add(id(p))
                out.append((prefix + name, p))
    return out


def _constraints(engine, params):
    """Per leaf the constraint module that maps it to its constrained value (``raw_x`` -> ``raw_x_constraint``) or None."""
    owner = {}
    for root in (engine.model, engine.likelihood):
        for mod in root.modules():
            for pname, p in mod.named_parameters(recurse=False):
                owner.setdefault(id(p), getattr(mod, pname + "_constraint", None))
    return [owner.get(id(p)) for _n, p in params]


def _element_names(params):
    names = []
    for name, p in params:
        names += [name] if p.numel() == 1 else [f"{name}[{i}]" for i in range(p.numel())]
    return names


def _on_clamp(engine, params, x=None):
    """Flat boolean mask of raw values that sit on a data clamp of the model (``model.parameter_clamps(train_x)`` ->
    {parameter name: (lo or None, hi or None)}): the model's forward resets such a value on every call, so the likelihood
    does not move with it."""
    hook = getattr(engine.model, "parameter_clamps", None)
    bounds = hook(engine._train_x if x is None else x) if callable(hook) else {}
    mask = []
    for name, p in params:
        lo, hi = bounds.get(name, (None, None))
        v = p.detach().reshape(-1).to(torch.float64)
        m = torch.zeros(v.numel(), dtype=torch.bool)
        if lo is not None:
            m |= v <= float(lo)
        if hi is not None:
            m |= v >= float(hi)
        mask += m.tolist()
    return np.asarray(mask, dtype=bool)


def jacobians(engine, params=None, x=None, theta_fn=None):
    """Forward-mode Jacobians of the host map at the current (clamped) parameters, one pass per raw value:
    -> (J_theta (P, R), J_m (n, R) on the engine's device, J_noise (n, R) on the device), R = number of raw values."""
    params = leaves(engine) if params is None else params
    base = {id(p): p.detach() for _n, p in params}
    with torch.no_grad(), _substituted(engine, base):
        theta0, mean0, noise0 = _host_map(engine, x, theta_fn)
    P, n = theta0.numel(), mean0.shape[0]
    dev = mean0.device
    cols_t, cols_m, cols_s = [], [], []
    for _name, p in params:
        for i in range(p.numel()):
            tangent = torch.zeros_like(p.detach())
            tangent.reshape(-1)[i] = 1.0
            with fwAD.dual_level():
                reps = dict(base)
                reps[id(p)] = fwAD.make_dual(p.detach(), tangent)
                with _substituted(engine, reps):
                    theta, mean, noise = _host_map(engine, x, theta_fn)
                tt, tm, ts = (fwAD.unpack_dual(v).tangent for v in (theta, mean, noise))
                cols_t.append(torch.zeros(P, dtype=torch.float64) if tt is None else tt.detach().to("cpu", torch.float64).reshape(P).clone())
                cols_m.append(torch.zeros(n, dtype=torch.float64, device=dev) if tm is None else tm.detach().to(torch.float64).reshape(n).clone())
                cols_s.append(torch.zeros(n, dtype=torch.float64, device=dev) if ts is None else ts.detach().to(torch.float64).expand(n).clone())
    return torch.stack(cols_t, 1), torch.stack(cols_m, 1), torch.stack(cols_s, 1)


def prior_hessian(engine, params=None):
    """Hessian of -log prior with respect to the raw values (R, R), by autograd on the host."""
    params = leaves(engine) if params is None else params
    mll = ExactMarginalLogLikelihood(engine.likelihood, engine.model)
    sizes = [p.numel() for _n, p in params]
    flat0 = torch.cat([p.detach().reshape(-1).to(torch.float64) for _n, p in params])

    def neg_log_prior(flat):
        reps, o = {}, 0
        for (_n, p), k in zip(params, sizes):
            reps[id(p)] = flat[o:o + k].reshape(p.shape).to(p.dtype)
            o += k
        with _substituted(engine, reps):
            return -mll.log_prior().reshape(())

    H = torch.autograd.functional.hessian(neg_log_prior, flat0)
    return 0.5 * (H + H.T).detach()


def invert_information(M, active):
    """Inverse of the symmetric matrix ``M`` on the identified subspace of its ``active`` rows: scale to unit diagonal,
    eigen-decompose, drop every direction whose scaled eigenvalue is below ``EIG_FLOOR`` (reported, never inverted) and
    pseudo-invert on the rest.  -> (cov (R, R) with NaN outside the active block, unidentified directions (k, R) in the
    scaled coordinates, smallest scaled eigenvalue, positive_definite)."""
    M = np.asarray(M, dtype=np.float64)
    R = M.shape[0]
    idx = np.nonzero(active)[0]
    cov = np.full((R, R), np.nan)
    if idx.size == 0:
        return cov, np.zeros((0, R)), float("nan"), False
    A = M[np.ix_(idx, idx)]
    A = 0.5 * (A + A.T)
    dg = np.abs(np.diag(A))
    s = np.where(dg > 0, np.sqrt(dg), 1.0)
    lam, V = np.linalg.eigh(A / np.outer(s, s))
    good = lam >= EIG_FLOOR
    Vg = V[:, good]
    inv = (Vg / lam[good]) @ Vg.T / np.outer(s, s)
    cov[np.ix_(idx, idx)] = inv
    unident = np.zeros((int((~good).sum()), R))
    unident[:, idx] = V[:, ~good].T
    return cov, unident, float(lam.min()), bool(good.all())


def assemble(F_dev, J_dir, W, on_clamp):
    """F_raw = J_dir^T F_dev J_dir + W^T W over the raw values, with the rows and columns of raw values on a clamp zeroed;
    ``J_dir`` (P + E, R) maps raw values to directions, ``W`` = L^-1 J_m (n, R).  -> (F_raw (R, R), active (R,))."""
    J_dir, W = np.array(J_dir, dtype=np.float64), np.array(W, dtype=np.float64)
    J_dir[:, on_clamp] = 0.0
    W[:, on_clamp] = 0.0
    active = (np.abs(J_dir).max(axis=0) > 0) | (np.abs(W).max(axis=0) > 0 if W.shape[0] else False)
    F = J_dir.T @ np.asarray(F_dev, dtype=np.float64) @ J_dir + W.T @ W
    F = 0.5 * (F + F.T)
    F[~active] = 0.0
    F[:, ~active] = 0.0
    return F, active


def noise_directions(J_noise):
    """The diagonal directions of the noise Jacobian: one per raw value the noise diagonal depends on, scaled to largest
    entry 1 (a learned homoskedastic term gives a vector of ones).  -> (directions (E, n) tensor or None, rows (E, R) that
    map raw values onto them)."""
    amp = J_noise.abs().amax(dim=0).to("cpu")
    ks = [k for k in range(J_noise.shape[1]) if float(amp[k]) > 0.0]
    if len(ks) > MAX_DIAG:
        raise NotImplementedError(f"the noise model has {len(ks)} learned parameters; dgp_fisher takes {MAX_DIAG} diagonal directions")
    rows = np.zeros((len(ks), J_noise.shape[1]))
    if not ks:
        return None, rows
    dirs = []
    for e, k in enumerate(ks):
        rows[e, k] = float(amp[k])
        dirs.append(J_noise[:, k] / amp[k].to(J_noise.device))
    return torch.stack(dirs), rows


def invert_with_prior(F_raw, active, H, prior):
    """``invert_information`` of F_raw (+ the prior's Hessian H on the active block when ``prior``): the one inversion behind
    ``hyperparameter_uncertainty``'s ``cov_raw`` and ``raw_covariance``."""
    return invert_information(F_raw + (np.where(np.outer(active, active), H, 0.0) if prior else 0.0), active)


def summarise(engine, params, F_raw, active, H, ci, prior):
    """The result Dataset from the raw-space information (see ``hyperparameter_uncertainty``)."""
    if not 0.0 < ci < 1.0:
        raise ValueError("ci must be in (0, 1)")
    z = NormalDist().inv_cdf(1 - (1 - ci) / 2)
    names = _element_names(params)
    cov, unident, lam_min, pd = invert_with_prior(F_raw, active, H, prior)
    with np.errstate(invalid="ignore"):
        se_raw = np.sqrt(np.diag(cov))
        corr = cov / np.outer(se_raw, se_raw)
    cons = _constraints(engine, params)
    est, slope, lower, upper, o = [], [], [], [], 0
    for (_name, p), c in zip(params, cons):
        k = p.numel()
        raw = p.detach().reshape(-1).to(torch.float64).clone().requires_grad_(True)
        f = (lambda v: v) if c is None else c.transform
        with torch.enable_grad():
            val = f(raw)
            (g,) = torch.autograd.grad(val.sum(), raw)
        s = torch.as_tensor(np.nan_to_num(se_raw[o:o + k], nan=0.0))
        with torch.no_grad():
            a, b = f(raw.detach() - z * s), f(raw.detach() + z * s)
        nan = torch.as_tensor(~active[o:o + k])
        a, b = torch.minimum(a, b).masked_fill(nan, float("nan")), torch.maximum(a, b).masked_fill(nan, float("nan"))
        est += val.detach().tolist()
        slope += g.abs().tolist()
        lower += a.tolist()
        upper += b.tolist()
        o += k
    se = np.asarray(slope) * se_raw
    dims, d2 = ("parameter",), ("parameter", "parameter_2")
    coords = {"parameter": np.array(names, dtype=object), "parameter_2": np.array(names, dtype=object),
              "direction": np.arange(unident.shape[0])}
    data = {"estimate": (dims, np.asarray(est)), "se": (dims, se), "lower": (dims, np.asarray(lower), {"ci": ci}),
            "upper": (dims, np.asarray(upper), {"ci": ci}), "se_raw": (dims, se_raw), "active": (dims, np.asarray(active, dtype=bool)),
            "cov_raw": (d2, cov), "corr": (d2, corr), "information": (d2, F_raw),
            "unidentified": (("direction", "parameter"), unident)}
    attrs = {"ci": ci, "prior": bool(prior), "n_eff": int(active.sum()) - unident.shape[0], "positive_definite": pd,
             "min_scaled_eigenvalue": lam_min, "units": "un-normalised log-likelihood (the training objective times n)"}
    return Dataset(data, coords=coords, attrs=attrs)


def host_jacobians(engine):
    """(params, J_theta, J_m, J_noise) at the held state: ``leaves`` and ``jacobians``, for callers that need them twice."""
    params = leaves(engine)
    return (params,) + tuple(jacobians(engine, params))


def raw_information(engine, x=None, host=None):
    """(params, F_raw, active) of one fitted engine whose factorisation is held (``_eval_ready`` has run).  ``x``: model-space
    prediction points the factorisation was prepared for -- the data clamps are then judged on [X; X*], as the model's
    forward sees them; ``host``: ``host_jacobians(engine)`` if the caller already has them."""
    params, J_theta, J_m, J_noise = host_jacobians(engine) if host is None else host
    plan = engine._plan
    dirs, rows = noise_directions(J_noise)
    with torch.no_grad():
        F_dev = plan.fisher(engine._factor_theta, None if dirs is None else dirs.to(engine.dtype).contiguous())
        W = plan.whiten(J_m) if bool((J_m != 0).any()) else J_m
    J_dir = np.concatenate([J_theta.numpy(), rows], axis=0)
    F_raw, active = assemble(F_dev.detach().to("cpu", torch.float64).numpy(), J_dir, W.detach().to("cpu", torch.float64).numpy(),
                             _on_clamp(engine, params, None if x is None else torch.cat([engine._train_x, x])))
    return params, F_raw, active


def hyperparameter_uncertainty(engine, ci=0.95, prior=True):
    """``MarginalHIP.hyperparameter_uncertainty``: standard errors, intervals and correlations of every trainable parameter
    at the fitted values, from the exact Fisher information of the marginal likelihood (one ``dgp_fisher`` on the held
    factorisation; nothing is refitted).  -> Dataset indexed by ``parameter`` (one entry per raw value, in
    ``named_parameters()`` order):

    ``estimate`` the constrained value; ``se`` its standard error (delta method through the constraint); ``lower`` / ``upper``
    the raw estimate -+ z se_raw pushed through the monotone constraint, so they respect its bounds; ``se_raw``; ``active``
    (False for a parameter the likelihood does not move with: one held on a data clamp, or with an all-zero Jacobian -- its
    errors are NaN); ``cov_raw`` / ``corr`` on (``parameter``, ``parameter_2``); ``information``, F_raw before the prior;
    ``unidentified`` on (``direction``, ``parameter``): the directions (in the unit-diagonal scaling of the inverted matrix)
    whose scaled eigenvalue is below 1e-10 -- the inverse is the pseudo-inverse on their complement, never an inflated
    number.  Attributes: ``n_eff`` (identified directions), ``positive_definite``, ``min_scaled_eigenvalue``.

    ``prior=True`` adds the Hessian of -log prior in raw space (the curvature the MAP objective really has).  Everything is
    in UN-normalised log-likelihood units: the objective the engine minimises is divided by n, this is not.  This result
    describes the hyperparameters alone; ``predict_marginalized`` and ``aggregate(..., hyperparameters=True)`` propagate it
    into predictions and loads (first order in ``cov_raw``)."""
    engine._eval_ready()
    params, F_raw, active = raw_information(engine)
    H = prior_hessian(engine, params).numpy() if prior else np.zeros_like(F_raw)
    return summarise(engine, params, F_raw, active, H, ci, prior)


# ---------------------------------------------------------------------------------------------------- propagation
def raw_covariance(engine, prior=True, x=None, host=None):
    """Sigma_raw, the covariance of the raw parameters that ``hyperparameter_uncertainty`` reports as ``cov_raw``, with
    ZEROS where that one holds NaN: -> (params, cov_raw (R, R), active (R,), unidentified (k, R)).  Raw values that are
    inactive or sit on a data clamp and unidentified directions contribute exactly zero -- the pseudo-inverse on the
    identified subspace, never an inflated number.  ``x``: the model-space prediction points (on the engine's device): the
    factorisation is prepared for them (``_eval_ready(x)``) and the data clamps are judged on [X; X*] -- a rating record with
    a test stage below the training minimum holds ``c`` on that clamp, and Sigma_raw is then the covariance of the other
    parameters with ``c`` FIXED, matching the zero column of ``prediction_jacobians``; None: the training rows only."""
    x = None if x is None else x.to(engine.device, engine.dtype).contiguous()
    if host is None:  # (a caller that hands over ``host`` took it after its own ``_eval_ready(x)``)
        engine._eval_ready(x)
    params, F_raw, active = raw_information(engine, x, host)
    H = prior_hessian(engine, params).numpy() if prior else np.zeros_like(F_raw)
    cov, unident, _lam_min, _pd = invert_with_prior(F_raw, active, H, prior)
    return params, np.nan_to_num(cov, nan=0.0), active, unident


def _forward_columns(engine, params, fn, size):
    """Forward-mode Jacobian of the 1-D tensor ``fn()`` (length ``size``) with respect to every raw value, one pass per
    value -> (size, R) float64 on the CPU; a value ``fn`` does not depend on gives a zero column."""
    base = {id(p): p.detach() for _n, p in params}
    cols = []
    for _name, p in params:
        for i in range(p.numel()):
            tangent = torch.zeros_like(p.detach())
            tangent.reshape(-1)[i] = 1.0
            with fwAD.dual_level():
                reps = dict(base)
                reps[id(p)] = fwAD.make_dual(p.detach(), tangent)
                with _substituted(engine, reps):
                    out = fn()
                tan = fwAD.unpack_dual(out).tangent if torch.is_tensor(out) else None
                cols.append(torch.zeros(size, dtype=torch.float64) if tan is None
                            else tan.detach().to("cpu", torch.float64).reshape(-1).expand(size).clone())
    return torch.stack(cols, 1)


def mean_jacobian_at(engine, x, params=None):
    """Forward-mode Jacobian of ``prior_mean`` at the model-space TEST rows ``x`` (m, d) -> (m, R) float64 on the CPU: the
    sibling of ``jacobians``' J_m (training rows), which existing callers keep getting unchanged."""
    params = leaves(engine) if params is None else params
    return _forward_columns(engine, params, lambda: engine.model.prior_mean(x), x.shape[0])


def _predictive_noise_jacobian(engine, params, m):
    """d (what ``predictive_noise`` adds to the latent variance) / d raw -> (m, R): the fixed part does not move; a learned
    homoskedastic term moves every point alike."""
    if getattr(engine.likelihood, "second_noise_covar", None) is None:
        return torch.zeros(m, sum(p.numel() for _n, p in params), dtype=torch.float64)
    return _forward_columns(engine, params, lambda: engine.likelihood.second_noise.reshape(-1), m)


def prediction_jacobians(engine, x, pred_noise=False, return_var=True, host=None):
    """Exact Jacobians of the model-space posterior at the points ``x`` (m, d) with respect to every raw value, at the fitted
    values: -> (J_mu (m, R), J_var (m, R)) float64 numpy, R raw values in ``leaves`` order.  ONE
    ``GPPlan.predict_sensitivity`` on the held factorisation gives the Jacobians over the device's directions; kernel rows
    are mapped through J_theta, diagonal rows through ``noise_directions``, right-hand-side rows are the non-zero columns of
    J_m at the training rows, and the forward-mode Jacobian of ``prior_mean`` at the test rows is added to J_mu.
    ``pred_noise`` adds the raw derivative of the predictive noise to J_var.  Columns of raw values that sit on a data clamp
    (evaluated after ``_eval_ready(x)``: the rating model's clamps see [X; X*]) are zero.  The Jacobians are exact; any
    variance built from them and ``raw_covariance`` is first order in that covariance.  ``return_var=False`` skips the
    device's quadratic-form pass (its dominant cost) and returns J_var = None; ``host``: ``host_jacobians(engine)`` taken after
    ``_eval_ready(x)``, if the caller already has them."""
    x = x.to(engine.device, engine.dtype).contiguous()
    if host is None:
        engine._eval_ready(x)
    params, J_theta, J_m, J_noise = host_jacobians(engine) if host is None else host
    dirs, rows = noise_directions(J_noise)
    amp = J_m.abs().amax(dim=0).to("cpu")
    ks = [k for k in range(J_m.shape[1]) if float(amp[k]) > 0.0]
    if len(ks) > MAX_DIAG:
        raise NotImplementedError(f"the prior mean has {len(ks)} parameters; dgp_predict_sensitivity takes {MAX_DIAG} right-hand sides")
    rhs = J_m[:, ks].T.to(engine.dtype).contiguous() if ks else None
    with torch.no_grad():
        dmean, dvar = engine._plan.predict_sensitivity(engine._factor_theta, x,
                                                       None if dirs is None else dirs.to(engine.dtype).contiguous(), rhs,
                                                       return_var=return_var)
    dmean = dmean.detach().to("cpu", torch.float64).numpy()
    P, E = J_theta.shape[0], rows.shape[0]
    J_dir = np.concatenate([J_theta.numpy(), rows], axis=0)  # (P + E, R): raw values -> directions of K^
    J_mu = dmean[:P + E].T @ J_dir
    for c, k in enumerate(ks):
        J_mu[:, k] += dmean[P + E + c]
    J_mu += mean_jacobian_at(engine, x, params).numpy()
    on = _on_clamp(engine, params, torch.cat([engine._train_x, x]))
    J_mu[:, on] = 0.0
    if not return_var:
        return J_mu, None
    J_var = dvar.detach().to("cpu", torch.float64).numpy().T @ J_dir
    if pred_noise:
        J_var += _predictive_noise_jacobian(engine, params, x.shape[0]).numpy()
    J_var[:, on] = 0.0
    return J_mu, J_var


def predict_marginalized(engine, covariates, ci=0.95, prior=True, pred_noise=False):
    """``MarginalHIP.predict_marginalized``: ``predict`` with the hyperparameters' uncertainty propagated to FIRST ORDER
    (delta method / Laplace): Var_total[f*] = Var[f* | raw^] + J_mu Sigma_raw J_mu^T in model space, J_mu the exact Jacobian of
    the posterior mean (``prediction_jacobians``) and Sigma_raw the exact inverse Fisher information (``raw_covariance``).
    -> Dataset on the covariates' coordinates: ``mean`` (``predict``'s target), ``se_plugin`` (``predict``'s standard error,
    bitwise), ``se_hyper`` and ``se`` (the total), both through ``dm.error_pipeline.inverse_transform`` of the model-space
    variance; ``lower`` / ``upper`` = ``dm.y_t(mu -+ q sqrt(var_total))``, the central ``ci`` interval of the monotone target
    transform (additive for a standardised target, multiplicative for a log target); ``inflation`` = var_total / var_plugin;
    ``var_plugin`` / ``var_hyper`` in model space.  Attributes: ``ci``, ``prior``, ``n_eff``, ``n_unidentified``, ``order``.
    ``pred_noise`` is accepted and ignored exactly as ``predict`` ignores it (the plug-in variance is ``predict``'s, which always
    carries the likelihood's predictive noise, and the first-order term involves J_mu only).  Second-order terms are not
    included; flow-normalized loads, exceedance and the ``*_many`` wrappers do not propagate."""
    if not 0.0 < ci < 1.0:
        raise ValueError("ci must be in (0, 1)")
    Xnew = torch.tensor(engine.dm.Xnew(covariates), dtype=engine.dtype)
    mu, var = engine._model_space_predict(Xnew)
    x = Xnew.to(engine.device, engine.dtype).contiguous()
    host = host_jacobians(engine)  # (``_model_space_predict`` has run ``_eval_ready(x)``)
    J_mu, _none = prediction_jacobians(engine, x, return_var=False, host=host)
    params, cov_raw, active, unident = raw_covariance(engine, prior=prior, x=x, host=host)
    mu_h, var_plugin = mu.cpu().numpy(), var.cpu().numpy()
    var_hyper = np.einsum("ik,kl,il->i", J_mu, cov_raw, J_mu)
    var_total = var_plugin.astype(np.float64) + var_hyper
    q = NormalDist().inv_cdf(1 - (1 - ci) / 2)
    sd = np.sqrt(var_total)
    coords = covariates.coords
    dims = tuple(coords)
    target = engine.dm.y_t(mu_h)
    attrs = dict(getattr(target, "attrs", {}) or {})
    flat = lambda a: np.asarray(a.values if hasattr(a, "values") else a).reshape(-1)  # noqa: E731
    inv = engine.dm.error_pipeline.inverse_transform
    data = {
        "mean": (dims, flat(target), attrs),
        "se_plugin": (dims, flat(inv(var_plugin)), attrs),
        "se_hyper": (dims, flat(inv(var_hyper.astype(var_plugin.dtype))), attrs),
        "se": (dims, flat(inv(var_total.astype(var_plugin.dtype))), attrs),
        "lower": (dims, flat(engine.dm.y_t((mu_h - q * sd).astype(mu_h.dtype))), dict(attrs, ci=ci)),
        "upper": (dims, flat(engine.dm.y_t((mu_h + q * sd).astype(mu_h.dtype))), dict(attrs, ci=ci)),
        "inflation": (dims, var_total / var_plugin),
        "var_plugin": (dims, var_plugin.astype(np.float64)),
        "var_hyper": (dims, var_hyper),
    }
    out_attrs = {"ci": ci, "prior": bool(prior), "n_eff": int(active.sum()) - unident.shape[0], "n_unidentified": int(unident.shape[0]),
                 "order": "first (delta method)"}
    return Dataset(data, coords=dict(coords), attrs=out_attrs)


def period_hyper_covariance(engine, x, a, groups, P, mode, s, prior=True, pred_noise=False):
    """cov_hyper (P, P) = G Sigma_raw G^T of the period sums of ``loads.point_moments``: the period Jacobian is
    mode 1 (log target)       G[g][k] = sum_{i in g} a_i (s J_mu[i][k] + 1/2 s^2 J_var[i][k]),  a_i = w_i exp(s mu_i + t + s^2 var_i / 2),
    mode 0 (standardised)     G[g][k] = s sum_{i in g} w_i J_mu[i][k],                           a_i = w_i,
    an O(m R) contraction on the host -- no m x m buffer, so the dense and the streamed path share it.  ``a`` (m,): the
    per-point factors above; ``groups`` (m,) period ids (-1: excluded).  First order in Sigma_raw.  -> (cov_hyper, G)."""
    x = x.to(engine.device, engine.dtype).contiguous()
    engine._eval_ready(x)
    host = host_jacobians(engine)
    J_mu, J_var = prediction_jacobians(engine, x, pred_noise=pred_noise, return_var=mode == MODE_LOG, host=host)  # mode 0: means only
    _params, cov_raw, _active, _unident = raw_covariance(engine, prior=prior, x=x, host=host)
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    rows = a[:, None] * (s * J_mu + (0.5 * s * s * J_var if mode == MODE_LOG else 0.0))
    groups = np.asarray(groups).reshape(-1)
    G = np.zeros((P, rows.shape[1]))
    keep = groups >= 0
    np.add.at(G, groups[keep], rows[keep])
    return G @ cov_raw @ G.T, G
