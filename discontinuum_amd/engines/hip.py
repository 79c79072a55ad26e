"""``MarginalHIP`` -- the MI355X-native exact-GP engine behind discontinuum's engine surface.

Drop-in for ``MarginalGPyTorch`` (``src/discontinuum/engines/gpytorch.py:36-626``): same
``fit / predict / predict_grid / sample / save / load / build_model`` signatures, attributes and error
behaviour, same optimisation loop (Adam/AdamW, ReduceLROnPlateau, clip-norm 1.0, NaN policy, early
stopping, resume).  What changes is underneath ``mll(self.model(train_x), train_y)`` and
``likelihood(model(x))``: the Gram build, Cholesky, solves and gradient contraction run as hand-written
HIP kernels on the GPU through the C ABI of ``libdgp_hip.so``.  There is no CPU path: construction of
the device plan raises if the GPU or the shared library is missing.

Differences from the reference, on purpose:
  * the factorisation is exact at every n (stock gpytorch switches to CG/Lanczos above n = 800,
    SURVEY.md Appendix A.7);
  * arithmetic dtype is ``self.dtype`` (float64 by default; the reference casts to float32 at
    ``engines/gpytorch.py:221-222``) -- set ``MarginalHIP.dtype = torch.float32`` to match it.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import tqdm

from .. import _lib
from ..backend import GPPlan
from ..gp.explicit import ExplicitObjective
from ..gp.lowering import lower
from ..gp.mll import ExactMarginalLogLikelihood, NotPSDError, objective_name, predictive_mean
from ..xr_compat import DataArray
from .base import BaseModel, ModelConfig, is_fitted


class _FlatState:
    """The optimiser state of all parameters in three flat buffers; ``state[p]['exp_avg' | 'exp_avg_sq' | 'step']``
    are views into them, so ``state_dict()`` still holds torch's per-parameter layout.  ``load_state_dict`` and
    torch's own ``step`` (the fallback) invalidate it: it is then rebuilt from whatever the state holds."""

    def __init__(self, params, state):
        self.sizes = [int(p.numel()) for p in params]
        self.shapes = [p.shape for p in params]
        self.exp_avg = torch.cat([state[p]["exp_avg"].detach().reshape(-1) for p in params])
        self.exp_avg_sq = torch.cat([state[p]["exp_avg_sq"].detach().reshape(-1) for p in params])
        self.steps = torch.stack([state[p]["step"].detach().reshape(()) for p in params])
        self.count = int(self.steps[0])  # equal for all parameters (checked by the caller)
        self.param_views = [p.detach().view(-1) for p in params]  # same storage as the parameters, flat shapes
        offset = 0
        for k, (p, n, shape) in enumerate(zip(params, self.sizes, self.shapes)):
            state[p]["exp_avg"] = self.exp_avg[offset:offset + n].view(shape)
            state[p]["exp_avg_sq"] = self.exp_avg_sq[offset:offset + n].view(shape)
            state[p]["step"] = self.steps[k]
            offset += n


def _flat_state(opt, params):
    """The optimiser's ``_FlatState``, (re)built if needed; None if the state is not one the fast path handles."""
    flat = opt.__dict__.get("_flat_state")
    if flat is not None:
        # the flat parameter views must still be the parameters' storage (someone may have reassigned ``p.data``)
        if (flat.param_views[0].data_ptr() == params[0].data_ptr()
                and flat.param_views[-1].data_ptr() == params[-1].data_ptr()):
            return flat
    state, first = opt.state, None
    for p in params:
        st = state.get(p)
        if not st or not torch.is_tensor(st.get("step")) or "exp_avg" not in st or "exp_avg_sq" not in st:
            return None  # before torch's first step has created the state
        if first is None:
            first = float(st["step"])
        elif float(st["step"]) != first:
            return None  # parameters that have taken different numbers of steps
    flat = opt.__dict__["_flat_state"] = _FlatState(params, state)
    return flat


def _lean_step(opt, decoupled, flat_grad=None):
    """One Adam / AdamW step with the arithmetic of ``torch.optim.adam._multi_tensor_adam`` (no amsgrad / maximize /
    capturable), element for element, on FLAT views of the state: a dozen scalar-sized host parameters cost torch's
    ``Optimizer.step`` about 200 us, three quarters of it bookkeeping and per-tensor dispatch; this is a dozen vector
    operations.  ``state_dict()`` / ``load_state_dict()`` and checkpoints keep torch's per-parameter layout
    (``_FlatState``), and parameters and state stay bit-identical to torch's (tests/test_engine_cpu.py).  Returns False
    if the fast path does not apply (first step, a parameter without gradient, several groups, unequal step counts):
    the caller then takes torch's own step."""
    if len(opt.param_groups) != 1:
        return False
    group = opt.param_groups[0]
    params = group["params"]
    if group.get("amsgrad") or group.get("maximize") or group.get("capturable") or group.get("differentiable"):
        return False
    if flat_grad is None:
        for p in params:
            if p.grad is None or p.grad.is_sparse:
                return False
    with torch.no_grad():
        flat = _flat_state(opt, params)
        if flat is None:
            return False
        beta1, beta2 = group["betas"]
        lr, wd, eps = float(group["lr"]), group["weight_decay"], group["eps"]
        if flat_grad is None:
            grad = torch.cat([p.grad.reshape(-1) for p in params])
        elif flat_grad.numel() != flat.exp_avg.numel():
            return False
        else:
            grad = flat_grad  # the caller's gradient of all parameters in group order (never modified here)
        flat.steps += 1
        flat.count += 1
        step = flat.count
        if wd != 0:
            if decoupled:
                torch._foreach_mul_(flat.param_views, 1 - lr * wd)
            else:
                grad = grad.add(torch.cat(flat.param_views), alpha=wd)
        flat.exp_avg.lerp_(grad, 1 - beta1)
        flat.exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        bias1, bias2 = 1 - beta1 ** step, 1 - beta2 ** step
        denom = flat.exp_avg_sq.sqrt().div_(bias2 ** 0.5).add_(eps)
        update = (flat.exp_avg * (-(lr / bias1))).div_(denom)  # addcdiv's  value * t1 / t2, in its order
        torch._foreach_add_(flat.param_views, list(update.split(flat.sizes)))
    return True


class _LeanMixin:
    """``step`` through ``_lean_step`` where it applies; anything that changes the state behind its back drops the
    flat view of it."""

    _decoupled = False

    def step(self, closure=None):
        if closure is None and _lean_step(self, self._decoupled):
            return None
        self.__dict__["_flat_state"] = None  # torch's own step may leave the parameters' step counts unequal
        return super().step(closure)

    def step_flat(self, flat_grad):
        """A step from the gradient of all parameters as ONE flat tensor (group order).  False if the flat state is
        not available (before torch's first step has created it): the caller then sets ``p.grad`` and calls ``step``."""
        return _lean_step(self, self._decoupled, flat_grad)

    def load_state_dict(self, state_dict):
        self.__dict__["_flat_state"] = None
        return super().load_state_dict(state_dict)

    def add_param_group(self, param_group):
        self.__dict__["_flat_state"] = None
        return super().add_param_group(param_group)


class _LeanAdam(_LeanMixin, torch.optim.Adam):
    _decoupled = False


class _LeanAdamW(_LeanMixin, torch.optim.AdamW):
    _decoupled = True


def _clip_grad_norm(params, max_norm):
    """``torch.nn.utils.clip_grad_norm_(params, max_norm)`` (2-norm, in place) for a few dozen scalar-sized host
    gradients: the same arithmetic -- scale by min(1, max_norm / (norm + 1e-6)) -- through one flat reduction instead
    of the foreach machinery (85 -> 30 us per iteration).  Returns the total norm as a float."""
    grads = [p.grad for p in params if p.grad is not None]
    if not grads:
        return 0.0
    flat = grads[0].reshape(-1) if len(grads) == 1 else torch.cat([g.reshape(-1) for g in grads])
    total = float(torch.linalg.vector_norm(flat))
    coef = max_norm / (total + 1e-6)
    if not coef >= 1.0:  # a NaN norm scales by NaN, an infinite one by 0, exactly like torch's clamped coefficient
        for g in grads:
            g.mul_(coef)
    return total


def _get_optimizer_name(optimizer_obj):
    if isinstance(optimizer_obj, torch.optim.AdamW):
        return "adamw"
    if isinstance(optimizer_obj, torch.optim.Adam):
        return "adam"
    return optimizer_obj.__class__.__name__


class MeanShortcut:
    """A prior mean / noise model with a handful of parameters that stay on the host.  ``residual_and_noise`` builds
    y - mu and the noise diagonal on the device WITHOUT autograd (scalars travel as kernel arguments, nothing is copied
    to the device); ``grads`` maps the reductions the fit step leaves in its result row (``DGP_OUT_SUM_DR``,
    ``DGP_OUT_DR_W0..``, ``DGP_OUT_SUM_DNOISE``) to d NLL / d param for ``params`` (host tensors with grad)."""

    params: tuple = ()

    def param_values(self):
        """Current values of ``params`` without side effects on the device (``params`` itself may be refreshed only
        by ``residual_and_noise``)."""
        return self.params

    def residual_and_noise(self, plan, target):
        raise NotImplementedError

    def grads(self, row):
        raise NotImplementedError


class ConstantMeanShortcut(MeanShortcut):
    """mu = c (``ConstantMean``), fixed noise: r = y - c, d NLL / d c = -sum_i d NLL / d r_i."""

    def __init__(self, constant, noise_dev):
        self.params, self.noise_dev = (constant,), noise_dev

    def residual_and_noise(self, plan, target):
        return target - float(self.params[0].detach()), self.noise_dev

    def grads(self, row):
        return (-row[_lib.OUT_SUM_DR],)


class CensorState:
    """The censoring of a fit: ``side`` (device int32, -1 = the target value is a limit and the truth lies below it, +1 =
    above, 0 = observed, 2 = the truth lies between the target value and ``upper``), ``upper`` (device, model space, read on
    the rows of side 2 only; None when there is no such row), the latest mode ``f`` of the Laplace approximation (device;
    None = cold start from the prior mean) and the ``status`` of the last mode search (Newton iterations, final max |df|,
    halvings, capped rows).  ``approximation`` = "ep": the fit runs expectation propagation instead; ``sites`` = (y~, n~) are then
    the warm start between training iterations (None = cold) and ``status`` the last call's (sweeps, final max |dmu|, final max
    v |dtau|, capped rows, rows held back, censored rows)."""

    def __init__(self, side, maxit=50, tol=1e-10, upper=None, approximation="laplace", ep_maxit=100, damping=1.0):
        self.side, self.f, self.status, self.maxit, self.tol = side, None, None, int(maxit), float(tol)
        self.upper = upper
        self.approximation, self.sites, self.ep_maxit, self.damping = approximation, None, int(ep_maxit), float(damping)

    def kwargs(self):
        """The keyword arguments of ``GPPlan.laplace_*`` that the bracketed rows add (none without such a row: the
        entry points of the one-sided fit, bit for bit)."""
        return {} if self.upper is None else {"upper": self.upper}

    def update(self, f, status):
        self.f, self.status = f.detach(), tuple(status)

    def update_sites(self, sites, status):
        self.sites, self.status = tuple(t.detach() for t in sites), tuple(status)


def censor_sides(censored, n, bracketed=False):
    """``fit(censored=...)`` as an int32 array of -1 / 0 / +1, or None when nothing is censored.  Booleans: True = the
    reported value is a detection limit and the truth is below it.  ``bracketed`` (the caller has a ``target_upper``): the
    code 2 -- the truth lies between the target value and the upper end -- is accepted too."""
    if censored is None:
        return None
    a = np.asarray(getattr(censored, "values", censored))
    if a.shape != (n,):
        raise ValueError(f"censored must align with the target: expected shape ({n},), got {a.shape}")
    if a.dtype == bool:
        side = np.where(a, -1, 0).astype(np.int32)
    else:
        if bracketed:
            if not np.all(np.isin(a, (-1, 0, 1, 2))):
                raise ValueError("censored must be boolean or hold -1 (below the limit), 0 (observed), +1 (above the limit), "
                                 "2 (between the target value and target_upper)")
        elif not np.all(np.isin(a, (-1, 0, 1))):
            raise ValueError("censored must be boolean or hold -1 (below the limit), 0 (observed), +1 (above the limit); the code "
                             "2 (between the target value and an upper end) needs target_upper")
        side = a.astype(np.int32)
    return side if side.any() else None


def _approximation_name(approximation):
    """``fit(approximation=...)`` as "laplace" or "ep" (None: "laplace")."""
    name = "laplace" if approximation is None else approximation
    if name not in ("laplace", "ep"):
        raise ValueError(f'approximation must be "laplace" or "ep", got {approximation!r}')
    return name


MIDPOINT_WIDTH = 1e-6  # a bracket narrower than this many sigma is an observation at its midpoint


class _Values:
    """The least a target pipeline's first step reads of a labelled array."""

    def __init__(self, values):
        self.values = values


def bracket_ends(side, y, upper_model, sigma):
    """The model-space ends of the bracketed rows (``side`` == 2) from the transformed lower ends ``y`` and upper ends
    ``upper_model``: a decreasing target transform has swapped them, so the ends are sorted; a bracket narrower than
    ``MIDPOINT_WIDTH`` sigma becomes an observation (side 0) at its midpoint.  -> (side, y, upper) as new numpy arrays; upper
    is NaN off the bracketed rows, or None when no bracketed row is left."""
    side = np.array(side, dtype=np.int32)
    y = np.array(y, dtype=np.float64)
    br = side == 2
    lo = np.where(br, np.minimum(y, upper_model), y)
    hi = np.where(br, np.maximum(y, upper_model), np.nan)
    if not np.all(np.isfinite(lo[br]) & np.isfinite(hi[br])):
        raise ValueError("target_upper (and the target) must be finite in model space on every row with censored == 2")
    narrow = br & ~(hi - lo >= MIDPOINT_WIDTH * sigma)
    y = np.where(narrow, 0.5 * (lo + hi), lo)
    side[narrow] = 0
    hi = np.where(narrow, np.nan, hi)
    return side, y, (hi if (side == 2).any() else None)


class PriorSpec:
    """What ``self.model(train_x)`` hands to the marginal likelihood: the device plan, the constrained kernel
    hyperparameters (host, with grad), the prior mean and the noise diagonal (device, with grad; evaluated when
    read), -- for mean / noise models that have one -- the host-side ``shortcut`` the marginal likelihood uses
    instead of them, and the ``CensorState`` of a fit with censored observations."""

    def __init__(self, plan, theta, mean, noise, shortcut=None, censored=None, objective="mll"):
        self.plan, self.theta, self._mean, self._noise, self.shortcut = plan, theta, mean, noise, shortcut
        self.censored = censored
        self.objective = objective  # "mll" or "loo": which data term the marginal-likelihood object evaluates
        self.upper = getattr(censored, "upper", None)  # the upper ends of the bracketed rows (model space) or None

    @property
    def mean(self):
        if callable(self._mean):
            self._mean = self._mean()
        return self._mean

    @property
    def noise(self):
        if callable(self._noise):
            self._noise = self._noise()
        return self._noise


class MarginalHIP(BaseModel):
    dtype = torch.float64
    device = "cuda"
    explicit_host_algebra = True  # closed-form host algebra per iteration where the model allows it (gp/explicit.py)
    _plan_factory = staticmethod(GPPlan)  # tests substitute an oracle-backed double; the product never does

    def __init__(self, model_config: dict | None = None):
        super().__init__(model_config=model_config)
        self._resume_info = None
        self._last_optimizer = None
        self._last_scheduler = None
        self._current_iteration = 0
        self._plan = None
        self._factor_key = None
        self._pending_device = None  # (train_x, train_y) whose upload is deferred to the first prediction (fit_many)
        self._censor = None  # CensorState of a fit with censored observations
        self._y_model = None
        self.laplace_status_ = None
        self.ep_status_ = None
        self._approximation = "laplace"
        self.objective_ = "mll"  # the training objective of the last fit: "mll", "loo" or "lgo"
        self.objective_folds_ = None  # "lgo": the fold id of every training observation (-1 = never held out)

    # ------------------------------------------------------------------ device plumbing
    def _tensor(self, a):
        return torch.as_tensor(np.asarray(a), dtype=self.dtype).to(self.device).contiguous()

    def _setup_device(self, train_x, train_y):
        """Lower the kernel tree, (re)create the device plan and upload the training inputs."""
        n, d = train_x.shape
        model_name, self._theta_fn = lower(self.model.covar_module, d)
        key = (model_name, n, d, self.dtype, str(self.device))
        if self._plan is None or self._plan_key != key:
            self._plan = self._plan_factory(model_name, n, d, dtype=self.dtype, device=self.device)
            self._plan_key = key
        self._train_x = train_x.to(self.device, self.dtype).contiguous()
        self._train_y = train_y.to(self.device, self.dtype).contiguous()
        self._plan.set_inputs(self._train_x)
        if getattr(self, "objective_", "mll") == "lgo":
            self._plan.set_folds(torch.as_tensor(np.asarray(self.objective_folds_, dtype=np.int64)))
        self._factor_key = None
        self._pending_device = None

    def _prior(self):
        """``self.model(train_x)`` of the reference loop (engines/gpytorch.py:350)."""
        return PriorSpec(
            plan=self._plan,
            theta=self._theta_fn(),
            mean=lambda: self.model.prior_mean(self._train_x),
            noise=lambda: self.likelihood.train_noise(self._train_x.device, self.dtype),
            shortcut=self._mean_shortcut(),
            censored=getattr(self, "_censor", None),
            objective=getattr(self, "objective_", "mll"),
        )

    def model_space_targets(self):
        """The model-space targets the fit ran on (numpy): ``dm.y``, with the entries of bracketed rows as ``fit`` placed them
        (the lower end in model space, or the midpoint of a very narrow bracket)."""
        own = getattr(self, "_y_model", None)
        return self.dm.y if own is None else own

    _CENSOR_REFUSAL = ("{what} is not available for a fit with censored observations: it reads the pseudo-data of the Laplace "
                       "approximation as if they were samples")

    def _refuse_censored(self, what, hint=""):
        if getattr(self, "_censor", None) is not None:
            text = self._CENSOR_REFUSAL.format(what=what)
            if self._censor.approximation == "ep":
                text = text.replace("the Laplace approximation", "expectation propagation")
            raise NotImplementedError(text + hint)

    def _set_censoring(self, censored, n, target_upper=None, y=None, approximation=None):
        """Parse ``censored`` and ``target_upper`` (see ``fit``) and keep them on the engine; the side vector (and the upper
        ends) go to the device with the data.  ``y``: the model-space targets (needed with ``target_upper``).  -> the
        model-space targets the fit runs on: ``y`` itself unless a bracketed row changed its entry (a decreasing transform
        swaps a bracket's ends; a very narrow bracket becomes an observation at its midpoint).  ``approximation``: "laplace" or
        "ep" (None: what the engine holds, "laplace" unless a fit or a checkpoint said otherwise)."""
        if approximation is not None:
            self._approximation = _approximation_name(approximation)
        side = censor_sides(censored, n, bracketed=target_upper is not None)
        self._censor_host = side  # as given: what a checkpoint carries
        self._upper_host = None   # data space, as given
        self._y_model = None      # the model-space targets of a fit with bracketed rows (numpy), where they differ from dm.y
        self._censor = None
        self.laplace_status_ = None
        self.ep_status_ = None
        if side is None:
            return y
        if getattr(self.likelihood, "second_noise_covar", None) is not None:
            raise NotImplementedError("censored observations need a fixed-noise likelihood: the Laplace fit produces no gradient "
                                      "for a learned noise term (rating-gp is not supported)")
        upper = None
        if (side == 2).any():
            raw = np.asarray(getattr(target_upper, "values", target_upper), dtype=np.float64)
            if raw.shape != (n,):
                raise ValueError(f"target_upper must align with the target: expected shape ({n},), got {raw.shape}")
            if y is None:
                raise ValueError("bracketed rows need the model-space targets")
            self._upper_host = raw
            br = side == 2
            # through the target pipeline as it was fitted on the target (never refitted); rows without a bracket are not read
            filled = np.where(br, raw, raw[br][0])
            upper_model = np.asarray(self.dm.target_pipeline.transform(_Values(filled)), dtype=np.float64).reshape(-1)
            noise = self.likelihood.train_noise(torch.device("cpu"), torch.float64)
            sigma = np.broadcast_to(np.sqrt(np.asarray(noise.detach().cpu().numpy(), dtype=np.float64)).reshape(-1), (n,))
            side, y_model, upper = bracket_ends(side, y.detach().cpu().numpy(), upper_model, sigma)
            self._y_model = y_model
            y = torch.as_tensor(y_model, dtype=y.dtype)
            if not side.any():
                return y
        self._censor = CensorState(torch.as_tensor(side, dtype=torch.int32).to(self.device).contiguous(),
                                   maxit=self.laplace_maxit, tol=self.laplace_tol,
                                   upper=None if upper is None else self._tensor(upper),
                                   approximation=getattr(self, "_approximation", "laplace"), ep_maxit=self.ep_maxit,
                                   damping=self.ep_damping)
        return y

    laplace_maxit, laplace_tol = 50, 1e-10  # Newton's mode search of a censored fit
    ep_maxit, ep_damping = 100, 1.0         # the sweeps of a censored fit by expectation propagation (tolerance: laplace_tol)

    def _record_censor_status(self):
        if self._censor is not None:
            if self._censor.approximation == "ep":
                self.ep_status_ = self._censor.status
            else:
                self.laplace_status_ = self._censor.status

    def _mean_shortcut(self):
        """The host-side form of this model's prior mean and noise (``MeanShortcut``) or None.  Here: a learned
        constant mean with fixed noise (loadest-gp); model packages override it for their own parametric means."""
        from ..gp.means import ConstantMean
        from ..gp.models import ExactGP

        module = getattr(self.model, "mean_module", None)
        if (type(module) is ConstantMean and type(self.model).prior_mean is ExactGP.prior_mean
                and getattr(self.likelihood, "second_noise_covar", None) is None):
            return ConstantMeanShortcut(module.constant, self.likelihood.train_noise(self._train_x.device, self.dtype))
        return None

    def _differentiable_mean(self, x: torch.Tensor):
        """Posterior mean at model-space points ``x`` WITH gradients to every hyperparameter
        (``likelihood(model(x)).mean`` inside the reference's penalty callback,
        src/rating_gp/models/gpytorch.py:160-176).  Valid inside a training iteration, after the marginal
        likelihood of that iteration has been evaluated (the plan holds its factorisation)."""
        x = x.to(self.device, self.dtype).contiguous()
        if hasattr(self.model, "prepare_eval"):
            self.model.prepare_eval(self._train_x, x)
        spec = self._prior()
        r = (self._train_y - spec.mean).contiguous()
        return predictive_mean(self._plan, spec.theta, r, spec.noise.contiguous(), x) + self.model.prior_mean(x)

    def _param_key(self):
        return tuple(float(v) for p in self.model.parameters() for v in p.detach().reshape(-1).tolist())

    # ------------------------------------------------------------------ data -> host model -> device
    def _attach(self, covariates, target, target_unc, refit_data=True):
        """Fit the data manager (unless the caller keeps the current one) and return the model-space training tensors
        (x, y, y_unc or None) in ``self.dtype``."""
        if refit_data:
            self.dm.fit(target=target, covariates=covariates, target_unc=target_unc)
        self.X, self.y = self.dm.X, self.dm.y
        x = torch.tensor(self.X, dtype=self.dtype)
        y = torch.tensor(self.y, dtype=self.dtype)
        unc = None
        if target_unc is not None:
            self.y_unc = self.dm.y_unc
            unc = torch.tensor(self.y_unc, dtype=self.dtype)
        return x, y, unc

    def _fresh_model(self, x, y, unc):
        """``build_model`` with the reference's calling convention: the uncertainty is only passed when there is one.
        (The hook also sets ``self.likelihood``.)"""
        self.model = self.build_model(x, y) if unc is None else self.build_model(x, y, unc)

    # ------------------------------------------------------------------ checkpointing
    # Dictionary layout of the reference's checkpoints (engines/gpytorch.py:107-160): state dicts of model / likelihood /
    # optimiser / scheduler plus bookkeeping, the parameters under gpytorch's raw_* names.  Cross-engine loading is NOT
    # claimed: a reference-written file pickles its own ModelConfig class (not importable here, and never unpickled --
    # load() reads with weights_only=True), and the buffer keys of priors / constraints are unpinned (see _load_state).
    _OPTIMIZER_KEYS = ("optimizer_state_dict", "optimizer_name", "optimizer_lr", "scheduler_state_dict", "scheduler_name")

    def save(self, f, optimizer_obj=None, scheduler=None, extra=None) -> None:
        for attr in ("model", "likelihood"):
            if not hasattr(self, attr):
                raise RuntimeError(f"No {attr} to save. Call fit() first.")
        opt = optimizer_obj if optimizer_obj is not None else getattr(self, "_last_optimizer", None)
        sch = scheduler if scheduler is not None else getattr(self, "_last_scheduler", None)
        record = {
            "model_class": f"{type(self).__module__}.{type(self).__name__}",
            "model_config": self._config_record(),
            "current_iteration": getattr(self, "_current_iteration", 0),
            "extra": extra or {},
            "model_state_dict": self.model.state_dict(),
            "likelihood_state_dict": self.likelihood.state_dict(),
            "censored": None if getattr(self, "_censor_host", None) is None else torch.as_tensor(self._censor_host, dtype=torch.int8),
            "target_upper": (None if getattr(self, "_upper_host", None) is None
                             else torch.as_tensor(self._upper_host, dtype=torch.float64)),
            "approximation": getattr(self, "_approximation", "laplace"),
            **({} if getattr(self, "objective_", "mll") == "mll" else {"objective": self.objective_}),
            **({} if getattr(self, "objective_", "mll") != "lgo" else
               {"objective_folds": torch.as_tensor(np.asarray(self.objective_folds_, dtype=np.int64))}),
            "optimizer_state_dict": None, "optimizer_name": None, "optimizer_lr": None,
            "scheduler_state_dict": None, "scheduler_name": None,
        }
        if opt is not None:
            groups = getattr(opt, "param_groups", None) or [{}]
            record.update(optimizer_state_dict=opt.state_dict(), optimizer_name=_get_optimizer_name(opt),
                          optimizer_lr=groups[0].get("lr"))
        if sch is not None:
            record.update(scheduler_state_dict=sch.state_dict(), scheduler_name=type(sch).__name__)
        torch.save(record, f)

    def _config_record(self):
        """The model configuration as plain data (a checkpoint must load with ``weights_only=True``)."""
        config = getattr(self, "model_config", None)
        if isinstance(config, ModelConfig):
            return {"transform": config.transform}
        return config if isinstance(config, dict) else None

    @staticmethod
    def _load_state(module, state, what):
        """``load_state_dict`` that insists on every PARAMETER (raw_*, the power law's a / b / c) and tolerates
        differences in the buffers that only describe priors and constraints (``*_prior.scale``, ``*_constraint.
        lower_bound`` ...): those are constants of the model definition, rebuilt by ``build_model``, and whether a prior
        registers them as buffers differs between gpytorch versions -- the gpytorch side of this boundary is parity
        unpinned."""
        result = module.load_state_dict(state, strict=False)
        params = {name for name, _ in module.named_parameters()}
        missing = [k for k in result.missing_keys if k in params]
        unexpected = [k for k in result.unexpected_keys
                      if k.rsplit(".", 1)[-1].startswith("raw_") or "powerlaw" in k or "mean_module" in k]
        if missing or unexpected:
            raise RuntimeError(f"{what} state does not match this model: missing parameters {missing}, "
                               f"unexpected parameters {unexpected}")

    @classmethod
    def load(cls, f, covariates, target, target_unc=None, censored=None, target_upper=None, approximation=None):
        """A model restored from ``save()`` output and re-attached to its data: ready to predict, or to continue
        training with ``fit(..., resume=True)`` (engines/gpytorch.py:47-105).  ``censored`` / ``target_upper``: as in
        ``fit``; None takes what the checkpoint carries (the codes and the brackets' upper ends).  ``approximation``: None takes
        the checkpoint's ("laplace" for a checkpoint written before expectation propagation existed).  The file is read with
        ``weights_only=True`` (nothing in it is executed); checkpoints of earlier versions that pickled the
        ``ModelConfig`` dataclass load under an allow-list of exactly that class."""
        with torch.serialization.safe_globals([ModelConfig]):
            record = torch.load(f, map_location="cpu", weights_only=True)
        # the reference rebuilds with the default configuration and ignores the one it saved (engines/gpytorch.py:69);
        # a model trained with transform="standard" would come back in the wrong data space, so the saved one is used
        saved_config = record.get("model_config")
        if isinstance(saved_config, dict) and "transform" in saved_config:
            saved_config = ModelConfig(transform=saved_config["transform"])
        self = cls(model_config=saved_config) if isinstance(saved_config, ModelConfig) else cls()
        x, y, unc = self._attach(covariates, target, target_unc)
        self._fresh_model(x, y, unc)
        self._load_state(self.model, record["model_state_dict"], "model")
        if record.get("likelihood_state_dict") is not None:
            self._load_state(self.likelihood, record["likelihood_state_dict"], "likelihood")
        self._current_iteration = record.get("current_iteration", 0)
        self._resume_info = {key: record.get(key) for key in cls._OPTIMIZER_KEYS}
        self._resume_info["current_iteration"] = self._current_iteration
        if censored is None and record.get("censored") is not None:
            censored = record["censored"].numpy().astype(np.int32)  # the side vector the checkpoint carries
            if target_upper is None and record.get("target_upper") is not None:
                target_upper = record["target_upper"].numpy()  # and the brackets' upper ends (data space)
        if approximation is None:
            approximation = record.get("approximation") or "laplace"
        self.objective_ = objective_name(record.get("objective"))  # a checkpoint without the key was trained on "mll"
        if self.objective_ == "lgo":
            self.objective_folds_ = record["objective_folds"].numpy().astype(np.int64)
        y = self._set_censoring(censored, y.shape[0], target_upper, y, approximation)
        self._setup_device(x, y)
        self.is_fitted = True
        return self

    # ------------------------------------------------------------------ fit
    @staticmethod
    def _new_optimizer(params, name, lr):
        """The reference's two optimisers with its hyperparameters (engines/gpytorch.py:268-288)."""
        decay = {"adam": (_LeanAdam, 1e-4), "adamw": (_LeanAdamW, 1e-2)}
        if name not in decay:
            raise ValueError(f"Unsupported optimizer: {name!r}. Supported optimizers are 'adam' and 'adamw'.")
        cls, weight_decay = decay[name]
        # foreach: the same update rule as one multi-tensor call per step
        return cls(params, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay, foreach=True)

    @staticmethod
    def _restore(obj, state):
        """Best-effort ``load_state_dict`` (a checkpoint from another optimiser layout must not stop a fit)."""
        if obj is not None and state is not None:
            try:
                obj.load_state_dict(state)
            except Exception:  # noqa: BLE001, S110
                pass

    def fit(self, covariates, target, target_unc=None, iterations: int = 100, optimizer: str | None = None,
            learning_rate: float | None = None, early_stopping: bool = False, patience: int = 60,
            scheduler: bool = True, resume: bool = False, penalty_callback=None, penalty_weight: float = 0.0, censored=None,
            target_upper=None, approximation="laplace", objective="mll", folds=None):
        """Train the hyperparameters; arguments and behaviour as ``MarginalGPyTorch.fit``
        (engines/gpytorch.py:162-458): Adam (default lr 0.05) or AdamW, gradient clipping to norm 1, optional
        ReduceLROnPlateau, NaN iterations skipped (more than ten in a row raise), optional early stopping, resume from a
        checkpoint (``load``) or from an interrupted call (``resume=True``), optional penalty term.

        ``censored``: array-like aligned with ``target``, boolean (True = the reported value is a detection limit and the
        truth is below it) or -1 / 0 / +1 (below / observed / above the reported limit).  The limits pass through the target
        pipeline like any value (it is monotone); the marginal likelihood becomes the Laplace approximation of the Tobit
        likelihood (``dgp_laplace_fit_step``) and every product that reads the held factorisation sees the Laplace
        posterior.  None or no censored row: the plain fit, bit for bit.  ``laplace_status_`` keeps the last mode search's
        (Newton iterations, final max |df|, halvings, capped rows).

        ``target_upper``: array-like aligned with ``target`` (data space), the upper ends of INTERVAL-censored rows.  A row
        with the code 2 in ``censored`` says that the truth lies between its ``target`` value and its ``target_upper`` value
        (EGRET's ConcLow / ConcHigh; ``loadest_gp.censoring_from_bounds`` builds the three arguments from such a pair); the
        code 2 is accepted only together with ``target_upper``, which is read on those rows alone.  The upper ends pass
        through the target pipeline AS FITTED ON ``target`` (it is never refitted on them); a decreasing pipeline swaps a
        bracket's ends, which are then sorted in model space.  A bracket narrower than 1e-6 sigma (the row's noise standard
        deviation in model space) is taken as an observation at its midpoint: the likelihood of so narrow a bracket is the
        Gaussian density there times the width, so this shifts the reported NLL by the constant -sum log(width_i) over
        those rows and leaves the mode and every gradient unchanged to O(width^2 / sigma^2).

        ``approximation``: "laplace" (the default; None means the same) or "ep".  With "ep" the censored rows are fitted by
        EXPECTATION PROPAGATION (``dgp_ep_fit_step``): Gaussian sites matched to the moments of the tilted distributions instead of
        a Gaussian at the posterior's mode -- the better approximation when most rows are censored far below their limits and
        the posterior is one-sided.  The sites are warm-started between training iterations; ``ep_status_`` keeps the last call's
        (sweeps, final max |dmu|, final max v |dtau|, capped rows, rows held back, censored rows).  Every product that reads the
        held factorisation then sees the EP posterior.  Without a censored row "ep" is the plain fit.  The keyword of THIS call
        decides: a resumed fit (or one that continues a loaded checkpoint) states it again.

        ``objective``: "mll" (the default; None means the same) minimises (NLL - log prior) / n, the marginal likelihood.
        "loo" minimises (L_LOO - log prior) / n with L_LOO = -sum_i log p(y_i | y_-i, theta), the exact leave-one-out predictive
        likelihood (``dgp_loo_fit_step``; minus the ``elpd`` that ``cross_validate("loo")`` reports) -- the more robust choice
        when the noise is fixed rather than learned to fit.  Priors, constraints, clamps, the jitter retries, the optimiser, the
        scheduler, early stopping and the penalty are the same; ``objective_`` records the choice.  Together with ``censored``
        it is refused: the pseudo-data of a censored fit are not samples, and leaving one out predicts nothing observed.
        "lgo" minimises (L_LGO - log prior) / n with L_LGO = -sum_g log p(y_g | y_-g, theta) over the folds of ``folds``, the
        exact leave-group-out predictive likelihood (``dgp_lgo_fit_step``; minus the ``elpd`` that ``cross_validate(folds)``
        reports): the criterion for records sampled in clusters, whose neighbours a few hours away make leave-one-out
        optimistic.  Folds of one give "loo", one fold of every row gives "mll".  Refused with ``censored`` like "loo".

        ``folds``: with ``objective="lgo"`` only, and required there: any scheme ``validation.cv_folds`` accepts -- a resample
        alias ("YE", "YE-SEP", "QE", "ME"), an int k, ``("random", k, seed)``, "loo" or explicit fold ids (-1 = never held
        out) -- evaluated on the training times as ``cross_validate`` does.  ``objective_folds_`` keeps the fold ids; a resumed
        fit states the keyword again."""
        approximation = _approximation_name(approximation)
        objective = objective_name(objective)
        if objective == "lgo" and folds is None:
            raise ValueError('objective="lgo" needs folds=<scheme>: what is held out together (see validation.cv_folds)')
        if objective != "lgo" and folds is not None:
            raise ValueError(f'folds belongs to objective="lgo", not to objective={objective!r}')
        if objective in ("loo", "lgo") and censored is not None and np.asarray(getattr(censored, "values", censored)).any():
            raise NotImplementedError(f'objective="{objective}" is not available together with censored observations: the pseudo-data of '
                                      "a censored fit are not samples, so their leave-one-out predictive likelihood is not the "
                                      "likelihood of anything observed (the reason influence() refuses them)")
        trained = bool(getattr(self, "model", None) is not None and getattr(self, "likelihood", None) is not None
                       and self.is_fitted)
        from_checkpoint = trained and self._resume_info is not None
        from_interruption = trained and resume and not from_checkpoint
        x, y, unc = self._attach(covariates, target, target_unc, refit_data=not from_interruption)
        restore = from_checkpoint or from_interruption
        if from_checkpoint:
            try:
                self.model.set_train_data(inputs=x, targets=y, strict=False)
            except Exception:  # noqa: BLE001
                restore = False
        if not restore:
            self._fresh_model(x, y, unc)
        if censored is not None or not restore:
            y = self._set_censoring(censored, y.shape[0], target_upper, y, approximation)
        elif getattr(self, "_upper_host", None) is not None:  # a resumed fit keeps its brackets
            y = self._set_censoring(self._censor_host, y.shape[0], self._upper_host, y, approximation)
        elif self._censor is not None and self._censor.approximation != approximation:
            y = self._set_censoring(self._censor_host, y.shape[0], None, y, approximation)
        if objective in ("loo", "lgo") and self._censor is not None:  # (the censoring a resumed fit or a checkpoint carries)
            raise NotImplementedError(f'objective="{objective}" is not available together with censored observations: the pseudo-data of '
                                      "a censored fit are not samples")
        self.objective_ = objective
        self.objective_folds_ = None
        if objective == "lgo":
            from ..validation import cv_folds

            self.objective_folds_ = cv_folds(np.asarray(self.dm.data.target.coords["time"].values), folds)[0]
        self._setup_device(x, y)
        if self._censor is not None:
            self._censor.f = None
            self._censor.sites = None
        self.model.train()
        self.likelihood.train()

        # what a previous run left behind: a checkpoint's record, or the live optimiser of an interrupted call
        previous = dict(self._resume_info or {})
        if from_interruption and self._last_optimizer is not None:
            groups = self._last_optimizer.param_groups
            previous = {"optimizer_name": _get_optimizer_name(self._last_optimizer),
                        "optimizer_lr": groups[0]["lr"] if groups else None,
                        "optimizer_state_dict": self._last_optimizer.state_dict(),
                        "scheduler_state_dict": self._last_scheduler.state_dict() if self._last_scheduler else None}
        # a saved optimiser kind outranks the argument, as in the reference (engines/gpytorch.py:268-288)
        saved = (previous.get("optimizer_name") or "").lower()
        asked = optimizer if optimizer is not None else (saved or "adam")
        name = next((kind for kind in ("adamw", "adam") if kind in (asked, saved)), asked)
        lr = learning_rate if learning_rate is not None else (previous.get("optimizer_lr") or 0.05)
        params = list(self.model.parameters())
        optimizer_obj = self._new_optimizer(params, name, lr)
        scheduler_obj = None
        if scheduler:
            scheduler_obj = torch.optim.lr_scheduler.ReduceLROnPlateau(
                optimizer_obj, mode="min", factor=0.7, patience=max(20, patience // 2), threshold=1e-4,
                threshold_mode="rel", min_lr=1e-6, cooldown=10)
        if restore:
            self._restore(optimizer_obj, previous.get("optimizer_state_dict"))
            self._restore(scheduler_obj, previous.get("scheduler_state_dict"))

        first = self._current_iteration if (resume and hasattr(self, "_current_iteration")) else 0
        if iterations <= first:
            print(f"Model already trained for {first} iterations (>= target {iterations}). No further training needed.")
            return
        mll = ExactMarginalLogLikelihood(self.likelihood, self.model)
        bar = tqdm.tqdm(range(iterations - first), ncols=100, desc=f"Training {first}->{iterations}")
        best, stale, bad_in_a_row, i = float("inf"), 0, 0, 0
        use_penalty = penalty_callback is not None and penalty_weight > 0.0
        # the iteration's host algebra in closed form where the model allows it (gp/explicit.py); a penalty joins that
        # path if it brings its own closed form (``explicit_terms``: rating-gp's monotonicity penalty does), any other
        # penalty callback is an autograd expression and keeps the autograd path
        closed_penalty = use_penalty and hasattr(penalty_callback, "explicit_terms")
        explicit = (ExplicitObjective.build(self, mll._priors)
                    if self.explicit_host_algebra and (not use_penalty or closed_penalty) and self._censor is None else None)
        try:
            for i in bar:
                self._current_iteration = first + i
                optimizer_obj.zero_grad(set_to_none=True)
                try:
                    if explicit is not None:
                        objective = torch.tensor([explicit.evaluate(
                            set_grads=False, penalty=penalty_callback if use_penalty else None,
                            penalty_weight=float(penalty_weight) if use_penalty else 0.0)], dtype=torch.float64)
                    else:
                        objective = -mll(self._prior(), self._train_y)
                        self._record_censor_status()
                except Exception:
                    bad_in_a_row += 1
                    if bad_in_a_row > 10:
                        raise
                    continue
                penalty = None
                if use_penalty and explicit is not None:
                    penalty = None if explicit.last_penalty is None else torch.tensor(explicit.last_penalty, dtype=torch.float64)
                elif use_penalty:
                    try:
                        value = penalty_callback()
                        penalty = value if torch.is_tensor(value) else None
                    except Exception:  # noqa: BLE001
                        penalty = None
                    if penalty is not None:
                        objective = objective + float(penalty_weight) * penalty.to(objective.device, objective.dtype)
                if not bool(torch.isfinite(objective).all()):
                    bad_in_a_row += 1
                    if bad_in_a_row > 10:
                        raise RuntimeError(
                            f"Encountered more than 10 consecutive NaN/Inf objectives at iteration {i + 1}")
                    continue
                bad_in_a_row = 0
                stepped = False
                if explicit is None:
                    objective.backward()
                    total_norm = _clip_grad_norm(params, 1.0)
                else:  # the gradient of all parameters is one flat array: clip it and step from it directly
                    total_norm = explicit.clip_flat_grad(1.0)
                    if math.isfinite(total_norm) and hasattr(optimizer_obj, "step_flat"):
                        stepped = optimizer_obj.step_flat(torch.from_numpy(explicit.flat_grad))
                    if not stepped:
                        explicit.assign_param_grads()
                # the reference scans every p.grad for NaN after clipping (engines/gpytorch.py:387-392); a clipped
                # gradient holds a NaN exactly when the pre-clip norm is NaN or Inf (Inf * 0 = NaN), so one scalar says it
                grads_broken = not math.isfinite(float(total_norm))
                if grads_broken:
                    for p in params:
                        if p.grad is not None:
                            p.grad = torch.nan_to_num(p.grad, nan=0.0, posinf=0.0, neginf=0.0)
                if not stepped:
                    optimizer_obj.step()
                value = float(objective.item())
                if scheduler_obj is not None:
                    scheduler_obj.step(value)
                if value < best - 1e-6:
                    best, stale = value, 0
                else:
                    stale += 1
                stop = early_stopping and stale >= patience
                if stop:
                    print(f"\nEarly stopping triggered after {i + 1} iterations")
                    print(f"Best objective: {best:.6f}")
                if not grads_broken:
                    note = f"obj={value:.4f}, lr={optimizer_obj.param_groups[0]['lr']:.1e}"
                    if penalty is not None and bool(torch.isfinite(penalty).all()):
                        note += f", pen={float(penalty.detach()):.3e}"
                    bar.set_postfix_str(note, refresh=False)  # shown at the bar's own refresh interval, not forced every iteration
                if stop:
                    break
        except KeyboardInterrupt:
            print(f"\nTraining interrupted at iteration {i + 1}")
            print(f"Best objective: {best:.6f}")
        finally:
            self.is_fitted = True
        self._last_optimizer, self._last_scheduler = optimizer_obj, scheduler_obj
        self._factor_key = None

    # ------------------------------------------------------------------ prediction
    def _device_ready(self):
        if getattr(self, "_pending_device", None) is not None:
            pending, self._pending_device = self._pending_device, None
            self._setup_device(*pending)

    def _ensure_factor(self):
        """Eval-mode cache of the reference's prediction strategy: (L, L^-1, alpha) at the current
        hyperparameters, rebuilt only when a parameter changed."""
        self._device_ready()
        key = self._param_key()
        if self._factor_key != key:
            with torch.no_grad():
                spec = self._prior()
                if spec.censored is not None and spec.censored.approximation == "ep":  # the EP posterior's pseudo-data system
                    cs = spec.censored
                    out, sites, stat = self._plan.ep_factorize(
                        spec.theta, self._train_y, spec.mean.contiguous(), spec.noise.contiguous(), cs.side, sites=cs.sites,
                        maxit=cs.ep_maxit, tol=cs.tol, damping=cs.damping, **cs.kwargs())
                    cs.update_sites(sites, stat)
                    self.ep_status_ = cs.status
                elif spec.censored is not None:  # the Laplace posterior's pseudo-data system, warm-started at the last mode
                    cs = spec.censored
                    out, f_hat, stat = self._plan.laplace_factorize(
                        spec.theta, self._train_y, spec.mean.contiguous(), spec.noise.contiguous(), cs.side, f=cs.f,
                        maxit=cs.maxit, tol=cs.tol, **cs.kwargs())
                    cs.update(f_hat, stat)
                    self.laplace_status_ = cs.status
                else:
                    r = (self._train_y - spec.mean).contiguous()
                    out = self._plan.factorize(spec.theta, r, spec.noise.contiguous())
                info = int(out[3].item())
            if info != 0:
                raise NotPSDError(f"Matrix not positive definite: Cholesky pivot {info} is not positive")
            self._factor_key = key
            self._factor_theta = spec.theta.detach()

    def _eval_ready(self, x=None):
        """What every product computed from the held factorisation starts with: the device state, eval mode, the model's
        data-dependent clamps for the model-space points ``x``, then the factorisation at the (clamped) hyperparameters --
        in this order: the parameter key ``_ensure_factor`` compares may depend on the clamps."""
        self._device_ready()
        self.model.eval()
        self.likelihood.eval()
        with torch.no_grad():
            if hasattr(self.model, "prepare_eval"):
                # data-dependent clamps see [X; X*]; without test points, the training rows only
                self.model.prepare_eval(self._train_x, self._train_x if x is None else x)
            self._ensure_factor()

    def _model_space_predict(self, x: torch.Tensor):
        """(mu, var) in model space -- ``__gpytorch_predict`` of the reference (engines/gpytorch.py:599-626)."""
        x = x.to(self.device, self.dtype).contiguous()
        self._eval_ready(x)
        with torch.no_grad():
            kmean, kvar = self._plan.predict(self._factor_theta, x)
            mu = kmean + self.model.prior_mean(x)
            var = kvar + self.likelihood.predictive_noise(x.shape[0], x.device, self.dtype)
        return mu, var

    @is_fitted
    def predict(self, covariates, diag=True, pred_noise=False):
        """Predictions in the original data space: (target, standard error) (engines/gpytorch.py:461-501).
        ``diag`` / ``pred_noise`` are accepted and ignored exactly like the reference does."""
        Xnew = torch.tensor(self.dm.Xnew(covariates), dtype=self.dtype)
        mu, var = self._model_space_predict(Xnew)
        target = self.dm.y_t(mu.cpu().numpy())
        target = target.assign_coords(covariates.coords)
        se = self.dm.error_pipeline.inverse_transform(var.cpu().numpy())
        se = se.assign_coords(covariates.coords)
        return target, se

    @is_fitted
    def predict_grid(self, covariate: str, coord: str | None = None, t_step: int = 12):
        """Posterior mean on a (coord x 18) grid (engines/gpytorch.py:503-549)."""
        if coord is None:
            coord = next(iter(self.dm.data.covariates.coords))
        coord_dim, covariate_dim = self.dm.get_dim(coord), self.dm.get_dim(covariate)
        x_max, x_min = self.dm.X.max(axis=0), self.dm.X.min(axis=0)
        n_cov = 18
        n_coord = int(np.round((x_max - x_min)[coord_dim] * t_step))
        x_coord = torch.linspace(float(x_min[coord_dim]), float(x_max[coord_dim]), n_coord, dtype=self.dtype)
        x_cov = torch.linspace(float(x_min[covariate_dim]), float(x_max[covariate_dim]), n_cov, dtype=self.dtype)
        mu, _var = self._model_space_predict(torch.cartesian_prod(x_coord, x_cov))
        target = self.dm.y_t(mu.cpu().numpy())
        index = self.dm.covariate_pipelines[coord].inverse_transform(x_coord.numpy())
        cov_vals = self.dm.covariate_pipelines[covariate].inverse_transform(x_cov.numpy())
        return DataArray(np.asarray(target.data).reshape(n_coord, n_cov), coords=[np.asarray(index), np.asarray(cov_vals)],
                         dims=[coord, covariate], attrs=target.attrs)

    @is_fitted
    def sample(self, covariates, n=1000):
        """Draws from the latent posterior (engines/gpytorch.py:551-593): full m x m covariance
        K** - V^T V with V = L^-1 K(X, X*), its Cholesky factor (our blocked HIP potrf, psd_safe_cholesky's jitter
        policy) times N(0, I) (``dgp_sample_draws``)."""
        Xnew = torch.tensor(self.dm.Xnew(covariates), dtype=self.dtype).to(self.device).contiguous()
        self._eval_ready(Xnew)
        with torch.no_grad():
            mean, factor, _jitter = self._plan.posterior_factor(self._factor_theta, Xnew)
            mean = mean + self.model.prior_mean(Xnew)
            sim = self._plan.sample_draws(factor, Xnew.shape[0], mean, n)  # (n, m) = mean + (L z)^T, one HIP launch
        temp = self.dm.y_t_device(sim.reshape(-1))
        data = np.asarray(temp.data).reshape(n, -1)
        return DataArray(data, coords=dict(covariates.coords, draw=np.arange(n)),
                         dims=["draw"] + list(covariates.coords), attrs=temp.attrs)

    @is_fitted
    def aggregate(self, covariates, weights, freq="YE", ci=0.95, pred_noise=False, return_cov=False, max_bytes=None,
                  hyperparameters=False, prior=True, interval="lognormal"):
        """Exact mean and covariance of the period sums sum_{i in period} weights_i target_i over the points of
        ``covariates`` (``freq``: a resample alias -- "YE", "YE-SEP" for water years, "QE", "ME"), from the latent
        posterior (``pred_noise=True`` adds the likelihood's predictive noise to its diagonal): what ``sample()``, a
        product with the weights and ``resample(time=freq).sum()`` estimate by Monte Carlo, in one posterior
        covariance and one ``dgp_period_moments`` pass.  Points with a non-finite weight are skipped.  -> Dataset on a
        ``time`` coordinate of period-end labels with ``mean``, ``se``, ``lower`` / ``upper`` (approximate ``ci``
        interval: lognormal / normal with the exact moments) and ``n_points``; with ``return_cov`` also the (P, P)
        covariance.  ``max_bytes`` (default ``loads.DEFAULT_MAX_BYTES``): device budget of the dense path; a record whose
        m x m covariance does not fit it takes the streamed ``dgp_posterior_period_moments``.  ``hyperparameters=True`` adds
        ``se_hyper``, ``se_total`` and ``lower_total`` / ``upper_total`` (with ``return_cov`` also ``cov_hyper``): the
        hyperparameters' uncertainty propagated to FIRST ORDER (delta method) through the exact period Jacobian and the exact
        inverse Fisher information (``prior``: with the priors' curvature).  ``interval="three-moment"`` adds ``skewness`` -- the
        exact skewness of every period sum, from one ``dgp_period_third_moments`` on the dense covariance -- and fits ``lower`` /
        ``upper`` to three exact moments instead of two (a shifted lognormal; still a fitted shape).  See
        ``discontinuum_amd.loads``."""
        from ..loads import DEFAULT_MAX_BYTES, aggregate

        if hyperparameters:
            self._refuse_censored("aggregate(hyperparameters=True)")
        return aggregate(self, covariates, weights, freq=freq, ci=ci, pred_noise=pred_noise, return_cov=return_cov,
                         max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes, hyperparameters=hyperparameters, prior=prior,
                         interval=interval)

    @is_fitted
    def exceedance(self, covariates, threshold=None, threshold_series=None, freq="YE", above=True, fraction=False, ci=0.95,
                   pred_noise=False, return_cov=False, max_bytes=None, streamed=False, window=None, align="right",
                   min_periods=None, statistic=None):
        """Expected number of points per period of ``freq`` at which the target exceeds a data-space threshold -- days per
        year above a criterion, for a daily record -- with its exact standard error: what ``sample()``, a comparison and a
        count per period estimate by Monte Carlo, in one posterior covariance and one ``dgp_exceedance_moments`` pass.
        ``threshold``: a number or a list of levels; ``threshold_series``: one threshold per point, (m,) or (L, m); exactly
        one of them.  ``above=False``: the complement; ``fraction=True``: divided by the points of the period.  -> Dataset
        on (``level``, ``time``) with ``mean``, ``se``, ``lower`` / ``upper`` (approximate ``ci`` interval: a beta
        distribution with the exact moments) and ``n_points``; with ``return_cov`` also the (L, P, P) covariance.  A record
        whose m x m covariance does not fit ``max_bytes`` (default ``loads.DEFAULT_MAX_BYTES``) raises ``ValueError``;
        ``streamed=True`` produces the covariance a panel of rows at a time instead (``dgp_posterior_exceedance_moments``) and
        works at any record length, with ``max_bytes`` bounding its work area.  ``window`` ("30D", "7D", ...; with ``align`` and
        ``min_periods`` as in ``rolling_mean``): the days on which the ROLLING mean over that averaging period -- the geometric
        mean for a log target -- exceeds the threshold, from one more pass (``dgp_window_moments``) between the two; without it
        the product is what it always was.  See ``discontinuum_amd.exceedance``."""
        from ..exceedance import exceedance
        from ..loads import DEFAULT_MAX_BYTES

        return exceedance(self, covariates, threshold=threshold, threshold_series=threshold_series, freq=freq, above=above,
                          fraction=fraction, ci=ci, pred_noise=pred_noise, return_cov=return_cov,
                          max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes, streamed=streamed, window=window,
                          align=align, min_periods=min_periods, statistic=statistic)

    @is_fitted
    def extreme_probability(self, covariates, threshold=None, threshold_series=None, kind="max", freq="YE", window=None,
                            align="right", min_periods=None, npoints=4096, nshifts=16, seed=0, max_bytes=None, pred_noise=False,
                            streamed=False, statistic=None):
        """Per period of ``freq`` the probability that the target stays below (``kind="max"``) or above (``"min"``) a
        data-space threshold at EVERY point of the period -- "not exceeded once in the year" -- as ``prob_never``, with
        ``prob_any`` = 1 - prob_never: the distribution function of the period's maximum (survival function of its minimum) at
        that level.  An orthant probability of the period's block of the posterior covariance, by a randomly shifted
        quasi-Monte-Carlo sweep on the device (``dgp_orthant_probability``): the one product that is NOT exact -- unbiased, with
        its own standard error ``error`` (about 1e-3 for a daily year at the defaults).  ``window``: the extreme of the rolling
        mean (``kind="min"``, ``window="7D"``: the 7-day low flow).  -> Dataset on (``level``, ``time``) with ``prob_never``,
        ``prob_any``, ``error``, ``n_points``.  See ``discontinuum_amd.extremes`` (also for the refusals)."""
        from ..extremes import extreme_probability
        from ..loads import DEFAULT_MAX_BYTES

        return extreme_probability(self, covariates, threshold=threshold, threshold_series=threshold_series, kind=kind, freq=freq,
                                   window=window, align=align, min_periods=min_periods, npoints=npoints, nshifts=nshifts, seed=seed,
                                   max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes, pred_noise=pred_noise,
                                   streamed=streamed, statistic=statistic)

    @is_fitted
    def extreme_quantiles(self, covariates, q=(0.05, 0.5, 0.95), kind="max", freq="YE", window=None, align="right",
                          min_periods=None, npoints=4096, nshifts=16, seed=0, max_bytes=None, grid=None, rounds=3, pred_noise=False,
                          streamed=False, statistic=None):
        """The ``q``-quantiles of every period's maximum (``kind="max"``) or minimum (``"min"``) of the target in data space --
        the annual peak with its interval, the annual minimum of a 7-day mean (``window="7D"``) -- by a bracketing search over
        levels on ``extreme_probability``'s sweep.  -> Dataset on (``quantile``, ``time``) with ``value``, ``bracket`` (the
        final bracket's width), ``bracket_prob``, ``error`` and ``n_points``.  NOT exact; see ``discontinuum_amd.extremes``."""
        from ..extremes import extreme_quantiles
        from ..loads import DEFAULT_MAX_BYTES

        return extreme_quantiles(self, covariates, q=q, kind=kind, freq=freq, window=window, align=align, min_periods=min_periods,
                                 npoints=npoints, nshifts=nshifts, seed=seed, max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes,
                                 grid=grid, rounds=rounds, pred_noise=pred_noise, streamed=streamed, statistic=statistic)

    @is_fitted
    def exceedance_distribution(self, covariates, threshold=None, threshold_series=None, freq="YE", above=True, window=None,
                                align="right", min_periods=None, npoints=4096, nshifts=16, seed=0, max_bytes=None, pred_noise=False,
                                streamed=False, kind=None, statistic=None):
        """Per period of ``freq`` the DISTRIBUTION of the number N of points at which the target lies above (``above=False``:
        below) a data-space threshold -- P(N <= k), for "no more than k exceedances in the year" -- and of the longest spell R
        of consecutive such points.  Joint paths of the period's block of the posterior are drawn, compared and counted on the
        device (``dgp_path_counts``) over the orthant sweep's randomly shifted rules: NOT exact -- unbiased, every value with its
        own standard error.  -> Dataset on (``level``, ``time``, ``count``) with ``pmf``, ``cdf``, ``cdf_error``, ``spell_pmf``,
        ``spell_cdf``, ``spell_cdf_error``, and on (``level``, ``time``) ``mean``, ``mean_error``, ``variance``,
        ``variance_error``, ``n_points``.  Spells are cut at period boundaries and at gaps of the record.  See
        ``discontinuum_amd.frequency`` (also for the refusals)."""
        from ..frequency import exceedance_distribution
        from ..loads import DEFAULT_MAX_BYTES

        return exceedance_distribution(self, covariates, threshold=threshold, threshold_series=threshold_series, freq=freq,
                                       above=above, window=window, align=align, min_periods=min_periods, npoints=npoints,
                                       nshifts=nshifts, seed=seed, max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes,
                                       pred_noise=pred_noise, streamed=streamed, kind=kind, statistic=statistic)

    @is_fitted
    def compliance_probability(self, covariates, threshold=None, threshold_series=None, allowed=None, allowed_fraction=None,
                               max_spell=None, freq="YE", above=True, window=None, align="right", min_periods=None, npoints=4096,
                               nshifts=16, seed=0, max_bytes=None, pred_noise=False, streamed=False, kind=None, statistic=None):
        """Per period of ``freq`` the probability that a frequency rule is met: ``prob`` = P(N <= ``allowed``), or
        P(N <= floor(``allowed_fraction`` x the period's points)), N the points beyond the threshold; with ``max_spell`` also
        ``prob_spell`` = P(longest spell <= ``max_spell``).  Exactly one of ``allowed`` / ``allowed_fraction``.  Read from
        ``exceedance_distribution``'s sweep: NOT exact, with ``error`` / ``error_spell``.  -> Dataset on (``level``, ``time``),
        with ``allowed_count`` and ``n_points`` on ``time``.  See ``discontinuum_amd.frequency``."""
        from ..frequency import compliance_probability
        from ..loads import DEFAULT_MAX_BYTES

        return compliance_probability(self, covariates, threshold=threshold, threshold_series=threshold_series, allowed=allowed,
                                      allowed_fraction=allowed_fraction, max_spell=max_spell, freq=freq, above=above, window=window,
                                      align=align, min_periods=min_periods, npoints=npoints, nshifts=nshifts, seed=seed,
                                      max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes, pred_noise=pred_noise,
                                      streamed=streamed, kind=kind, statistic=statistic)

    @is_fitted
    def rolling_mean(self, covariates, window, statistic=None, align="right", min_periods=None, ci=0.95, return_cov=False,
                     max_bytes=None, streamed=False):
        """The rolling mean of the target over ``window`` ("30D", "7D", "96h" or a ``numpy.timedelta64``; membership by time,
        so gaps and irregular records are handled) with its exact uncertainty: what ``sample()`` and a rolling mean of every
        draw estimate by Monte Carlo, in one posterior covariance and one ``dgp_window_moments`` pass.  ``statistic=None`` is
        the model-space mean -- the GEOMETRIC mean for a log target, exactly lognormal, with an exact ``ci`` interval; the
        plain mean for a linear one --; ``statistic="mean"`` on a log target is the arithmetic n-day mean (mean and se exact,
        interval approximate).  ``align="right"``: the trailing window (t - window, t]; ``"center"``: [t - window / 2,
        t + window / 2).  ``min_periods=None``: the largest point count any window of the record holds, so that leading
        partial windows and windows over gaps are left out.  -> Dataset on the qualifying outputs' ``time`` with ``mean``,
        ``se``, ``lower``, ``upper`` and ``n_points``; with ``return_cov`` also the (q, q) covariance.  ``streamed=True``
        (never chosen automatically): the same Dataset without the dense covariance, from the band of it the windows reach
        (``dgp_posterior_window_variances``), for records of any length; ``max_bytes`` bounds its work area and ``return_cov``
        is refused.  See ``discontinuum_amd.rolling``."""
        from ..loads import DEFAULT_MAX_BYTES
        from ..rolling import rolling_mean

        return rolling_mean(self, covariates, window, statistic=statistic, align=align, min_periods=min_periods, ci=ci,
                            return_cov=return_cov, max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes, streamed=streamed)

    @is_fitted
    def sample_value(self, covariates, weights, freq="YE", sample_var=None, given=None, ci=0.95, max_bytes=None, streamed=False):
        """For every day of ``covariates``: by how much one more sample on that day is expected to reduce the variance of
        each period sum sum_{i in period} weights_i target_i (hyperparameters held fixed, the expectation over the
        not-yet-seen sample value) -- one posterior covariance and one ``dgp_sample_value`` pass, where the reference would
        refit on simulated data.  ``sample_var``: the sample's model-space noise variance (default: the likelihood's
        learned noise); ``given``: dates or indices of samples to condition on first.  -> Dataset on (``period``, ``time``)
        with ``variance_reduction``, ``se_now``, ``se_expected`` and a per-day ``score``.  ``streamed=True``: the path for
        records whose dense covariance exceeds ``max_bytes`` (row panels, never the whole matrix).  See
        ``discontinuum_amd.design.sample_value``."""
        from ..design import sample_value
        from ..loads import DEFAULT_MAX_BYTES

        return sample_value(self, covariates, weights, freq=freq, sample_var=sample_var, given=given, ci=ci,
                            max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes, streamed=streamed)

    @is_fitted
    def design_value(self, covariates, weights, samples, freq="YE", sample_var=None, return_cov=False, max_bytes=None,
                     streamed=False):
        """The exact expected value of a sampling design: per period the variance of the period sum that samples on the days
        ``samples`` (dates or indices) explain, with ``se_now``, ``se_expected`` and the explained ``fraction``; with
        ``return_cov`` also the (P, P) matrix.  See ``discontinuum_amd.design.design_value``."""
        from ..design import design_value
        from ..loads import DEFAULT_MAX_BYTES

        return design_value(self, covariates, weights, samples, freq=freq, sample_var=sample_var, return_cov=return_cov,
                            max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes, streamed=streamed)

    @is_fitted
    def design(self, covariates, weights, k, objective="relative", candidates=None, replicates=False, given=None, freq="YE",
               sample_var=None, max_bytes=None, streamed=False):
        """Greedy choice of ``k`` days to sample for the period sums' uncertainty: exact for linear targets and for the
        first pick of log targets, a plug-in approximation of the marginal gain after that; the reported value of every
        nested prefix of the chosen design is exact.  -> Dataset along ``pick``.  See ``discontinuum_amd.design.design``."""
        from ..design import design
        from ..loads import DEFAULT_MAX_BYTES

        return design(self, covariates, weights, k, objective=objective, candidates=candidates, replicates=replicates,
                      given=given, freq=freq, sample_var=sample_var, max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes,
                      streamed=streamed)

    @is_fitted
    def influence(self, covariates, weights, folds="loo", freq="YE", max_bytes=None):
        """What the samples in hand were worth: for every fold of training observations (``folds``: everything
        ``cross_validate`` accepts) the exact change of every period sum sum_{i in period} weights_i target_i over the points of
        ``covariates`` had that fold not been sampled -- case deletion at fixed hyperparameters in one ``predict`` and one
        ``dgp_deletion_influence`` pass, where the reference would refit once per deletion.  -> Dataset on (``fold``,
        ``period``) with ``load_change`` (without the fold minus with it), ``relative_change``, ``load_without``,
        ``fold_size``, ``max_shift``, ``info``, ``se_jackknife`` and, for linear targets, ``var_change`` / ``se_without``.
        See ``discontinuum_amd.influence.influence``."""
        from ..influence import influence

        self._refuse_censored("influence")
        return influence(self, covariates, weights, folds=folds, freq=freq, max_bytes=max_bytes)

    @is_fitted
    def duration_curve(self, covariates, levels=None, above=True, ci=0.95, pred_noise=False, max_bytes=None, streamed=False,
                       window=None, align="right", min_periods=None, statistic=None):
        """Fraction of the record ``covariates`` on which the target exceeds each of ``levels`` (default: 21 quantiles of
        the posterior mean), with the exact standard error of that fraction and approximate ``ci`` intervals -- for a
        rating model over a stage record, the flow-duration curve.  -> Dataset on ``level`` with ``mean``, ``se``,
        ``lower``, ``upper``.  ``max_bytes`` / ``streamed``, ``window`` / ``align`` / ``min_periods``: as for ``exceedance``.
        See ``discontinuum_amd.exceedance.duration_curve``."""
        from ..exceedance import duration_curve
        from ..loads import DEFAULT_MAX_BYTES

        return duration_curve(self, covariates, levels=levels, above=above, ci=ci, pred_noise=pred_noise,
                              max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes, streamed=streamed, window=window,
                              align=align, min_periods=min_periods, statistic=statistic)

    @is_fitted
    def exceedance_probability(self, covariates, threshold, above=True, pred_noise=False, window=None, align="right",
                               min_periods=None, max_bytes=None, streamed=False):
        """Pointwise probability that the target exceeds ``threshold`` (a data-space number or one value per point) at each
        point of ``covariates``, from the prediction's mean and variance.  -> DataArray on the covariates' coordinate.  See
        ``discontinuum_amd.exceedance.exceedance_probability``.  ``window``: the same for the rolling mean over that window, on the
        qualifying outputs' ``time``; ``streamed=True`` (with ``window``): from the streamed band pass, without the dense
        covariance."""
        from ..exceedance import exceedance_probability
        from ..loads import DEFAULT_MAX_BYTES

        return exceedance_probability(self, covariates, threshold, above=above, pred_noise=pred_noise, window=window, align=align,
                                      min_periods=min_periods, max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes,
                                      streamed=streamed)

    @is_fitted
    def excess(self, covariates, threshold=None, threshold_series=None, weights=None, freq="YE", above=True, ci=0.95,
               pred_noise=False, return_cov=False, max_bytes=None, streamed=False):
        """BY HOW MUCH a threshold is overshot: per period of ``freq`` the expected sum_i w_i (c_i - tau_i)^+ of the
        data-space target over the points of ``covariates`` -- ``above=False``: the deficit sum_i w_i (tau_i - c_i)^+ -- with
        its exact standard error, in one posterior covariance and one ``dgp_excess_moments`` pass (log targets).  With
        ``weights`` = seconds per step over a stage record: the flood volume above bankfull, or the deficit volume below a
        low-flow threshold.  -> Dataset on (``level``, ``time``): ``mean``, ``se``, approximate ``lower`` / ``upper``,
        ``total``, ``share`` (a ratio of expectations), ``n_points``.  A record whose dense footprint exceeds ``max_bytes``
        (default ``loads.DEFAULT_MAX_BYTES``; a 15-minute stage record of sixteen months already does) is refused;
        ``streamed=True`` (never chosen automatically) produces the covariance a panel of rows at a time instead
        (``dgp_posterior_excess_moments``) and ``max_bytes`` then bounds its work area.  See ``discontinuum_amd.excess.excess``."""
        from ..excess import excess
        from ..loads import DEFAULT_MAX_BYTES

        return excess(self, covariates, threshold=threshold, threshold_series=threshold_series, weights=weights, freq=freq,
                      above=above, ci=ci, pred_noise=pred_noise, return_cov=return_cov,
                      max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes, streamed=streamed)

    @is_fitted
    def cross_validate(self, folds="loo", ci=0.95, return_folds=False, laplace=None):
        """Exact leave-one-out / leave-group-out cross-validation of the training observations at the fitted
        hyperparameters, from the factorisation the engine holds (no refit; ``dgp_cross_validate``).  ``folds``: "loo", a
        resample alias ("YE", "YE-SEP", "QE", "ME": one fold per period), an int k (contiguous blocks in time), ``("random",
        k, seed)`` or an explicit array of fold ids.  -> Dataset of ``observed`` / ``predicted`` / ``se`` / ``lower`` /
        ``upper`` / ``z`` / ``fold`` with ``elpd``, ``rmse``, ``coverage`` among its attributes; see
        ``discontinuum_amd.validation.cross_validate``.  A fit with censored observations is refused unless
        ``laplace="cavity"`` asks for the Laplace cavity folds (``dgp_laplace_cross_validate``): approximate -- the pseudo-data
        of the rows that stay are held at the full-data mode -- with a pointwise ``elpd``, PIT intervals for censored rows and
        ``rmse`` / ``coverage`` over the observed rows only."""
        from ..validation import cross_validate

        return cross_validate(self, folds=folds, ci=ci, return_folds=return_folds, laplace=laplace)

    @is_fitted
    def decompose(self, covariates, groups=None, ci=0.95, return_cov=False):
        """Exact posterior of every additive part of the covariance at the points of ``covariates``, with the
        cross-covariances between the parts (``dgp_predict_terms``; one pass, from the factorisation the engine holds).
        -> Dataset on (``component``, the covariates' coordinate) with ``mean`` and ``se`` in the units of the transformed
        target, for log targets also the multiplicative ``factor`` with its exact ``ci`` interval; the components are the
        model's ``component_names`` plus the deterministic prior mean ``"mean"``.  ``groups={"shift": ("shift_1",
        "shift_2")}`` merges parts (variance from the cross-covariances).  See ``discontinuum_amd.components.decompose``."""
        from ..components import decompose

        return decompose(self, covariates, groups=groups, ci=ci, return_cov=return_cov)

    @is_fitted
    def slope(self, covariates, wrt=None, ci=0.95, return_cov=False):
        """Exact posterior of the DERIVATIVES of the fitted surface with respect to its covariates at the points of
        ``covariates`` (``dgp_predict_slopes``; one pass, from the factorisation the engine holds): d ln C / d ln Q, the
        trend rate d ln C / dt, d ln Q / d stage.  ``wrt``: a covariate name or a list of names (default: all).  -> Dataset
        on (``wrt``, the covariates' coordinate) with ``mean``, ``se``, ``lower`` / ``upper`` (exact central ``ci`` interval)
        and ``prob_positive``, in units of the transformed target per unit of the covariate (of its logarithm for log
        covariates, per year for time).  See ``discontinuum_amd.slopes.slope``."""
        from ..slopes import slope

        return slope(self, covariates, wrt=wrt, ci=ci, return_cov=return_cov)

    @is_fitted
    def hyperparameter_uncertainty(self, ci=0.95, prior=True):
        """How well the data determine the hyperparameters: standard errors, ``ci`` intervals and correlations of every
        trainable parameter from the exact Fisher information of the marginal likelihood at the fitted values (``dgp_fisher``
        on the factorisation the engine holds; no refit, no second derivatives).  ``prior=True`` adds the curvature of the
        priors.  -> Dataset indexed by ``parameter`` with ``estimate``, ``se``, ``lower`` / ``upper``, ``se_raw``, ``active``,
        ``cov_raw``, ``corr``, ``information`` and the ``unidentified`` directions, in un-normalised log-likelihood units
        (the training objective is this divided by n).  See ``discontinuum_amd.hyperpar.hyperparameter_uncertainty``."""
        from ..hyperpar import hyperparameter_uncertainty

        self._refuse_censored("hyperparameter_uncertainty")
        return hyperparameter_uncertainty(self, ci=ci, prior=prior)

    @is_fitted
    def predict_marginalized(self, covariates, ci=0.95, prior=True, pred_noise=False):
        """``predict`` with the hyperparameters' uncertainty propagated to FIRST ORDER (delta method): Var_total[f*] =
        Var[f* | fitted] + J_mu Sigma_raw J_mu^T, J_mu the exact Jacobian of the posterior mean at every prediction point
        (one ``dgp_predict_sensitivity`` on the factorisation the engine holds; no refit) and Sigma_raw the exact inverse
        Fisher information of ``hyperparameter_uncertainty`` (``prior=True``: with the priors' curvature; inactive, clamped
        and unidentified directions contribute zero).  -> Dataset on the covariates' coordinates with ``mean``,
        ``se_plugin`` (``predict``'s, bitwise), ``se_hyper``, ``se`` (total), ``lower`` / ``upper``, ``inflation``,
        ``var_plugin`` / ``var_hyper``.  Second-order terms are not included.  See
        ``discontinuum_amd.hyperpar.predict_marginalized``."""
        from ..hyperpar import predict_marginalized

        self._refuse_censored("predict_marginalized")
        return predict_marginalized(self, covariates, ci=ci, prior=prior, pred_noise=pred_noise)

    def build_model(self, X, y, **kwargs):
        raise NotImplementedError("This method must be implemented in a subclass")
