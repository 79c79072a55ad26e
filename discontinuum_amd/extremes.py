"""Period maxima and minima of a fitted model's posterior: the probability that a criterion is never exceeded in a period,
the distribution of the annual peak, the annual minimum of an n-day mean.

Every other product of a held factorisation is a moment or a linear functional of the latent posterior f ~ N(mu, C).  The
extreme of a period is neither: P(max_{i in period} f_i <= u_i) is a multivariate normal orthant probability in as many
dimensions as the period has points, taken over the period's block of the covariance ``dgp_posterior_cov`` writes.  It is
computed by Genz's separation of variables -- the block is factored (``psd_safe_factor``'s blocked potrf, always in float64,
with the jitter ladder of the covariance's own dtype) and a randomly shifted quasi-Monte-Carlo rule runs over a sequential conditioning recurrence on the
device (``dgp_orthant_probability``, csrc/dgp_orthant.hip).

This is the one product here that is NOT EXACT.  It is exact in expectation (the estimator is unbiased) and reports its own
standard error, ``error``: the sample standard deviation of ``nshifts`` independently shifted rules over sqrt(nshifts).  That
error is not the sampling noise of ``sample()``: on a 365-day block 16 shifts x 4096 points give about 1e-3, for which joint
draws of the record would have to number about 1e5.  Everything before the sweep -- the covariance, the threshold's exact
monotone map to model space, the window's W C W^T -- is as exact as in ``exceedance``; censored and EP fits hold an ordinary
latent posterior (Gaussian BY APPROXIMATION) and take the same path.
"""
from __future__ import annotations

import numpy as np
import torch
from scipy.special import ndtri

from .backend import MODE_LOG, ORTHANT_MAX_DIM, ORTHANT_MAX_LEVELS, GPPlan
from .exceedance import WINDOW_REFUSALS, _data_space, _output_groups, model_space_threshold
from .loads import DEFAULT_MAX_BYTES, _kept, _site_bytes, _target_attrs, period_groups, target_transform
from .xr_compat import Dataset

KINDS = ("max", "min")

REFUSALS = {
    "streamed": "period extremes need the dense posterior covariance: the sweep factors every period's block of it, and the "
                "streamed passes never hold a block whole; drop streamed=True",
    "pred_noise": "pred_noise=True is not implemented for period extremes: the extreme of hypothetical noisy observations is "
                  "not the extreme of the target",
    "flux": "kind='flux' is not implemented for period extremes: the peak daily load has a different threshold on every day; "
            "pass the per-day concentration thresholds as threshold_series with kind='max'",
    "statistic": "the extreme of the arithmetic rolling mean of a log target is not implemented: that mean is a sum of "
                 "lognormals, not a Gaussian; use the model-space statistic (the geometric mean)",
}


def _check_request(model, kind, pred_noise, streamed, window, statistic):
    """The refusals of a period extreme, each saying why; -> nothing."""
    if kind == "flux":
        raise NotImplementedError(REFUSALS["flux"])
    if kind not in KINDS:
        raise ValueError(f"kind must be 'max' or 'min', not {kind!r}")
    if streamed:
        raise NotImplementedError(REFUSALS["streamed"])
    if pred_noise:
        raise ValueError(REFUSALS["pred_noise"])
    mode, _s, _t = target_transform(model.dm)
    model_space = "geometric_mean" if mode == MODE_LOG else "mean"
    if statistic is not None and statistic not in ("mean", "geometric_mean"):
        raise ValueError(f"statistic must be 'mean' or 'geometric_mean', not {statistic!r}")
    if statistic is not None and window is None:
        raise ValueError("statistic applies to a rolling mean: give window=")
    if statistic == "mean" and mode == MODE_LOG:
        raise NotImplementedError(REFUSALS["statistic"])
    if statistic is not None and statistic != model_space:
        raise ValueError(f"the model-space statistic of this target is {model_space!r}, not {statistic!r}")


def check_budget(dense_bytes, longest, max_bytes):
    """The footprint and size refusals: a record whose dense path exceeds ``max_bytes`` (the text pattern of the three-moment
    interval's), and a period longer than the sweep's limit."""
    if dense_bytes > max_bytes:
        raise NotImplementedError(f"period extremes need the dense m x m covariance: this record ({dense_bytes} bytes dense, "
                                  f"max_bytes = {max_bytes}) takes the streamed passes, for which no orthant sweep exists")
    if longest > ORTHANT_MAX_DIM:
        raise ValueError(f"a period holds {longest} points, more than the orthant sweep's limit of {ORTHANT_MAX_DIM} dimensions; "
                         "use a shorter freq")


class _Periods:
    """What one call prepares and every sweep reuses: the kept outputs in period order, their model-space mean, and per
    non-empty period the outputs' positions and the float64 factor of its block of the covariance."""

    def __init__(self, model, covariates, freq, window, align, min_periods, max_bytes):
        time = np.asarray(covariates.coords["time"].values).reshape(-1)
        self.m_all = len(time)
        esz = torch.empty((), dtype=model.dtype).element_size()
        if window is not None:
            from .rolling import time_windows, window_bytes

            Xall = np.asarray(model.dm.Xnew(covariates))
            order, lo, hi, keep = time_windows(time, window, align, min_periods, valid=np.all(np.isfinite(Xall), axis=1))
            if not keep.any():
                raise ValueError(f"no window of the record holds min_periods = {min_periods} points")
            groups, labels, n_points = _output_groups(time[order], keep, freq)
            extra = window_bytes(len(order), len(lo))
        else:
            order, groups, labels, n_points, _dropped = _kept(*period_groups(time, np.ones(self.m_all), freq))
            extra = 0
        self.order, self.groups, self.labels, self.n_points = order, np.asarray(groups), labels, np.asarray(n_points)
        m = len(order)
        self.dense_bytes = _site_bytes(model.dm.X.shape[0], m, esz) + extra
        check_budget(self.dense_bytes, int(self.n_points.max()) if len(self.n_points) else 0, max_bytes)
        self.sweep_bytes = int(max_bytes) - self.dense_bytes
        Xnew = torch.tensor(model.dm.Xnew(covariates), dtype=model.dtype)[torch.as_tensor(order)].to(model.device).contiguous()
        model._eval_ready(Xnew)
        plan = self.plan = model._plan
        with torch.no_grad():
            kmean, cov = plan.posterior_cov(model._factor_theta, Xnew)
            mu = (kmean + model.model.prior_mean(Xnew)).contiguous()
            if window is not None:
                mu, cov = plan.window_moments(cov, m, mu, torch.from_numpy(np.ascontiguousarray(lo)), torch.from_numpy(np.ascontiguousarray(hi)))
            self.mu = mu.double().cpu().numpy()
            self.sd = torch.sqrt(torch.clamp(torch.diagonal(cov)[:m].double(), min=0.0)).cpu().numpy()
            host = plan if plan.dtype == torch.float64 else self._host_plan(model)
            ladder = plan._jitter_ladder() if hasattr(plan, "_jitter_ladder") else None  # the ladder of the COVARIANCE's dtype
            self.blocks, self.jitter = [], 0.0
            for g in range(len(labels)):
                idx = np.nonzero(self.groups == g)[0]
                if idx.size == 0:
                    continue
                it = torch.as_tensor(idx, device=cov.device)
                blk = cov.index_select(0, it).index_select(1, it).double()  # rows >= columns: the valid lower triangle
                blk = torch.tril(blk) + torch.tril(blk, -1).T
                M = -(-idx.size // 128) * 128
                full = torch.eye(M, dtype=torch.float64, device=cov.device)
                full[:idx.size, :idx.size] = blk
                Lbuf, jitter = host.psd_safe_factor(full.contiguous(), int(idx.size), ladder=ladder)
                self.blocks.append((g, idx, Lbuf.clone()))
                self.jitter = max(self.jitter, float(jitter))

    @staticmethod
    def _host_plan(model):
        """A float64 plan whose ``psd_safe_factor`` factors the blocks of a float32 model: kept on the model."""
        host = getattr(model, "_extreme_host", None)
        if host is None or host.device != model._plan.device:
            host = model._extreme_host = GPPlan(model._plan.model, 128, model._plan.d, dtype=torch.float64, device=model._plan.device)
        return host

    def sweep(self, u, kind, npoints, nshifts, seed):
        """Model-space thresholds ``u`` (L, kept outputs) -> (prob_never (L, P), error (L, P)); NaN for an empty period."""
        u = np.asarray(u, dtype=np.float64)
        L, P = u.shape[0], len(self.labels)
        prob, err = np.full((L, P), np.nan), np.full((L, P), np.nan)
        for g, idx, Lbuf in self.blocks:
            c = u[:, idx] - self.mu[idx][None, :]
            inf = np.full_like(c, np.inf)
            lo, hi = (-inf, c) if kind == "max" else (c, inf)
            for l0 in range(0, L, ORTHANT_MAX_LEVELS):
                p, e = self.plan.orthant_probability(Lbuf, int(idx.size), lo[l0:l0 + ORTHANT_MAX_LEVELS], hi[l0:l0 + ORTHANT_MAX_LEVELS],
                                                     npoints=npoints, nshifts=nshifts, seed=seed, max_bytes=self.sweep_bytes)
                prob[l0:l0 + ORTHANT_MAX_LEVELS, g] = p.cpu().numpy()
                err[l0:l0 + ORTHANT_MAX_LEVELS, g] = e.cpu().numpy()
        return np.clip(prob, 0.0, 1.0), err


def _threshold_rows(threshold, threshold_series, m_all):
    """(levels coordinate, (L, m_all) data-space series) from exactly one of the two arguments, as ``exceedance`` reads them."""
    if (threshold is None) == (threshold_series is None):
        raise ValueError("give exactly one of threshold and threshold_series")
    if threshold is not None:
        levels = np.atleast_1d(np.asarray(threshold, dtype=np.float64))
        if levels.ndim != 1 or levels.size == 0:
            raise ValueError("threshold must be a number or a 1-D list of levels")
        return levels, np.broadcast_to(levels[:, None], (levels.size, m_all))
    series = np.asarray(threshold_series, dtype=np.float64)
    series = series[None, :] if series.ndim == 1 else series
    if series.ndim != 2 or series.shape[1] != m_all or series.shape[0] == 0:
        raise ValueError(f"threshold_series must have shape ({m_all},) or (L, {m_all})")
    return np.arange(series.shape[0]), series


def _attrs(model, kind, window, align, npoints, nshifts, seed, jitter):
    attrs = dict(_target_attrs(model.dm), kind=kind, npoints=int(npoints), nshifts=int(nshifts), seed=int(seed), jitter=float(jitter),
                 exact=False)
    if window is not None:
        attrs.update(window=str(window), align=align, statistic="geometric_mean" if target_transform(model.dm)[0] == MODE_LOG else "mean")
    return attrs


def extreme_probability(model, covariates, threshold=None, threshold_series=None, kind="max", freq="YE", window=None, align="right",
                        min_periods=None, npoints=4096, nshifts=16, seed=0, max_bytes: int = DEFAULT_MAX_BYTES, pred_noise=False,
                        streamed=False, statistic=None):
    """``MarginalHIP.extreme_probability``: per period of ``freq`` the probability that the target stays on the safe side of a
    threshold at EVERY point of the period -- ``kind="max"``: P(target <= threshold throughout), the distribution function of
    the period's maximum at that level; ``kind="min"``: P(target >= threshold throughout), the survival function of its minimum.

    ``threshold`` / ``threshold_series``, the exact map to model space, the periods and the dropped points: as for
    ``exceedance``.  ``window`` (with ``align``, ``min_periods``): the extreme of the ROLLING mean over that window (the
    geometric mean for a log target) -- ``kind="min"`` with ``window="7D"`` on a stage record is the 7-day low-flow statistic.
    -> Dataset on (``level``, ``time``) with ``prob_never``, ``prob_any`` = 1 - prob_never, ``error`` (the standard error of the
    estimate: this product is NOT exact, see the module's text) and ``n_points``; the attrs carry ``npoints``, ``nshifts``,
    ``seed`` and ``jitter``, the largest jitter a block's factorisation needed.  An empty period holds NaN.
    Refused, each with its reason: ``streamed=True`` and a record whose dense footprint exceeds ``max_bytes``,
    ``pred_noise=True``, ``kind="flux"``, the arithmetic ``statistic="mean"`` of a log target, a period of more than
    ``backend.ORTHANT_MAX_DIM`` points."""
    _check_request(model, kind, pred_noise, streamed, window, statistic)
    time = np.asarray(covariates.coords["time"].values).reshape(-1)
    levels, series = _threshold_rows(threshold, threshold_series, len(time))
    periods = _Periods(model, covariates, freq, window, align, min_periods, max_bytes)
    u = model_space_threshold(model.dm, series[:, periods.order])
    prob, err = periods.sweep(u, kind, npoints, nshifts, seed)
    attrs = _attrs(model, kind, window, align, npoints, nshifts, seed, periods.jitter)
    dims = ("level", "time")
    return Dataset(
        {
            "prob_never": (dims, prob, attrs),
            "prob_any": (dims, 1.0 - prob, attrs),
            "error": (dims, err, attrs),
            "n_points": ("time", periods.n_points),
        },
        coords={"level": levels, "time": periods.labels},
        attrs=dict(attrs, freq=freq),
    )


def quantile_brackets(mu, sd, q, kind):
    """Model-space brackets [lo, hi] that hold the ``q``-quantiles of the maximum (minimum) of independent-or-not normals with
    means ``mu`` and deviations ``sd``, from the two elementary bounds on its distribution function F:
    max: F(t) <= min_i Phi_i(t) and 1 - F(t) <= sum_i (1 - Phi_i(t)); min: mirrored.  lo has F <= min(q) / 2,
    hi has F >= 1 - (1 - max(q)) / 2, whatever the correlations."""
    mu, sd, q = np.asarray(mu, dtype=np.float64), np.asarray(sd, dtype=np.float64), np.asarray(q, dtype=np.float64)
    m = mu.size
    a, b = q.min() / 2, (1 - q.max()) / 2
    if kind == "max":
        return float(np.max(mu + sd * ndtri(a))), float(np.max(mu - sd * ndtri(b / m)))
    return float(np.min(mu + sd * ndtri(a / m))), float(np.min(mu - sd * ndtri(b)))


def quantile_search(cdf, lo, hi, q, grid=16, rounds=3):
    """The bracketing search of ``extreme_quantiles`` on the host: for P periods and K probabilities ``q`` find t with
    F_p(t) = q_k for non-decreasing distribution functions known only through ``cdf(t (P, K, G)) -> (F (P, K, G), error)``.
    Every (period, probability) keeps its own bracket, starting at [lo_p, hi_p]; a round evaluates ``grid`` levels across every
    bracket in ONE call and shrinks each bracket to the adjacent pair of levels around q (the values made monotone by a running
    maximum first, so that noise cannot lose the bracket); after ``rounds`` rounds the answer is the linear interpolation in the
    last pair.  -> dict of (P, K) arrays: ``value``, ``lower`` / ``upper`` (the last pair), ``f_lower`` / ``f_upper`` (F there)
    and ``error`` (the larger of the pair's errors).  A q outside [F(lo), F(hi)] is answered by the nearer end."""
    lo, hi, q = np.asarray(lo, dtype=np.float64).reshape(-1), np.asarray(hi, dtype=np.float64).reshape(-1), np.asarray(q, dtype=np.float64).reshape(-1)
    P, K, G = lo.size, q.size, int(grid)
    if G < 3 or rounds < 1:
        raise ValueError("the search needs grid >= 3 and rounds >= 1")
    a, b = np.repeat(lo[:, None], K, axis=1), np.repeat(hi[:, None], K, axis=1)
    fa = fb = ea = eb = None
    frac = np.linspace(0.0, 1.0, G)
    for _ in range(int(rounds)):
        t = a[:, :, None] + (b - a)[:, :, None] * frac[None, None, :]
        F, E = cdf(t)
        F = np.maximum.accumulate(np.asarray(F, dtype=np.float64), axis=2)
        E = np.asarray(E, dtype=np.float64)
        # the last level with F <= q (at least the first), and its right neighbour
        j = np.clip((F <= q[None, :, None]).sum(axis=2) - 1, 0, G - 2)
        take = lambda x, jj: np.take_along_axis(x, jj[:, :, None], axis=2)[:, :, 0]  # noqa: E731
        a, b, fa, fb, ea, eb = take(t, j), take(t, j + 1), take(F, j), take(F, j + 1), take(E, j), take(E, j + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(fb > fa, (q[None, :] - fa) / np.where(fb > fa, fb - fa, 1.0), 0.5)
    value = a + np.clip(w, 0.0, 1.0) * (b - a)
    return dict(value=value, lower=a, upper=b, f_lower=fa, f_upper=fb, error=np.maximum(ea, eb))


def extreme_quantiles(model, covariates, q=(0.05, 0.5, 0.95), kind="max", freq="YE", window=None, align="right", min_periods=None,
                      npoints=4096, nshifts=16, seed=0, max_bytes: int = DEFAULT_MAX_BYTES, grid=None, rounds=3, pred_noise=False,
                      streamed=False, statistic=None):
    """``MarginalHIP.extreme_quantiles``: the ``q``-quantiles of every period's maximum (``kind="max"``) or minimum (``"min"``)
    of the target, in data space -- the annual peak with its interval, the annual minimum of a 7-day mean (``window="7D"``).

    A bracketing search over levels on top of ``extreme_probability``'s sweep (``quantile_search``): the covariance and the
    blocks' factors are produced once; every round runs ``grid`` levels (default: the most that keep one call at 64 levels,
    at most 16) for every probability and ALL periods, ``rounds`` rounds shrink each bracket by (grid - 1) per round from the
    elementary bounds of ``quantile_brackets``; the value is the monotone (linear) interpolation in the last bracket.  The
    same shifts serve every level and round, so the estimated distribution function is one smooth function of the level.
    -> Dataset on (``quantile``, ``time``) with ``value``, ``bracket`` (the last bracket's width, data space),
    ``bracket_prob`` (the probability mass between its ends), ``error`` (the standard error of the bracketing probabilities)
    and ``n_points``.  NOT exact, like ``extreme_probability``, whose refusals apply."""
    _check_request(model, kind, pred_noise, streamed, window, statistic)
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if q.ndim != 1 or q.size == 0 or q.size > ORTHANT_MAX_LEVELS // 3 or not np.all((q > 0) & (q < 1)):
        raise ValueError(f"q must be a 1-D list of at most {ORTHANT_MAX_LEVELS // 3} probabilities strictly between 0 and 1")
    G = min(16, ORTHANT_MAX_LEVELS // q.size) if grid is None else int(grid)
    periods = _Periods(model, covariates, freq, window, align, min_periods, max_bytes)
    P, K = len(periods.labels), q.size
    live = [g for g, _idx, _L in periods.blocks]
    lo, hi = np.zeros(P), np.ones(P)
    for g, idx, _L in periods.blocks:
        lo[g], hi[g] = quantile_brackets(periods.mu[idx], periods.sd[idx], q, kind)

    def cdf(t):  # (P, K, G) model-space levels -> the distribution function of the extreme and its error
        rows = t.reshape(P, K * G)
        u = np.zeros((K * G, len(periods.order)))
        for g, idx, _L in periods.blocks:
            u[:, idx] = rows[g][:, None]
        prob, err = periods.sweep(u, kind, npoints, nshifts, seed)
        F = prob if kind == "max" else 1.0 - prob
        F, err = np.where(np.isnan(F), 0.0, F), np.where(np.isnan(err), 0.0, err)
        return F.T.reshape(P, K, G), err.T.reshape(P, K, G)

    res = quantile_search(cdf, lo, hi, q, grid=G, rounds=rounds)
    dead = np.ones(P, dtype=bool)
    dead[live] = False
    out = {k: np.where(dead[:, None], np.nan, v).T for k, v in res.items()}  # (K, P)
    value, lower, upper = (_data_space(model, out[k]) for k in ("value", "lower", "upper"))
    attrs = dict(_attrs(model, kind, window, align, npoints, nshifts, seed, periods.jitter), grid=G, rounds=int(rounds))
    dims = ("quantile", "time")
    return Dataset(
        {
            "value": (dims, value, attrs),
            "bracket": (dims, upper - lower, attrs),
            "bracket_prob": (dims, out["f_upper"] - out["f_lower"], attrs),
            "error": (dims, out["error"], attrs),
            "n_points": ("time", periods.n_points),
        },
        coords={"quantile": q, "time": periods.labels},
        attrs=dict(attrs, freq=freq),
    )


__all__ = ["extreme_probability", "extreme_quantiles", "quantile_search", "quantile_brackets", "check_budget", "REFUSALS", "KINDS"]
