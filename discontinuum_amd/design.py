"""Exact value of additional samples for the period loads of a fitted model: monitoring design from the held fit.

Which days, had they been sampled, would have reduced the uncertainty of each period's load the most, and how much does a
given sampling scheme buy?  The reference could only answer by refitting on simulated data.  At FIXED hyperparameters the
answer is closed-form.  Let f ~ N(mu, C) be the latent posterior over the m days of a record (model space), c_i =
exp(s f_i + t) (log targets) or s f_i + t the data-space value and L_p = sum_{i in p} w_i c_i the period sums -- exactly
``loads.aggregate``'s setting.  A hypothetical sample y_c = f_c + eps, Var eps = tau_c^2, on day c changes the covariance
deterministically and the mean randomly.  With v_c = C_cc + tau_c^2, b_ic = C_ic / sqrt(v_c) and A_i = w_i exp(s mu_i + t
+ s^2 C_ii / 2) (A_i = w_i for a linear target), the law of total variance gives the EXPECTED reduction of Var(L_p):

    gain[p, c] = Var(E[L_p | y_c]) = sum_{i,j in p} A_i A_j expm1(s^2 b_ic b_jc)      (log)
    gain[p, c] = s^2 (sum_{i in p} A_i b_ic)^2                                       (linear)

computed for every day c and every period p in one pass over the covariance by ``dgp_sample_value`` (the exponential
series, ``backend.series_terms`` terms).  "Expected" means: the hyperparameters are held fixed, and the expectation is
over the not-yet-seen value of the sample.  A set S of samples conditions by the pivoted-Cholesky recurrence: rows
B_t = (C[:, c_t] - B_<t^T B_<t[:, c_t]) / sqrt(v'_{c_t}), v'_c = C_cc - sum_t B_tc^2 + tau_c^2, so that C | S = C - B^T B
and R = B^T B is the explained covariance.  The exact value of a whole design is

    V_pq(S) = Cov(E[L_p | y_S], E[L_q | y_S]) = sum_{i in p, j in q} A_i A_j expm1(s^2 R_ij)

(``dgp_period_moments`` on R with the mean shifted so that its a_i equals A_i); the expected remaining variance of L_p is
Var(L_p) - V_pp(S).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pandas as pd
import torch

from . import _lib
from .backend import MODE_LOG, series_terms
from .loads import DEFAULT_MAX_BYTES, _kept, _site_bytes, _target_attrs, intervals, period_groups, target_transform
from .xr_compat import Dataset

MAX_ROWS = 64  # conditioning rows of one ``dgp_sample_value`` call: samples given plus samples picked


def default_sample_var(model):
    """The model-space noise variance of a NEW sample: the likelihood's learned noise, as ``predictive_noise`` gives it for
    points that are not the training set (the fixed per-observation part belongs to the training points); 0 -- an exact
    measurement -- for a likelihood without a learned term."""
    second = model.likelihood.second_noise
    return 0.0 if second is None else float(second.detach().reshape(-1)[0])


def _prepare(model, covariates, weights, freq, sample_var, max_bytes, extra_buffers=0, streamed=False):
    """The shared front half: groups, the posterior covariance, the current moments, A_i, tau^2 and the series length.
    ``streamed``: no covariance -- the latent mean and variance from ``predict``, the current moments from
    ``posterior_period_moments``, a column provider (``posterior_cov_columns``) where the dense path carries ``cov``, and
    the panel height ``max_bytes`` leaves ``posterior_sample_value`` (a ``ValueError`` naming the bytes when 128 rows do
    not fit)."""
    time_all = np.asarray(covariates.coords["time"].values).reshape(-1).astype("datetime64[ns]")
    m_all = len(time_all)
    w_all = np.asarray(weights, dtype=np.float64).reshape(-1)
    order, groups, labels, n_points, _dropped = _kept(*period_groups(time_all, w_all, freq))
    m, P = len(order), len(labels)
    if sample_var is None:
        tau2 = np.full(m, default_sample_var(model))
    else:
        tau2 = np.asarray(sample_var, dtype=np.float64)
        if tau2.ndim == 0:
            tau2 = np.full(m, float(tau2))
        elif tau2.shape == (m_all,):
            tau2 = tau2[order]
        else:
            raise ValueError(f"sample_var must be a number or an array of shape ({m_all},)")
    if not np.all(np.isfinite(tau2)) or np.any(tau2 < 0):
        raise ValueError("sample_var must be finite and >= 0 (a model-space variance)")
    mode, s, t = target_transform(model.dm)
    esz = torch.empty((), dtype=model.dtype).element_size()
    M = int(_lib.load().dgp_padded_n(m))
    need = _site_bytes(model.dm.X.shape[0], m, esz) + extra_buffers * 8 * M * M
    if not streamed and need > max_bytes:
        raise ValueError(f"the value of samples needs the dense posterior covariance{' and a second (M, M) buffer' if extra_buffers else ''}"
                         f": a footprint of {need} bytes for m = {m} points exceeds max_bytes = {max_bytes}")
    Xnew = torch.tensor(model.dm.Xnew(covariates), dtype=model.dtype)[torch.as_tensor(order)].to(model.device).contiguous()
    model._eval_ready(Xnew)
    if streamed:
        return _prepare_streamed(model, Xnew, time_all, m_all, w_all, order, groups, labels, n_points, tau2, mode, s, t, freq, max_bytes)
    with torch.no_grad():
        kmean, cov = model._plan.posterior_cov(model._factor_theta, Xnew)
        dev = cov.device
        mapped = (s * (kmean + model.model.prior_mean(Xnew)) + t).contiguous()
        mean_d, cov_d = model._plan.period_moments(cov, m, mapped, s * s, w_all[order], groups, P, mode)
        w_t = torch.as_tensor(w_all[order], dtype=torch.float64, device=dev)
        diag = torch.diagonal(cov)[:m].double()
        a = w_t * torch.exp(mapped.double() + 0.5 * s * s * diag) if mode == MODE_LOG else w_t
        beta = s * s * float(diag.max()) if mode == MODE_LOG else 0.0
        # tau^2 as the kernel reads it (the buffer's dtype): the rows formed on the host divide by the same variance
        obs_var = torch.as_tensor(tau2, dtype=cov.dtype, device=dev)
    return SimpleNamespace(
        model=model, cov=cov, dev=dev, streamed=False, m=m, P=P, mode=mode, s2=s * s, mapped=mapped, diag=diag, w=w_all[order], groups=groups,
        labels=labels, n_points=n_points, order=order, time=time_all[order], m_all=m_all, a=a.contiguous(),
        tau2=obs_var.double(), obs_var=obs_var, nterms=series_terms(beta) if mode == MODE_LOG else 1,
        mean_now=mean_d.cpu().numpy(), cov_now=cov_d.cpu().numpy(), freq=freq)


def _prepare_streamed(model, Xnew, time_all, m_all, w_all, order, groups, labels, n_points, tau2, mode, s, t, freq, max_bytes):
    """``_prepare`` without the dense covariance (``streamed=True``): the same fields, ``cov`` = None, plus ``columns``
    (index list -> C[:, idx] as (len, m) float64), ``gain`` (rows -> ``posterior_sample_value``) and ``panel_rows``."""
    plan, theta = model._plan, model._factor_theta
    m, P = len(order), len(labels)
    with torch.no_grad():
        kmean, var = plan.predict(theta, Xnew)
        dev = var.device
        mapped = (s * (kmean + model.model.prior_mean(Xnew)) + t).contiguous()
        mean_d, cov_d = plan.posterior_period_moments(theta, Xnew, mapped, s * s, w_all[order], groups, P, mode)
        w_t = torch.as_tensor(w_all[order], dtype=torch.float64, device=dev)
        diag = var.double()
        a = w_t * torch.exp(mapped.double() + 0.5 * s * s * diag) if mode == MODE_LOG else w_t
        beta = s * s * float(diag.max()) if mode == MODE_LOG else 0.0
        obs_var = torch.as_tensor(tau2, dtype=var.dtype, device=dev)
    nterms = series_terms(beta) if mode == MODE_LOG else 1
    panel_rows = plan.sample_value_panel_rows(m, P, MAX_ROWS, nterms, max_bytes)
    fit = SimpleNamespace(
        model=model, cov=None, dev=dev, streamed=True, m=m, P=P, mode=mode, s2=s * s, mapped=mapped, diag=diag, w=w_all[order],
        groups=groups, labels=labels, n_points=n_points, order=order, time=time_all[order], m_all=m_all, a=a.contiguous(),
        tau2=obs_var.double(), obs_var=obs_var, nterms=nterms, mean_now=mean_d.cpu().numpy(), cov_now=cov_d.cpu().numpy(), freq=freq,
        panel_rows=panel_rows, columns=lambda idx: plan.posterior_cov_columns(theta, Xnew, idx))
    fit.gain = lambda rows: plan.posterior_sample_value(theta, Xnew, fit.a, fit.s2, groups, P, obs_var=obs_var, rows=rows,
                                                        nterms=nterms, panel_rows=panel_rows)
    return fit


def _day_indices(fit, days, what):
    """Dates or indices into the covariates' time axis -> positions among the kept, period-sorted days."""
    if days is None:
        return np.zeros(0, dtype=np.int64)
    days = np.atleast_1d(np.asarray(days))
    if days.dtype.kind in "iu":
        if days.size and (days.min() < 0 or days.max() >= fit.m_all):
            raise ValueError(f"{what}: index out of range for {fit.m_all} points")
        inverse = np.full(fit.m_all, -1, dtype=np.int64)
        inverse[fit.order] = np.arange(fit.m)
        pos = inverse[days]
        if np.any(pos < 0):
            raise ValueError(f"{what}: point {int(days[np.nonzero(pos < 0)[0][0]])} has no finite weight and time")
        return pos
    stamps = pd.DatetimeIndex(days).to_numpy().astype("datetime64[ns]")
    lookup = pd.Index(fit.time)
    pos = lookup.get_indexer(stamps)
    if np.any(pos < 0):
        raise ValueError(f"{what}: {pd.Timestamp(stamps[np.nonzero(pos < 0)[0][0]]).date()} is not a day of the record")
    return pos.astype(np.int64)


def _column(fit, c):
    """Column c of the symmetric covariance from the buffer's lower triangle, in double."""
    if fit.streamed:
        return fit.columns([int(c)])[0]
    return torch.cat([fit.cov[c, :c], fit.cov[c:fit.m, c]]).double()


def _next_row(fit, rows, c, var=None, col=None):
    """The conditioning row of a sample on day c after ``rows``: (C[:, c] - rows^T rows[:, c]) / sqrt(v'_c); ``var``: v'_c
    as ``dgp_sample_value`` returned it (default: computed here); ``col``: C[:, c] when the caller already holds it.  A
    sample with v'_c not > 0 carries nothing: a zero row."""
    col = _column(fit, c) if col is None else col
    if rows.shape[0]:
        col = col - rows.T @ rows[:, c]
    v = col[c] + fit.tau2[c] if var is None else var
    return col / torch.sqrt(v) if float(v) > 0 else torch.zeros_like(col)


def conditioning_rows(fit, picks):
    """Rows B (len(picks), m) of the pivoted-Cholesky recurrence for the samples ``picks`` (positions, in order)."""
    rows = torch.zeros(len(picks), fit.m, dtype=torch.float64, device=fit.dev)
    cols = None
    if fit.streamed and len(picks):  # every distinct day's column in calls of up to MAX_ROWS columns
        days = sorted({int(c) for c in picks})
        got = torch.cat([fit.columns(days[lo:lo + MAX_ROWS]) for lo in range(0, len(days), MAX_ROWS)])
        cols = {c: got[k] for k, c in enumerate(days)}
    for k, c in enumerate(picks):
        rows[k] = _next_row(fit, rows[:k], int(c), col=None if cols is None else cols[int(c)])
    return rows


def _explained_cov(fit, rows):
    """R = rows^T rows, the covariance the samples explain, as an (M, M) float64 buffer beside the posterior covariance."""
    M = fit.cov.shape[-1]
    padded = torch.zeros(rows.shape[0], M, dtype=torch.float64, device=fit.cov.device)
    padded[:, : fit.m] = rows
    return padded.T @ padded


def _explained(fit, R):
    """V(S) (P, P) of the design with explained covariance ``R``: ``period_moments`` on R with the mean shifted by
    s^2 (C_ii - R_ii) / 2, so that its a_i = w_i exp(mu_i + s^2 R_ii / 2) equals A_i."""
    shifted = (fit.mapped.double() + 0.5 * fit.s2 * (fit.diag - torch.diagonal(R)[: fit.m])).contiguous()
    _mean, V = fit.model._plan.period_moments(R, fit.m, shifted, fit.s2, fit.w, fit.groups, fit.P, fit.mode)
    return V.cpu().numpy()


def _explained_rows(fit, rows):
    """V(S) (P, P) of the design with conditioning rows ``rows``.  Dense: ``_explained`` on R = rows^T rows.  Streamed:
    ``lowrank_period_moments`` on the rows, the mean shifted by s^2 (C_ii - R_ii) / 2 in the same way -- no (M, M) buffer."""
    if not fit.streamed:
        return _explained(fit, _explained_cov(fit, rows))
    if rows.shape[0] == 0:
        return np.zeros((fit.P, fit.P))
    shifted = (fit.mapped.double() + 0.5 * fit.s2 * (fit.diag - (rows * rows).sum(dim=0))).contiguous()
    _mean, V = fit.model._plan.lowrank_period_moments(rows.contiguous(), fit.m, shifted, fit.s2, fit.w, fit.groups, fit.P, fit.mode)
    return V.cpu().numpy()


def _gain(fit, rows):
    """(gain, var) of one more sample after ``rows`` (None: none): ``sample_value`` on the dense covariance, or the streamed
    ``posterior_sample_value``."""
    if fit.streamed:
        return fit.gain(rows)
    return fit.model._plan.sample_value(fit.cov, fit.m, fit.a, fit.s2, fit.groups, fit.P, obs_var=fit.obs_var, rows=rows, nterms=fit.nterms)


def _se(var):
    return np.sqrt(np.clip(var, 0.0, None))


def sample_value(model, covariates, weights, freq="YE", sample_var=None, given=None, ci=0.95, max_bytes: int = DEFAULT_MAX_BYTES,
                 streamed=False):
    """``MarginalHIP.sample_value``: for every day of ``covariates`` the expected reduction of the variance of every period
    sum sum_{i in period} weights_i target_i, had that day been sampled -- one ``posterior_cov`` and one
    ``dgp_sample_value``.  "Expected": the hyperparameters stay fixed, and the expectation is over the not-yet-seen value
    of the sample.

    ``sample_var``: model-space noise variance of the hypothetical sample, a number or one value per point; default the
    likelihood's learned noise (``default_sample_var``).  ``given``: dates or indices of samples to condition on first;
    the gains are then those of one sample MORE (exact for linear targets; for log targets a plug-in that drops the factor
    exp(s^2 R_ij) between already-explained pairs, see ``design``).
    -> Dataset on (``period``, ``time``): ``variance_reduction`` (period, time), ``se_now`` = sqrt Var(L_p), ``mean`` /
    ``lower`` / ``upper`` of the current sums as ``aggregate`` gives them, ``se_given`` (the exact expected standard error
    after the ``given`` samples; = ``se_now`` without them), ``se_expected`` = sqrt max(Var - explained(given) - gain, 0)
    (period, time), ``score`` (time) = sum_p gain / Var_p and ``n_points``.  A record whose dense footprint exceeds
    ``max_bytes`` raises ``ValueError``.

    ``streamed=True`` (never chosen automatically) is the path for such LONG RECORDS: the covariance is produced in row
    panels and never stored -- ``predict``, ``posterior_period_moments`` and one ``posterior_sample_value`` whose work area,
    and with it the panel height, ``max_bytes`` bounds (``ValueError`` naming the bytes when a 128-row panel does not fit);
    ``given`` costs ``posterior_cov_columns`` and ``lowrank_period_moments``, no (M, M) buffer."""
    fit = _prepare(model, covariates, weights, freq, sample_var, max_bytes, extra_buffers=0 if given is None else 1, streamed=streamed)
    picks = _day_indices(fit, given, "given")
    if len(picks) > MAX_ROWS:
        raise ValueError(f"at most {MAX_ROWS} given samples")
    var_now = np.clip(np.diagonal(fit.cov_now), 0.0, None)
    with torch.no_grad():
        rows = conditioning_rows(fit, picks) if len(picks) else None
        explained = np.diagonal(_explained_rows(fit, rows)) if len(picks) else np.zeros(fit.P)
        gain_d, _var = _gain(fit, rows)
    gain = gain_d.cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        score = np.where(var_now[:, None] > 0, gain / var_now[:, None], 0.0).sum(axis=0)
    lower, upper = intervals(fit.mode, fit.mean_now, var_now, ci)
    attrs = _target_attrs(model.dm)
    return Dataset(
        {
            "variance_reduction": (("period", "time"), gain, attrs),
            "se_expected": (("period", "time"), _se(var_now[:, None] - explained[:, None] - gain), attrs),
            "score": ("time", score),
            "mean": ("period", fit.mean_now, attrs),
            "se_now": ("period", _se(var_now), attrs),
            "se_given": ("period", _se(var_now - explained), attrs),
            "lower": ("period", lower, dict(attrs, ci=ci)),
            "upper": ("period", upper, dict(attrs, ci=ci)),
            "n_points": ("period", fit.n_points),
        },
        coords={"period": fit.labels, "time": fit.time},
        attrs=dict(attrs, freq=freq, nterms=fit.nterms),
    )


def _value_dataset(fit, V, extra=None):
    var_now = np.clip(np.diagonal(fit.cov_now), 0.0, None)
    ve = np.diagonal(V)
    with np.errstate(divide="ignore", invalid="ignore"):
        fraction = np.where(var_now > 0, ve / var_now, 0.0)
    attrs = _target_attrs(fit.model.dm)
    data = {
        "variance_explained": ("time", ve, attrs),
        "se_now": ("time", _se(var_now), attrs),
        "se_expected": ("time", _se(var_now - ve), attrs),
        "fraction": ("time", fraction),
        "n_points": ("time", fit.n_points),
    }
    return Dataset(data, coords={"time": fit.labels}, attrs=dict(attrs, freq=fit.freq, **(extra or {})))


def design_value(model, covariates, weights, samples, freq="YE", sample_var=None, return_cov=False,
                 max_bytes: int = DEFAULT_MAX_BYTES, streamed=False):
    """``MarginalHIP.design_value``: the EXACT value V(S) of a given sampling design ``samples`` (dates or indices into
    ``covariates``; a day may repeat: replicate samples): how much of each period sum's variance the samples are expected
    to explain, at fixed hyperparameters, the expectation taken over the not-yet-seen sample values.  The conditioning rows
    are built on the device, R = B^T B goes into a second (M, M) buffer and ``dgp_period_moments`` runs on it.
    -> Dataset on ``time`` (period labels) with ``variance_explained`` = V_pp, ``se_now``, ``se_expected`` =
    sqrt max(Var - V_pp, 0), ``fraction`` = V_pp / Var and ``n_points``; with ``return_cov`` also the (P, P) matrix V.  The
    two (M, M) buffers must fit ``max_bytes``, else ``ValueError`` -- unless ``streamed=True`` (long records; see
    ``sample_value``): the rows come from ``posterior_cov_columns``, V(S) from ``lowrank_period_moments`` on them (at most 64
    samples), and no (M, M) buffer exists."""
    fit = _prepare(model, covariates, weights, freq, sample_var, max_bytes, extra_buffers=1, streamed=streamed)
    picks = _day_indices(fit, samples, "samples")
    if streamed and len(picks) > MAX_ROWS:
        raise ValueError(f"at most {MAX_ROWS} samples with streamed=True")
    with torch.no_grad():
        V = _explained_rows(fit, conditioning_rows(fit, picks))
    ds = _value_dataset(fit, V, {"n_samples": len(picks)})
    return (ds, V) if return_cov else ds


def _objective_weights(fit, objective):
    var_now = np.clip(np.diagonal(fit.cov_now), 0.0, None)
    if isinstance(objective, str) and objective == "relative":
        with np.errstate(divide="ignore"):
            return np.where(var_now > 0, 1.0 / np.where(var_now > 0, var_now, 1.0), 0.0)
    if isinstance(objective, str) and objective == "absolute":
        return np.ones(fit.P)
    try:
        stamp = pd.Timestamp(objective)
    except (ValueError, TypeError):
        raise ValueError(f"objective must be 'relative', 'absolute' or a period label, not {objective!r}") from None
    hit = np.nonzero(pd.DatetimeIndex(fit.labels) == stamp)[0]
    if not len(hit):
        raise ValueError(f"objective: {stamp.date()} is none of the period labels")
    return (np.arange(fit.P) == hit[0]).astype(np.float64)


def design(model, covariates, weights, k, objective="relative", candidates=None, replicates=False, given=None, freq="YE",
           sample_var=None, max_bytes: int = DEFAULT_MAX_BYTES, streamed=False):
    """``MarginalHIP.design``: GREEDY choice of ``k`` days to sample.  Each step runs ``dgp_sample_value`` with the rows of
    the samples so far, scores every day by sum_p omega_p gain[p, c] -- omega_p = 1 / Var_p (``objective="relative"``), 1
    (``"absolute"``) or one period's label alone --, masks the days outside ``candidates`` (a boolean mask, dates or
    indices; default every day) and, unless ``replicates``, the days already taken (``given`` included), takes the
    largest score (ties: the earliest day of the period-sorted record) and appends its conditioning row.

    The selection is exact for linear targets.  For log targets it is exact for the first pick; after that the score is a
    PLUG-IN approximation of the marginal gain: it drops the factor exp(s^2 R_ij) between already-explained pairs (0.988 to
    1.000 of the exact marginal gain in the numpy check that came with the formulas).  The REPORTED value of the chosen design is always
    exact: ``variance_explained`` / ``se_expected`` of every nested prefix come from ``design_value``'s path.  "Expected"
    means: hyperparameters held fixed, the expectation taken over the not-yet-seen sample values.
    -> Dataset on (``pick``, ``period``): ``time`` and ``index`` (into ``covariates``) of each pick, its ``score``,
    ``variance_explained`` and ``se_expected`` (pick, period) of the design ``given`` + picks[: j + 1], ``se_now`` (period).
    ``given`` plus ``k`` may not exceed 64 samples; ``k`` larger than the number of candidates raises ``ValueError``.
    ``streamed=True``: the long-record path of ``sample_value`` -- one ``posterior_sample_value`` per step, each pick's column
    from ``posterior_cov_columns``, every prefix's value from ``lowrank_period_moments``; no (M, M) buffer."""
    k = int(k)
    fit = _prepare(model, covariates, weights, freq, sample_var, max_bytes, extra_buffers=1, streamed=streamed)
    taken = _day_indices(fit, given, "given")
    if k < 1 or len(taken) + k > MAX_ROWS:
        raise ValueError(f"k must be at least 1 and given + k at most {MAX_ROWS} samples")
    allowed = np.ones(fit.m, dtype=bool)
    if candidates is not None:
        cand = np.asarray(candidates)
        if cand.dtype == bool:
            if cand.shape != (fit.m_all,):
                raise ValueError(f"a candidate mask must have shape ({fit.m_all},)")
            allowed = cand[fit.order]
        else:
            allowed = np.zeros(fit.m, dtype=bool)
            allowed[_day_indices(fit, cand, "candidates")] = True
    if not replicates:
        allowed[taken] = False
    if (k > int(allowed.sum())) if not replicates else not allowed.any():
        raise ValueError(f"k = {k} exceeds the {int(allowed.sum())} candidate days")
    omega = torch.as_tensor(_objective_weights(fit, objective), dtype=torch.float64, device=fit.dev)
    allowed_t = torch.as_tensor(allowed, device=fit.dev)
    picks, scores, values = [], [], []
    with torch.no_grad():
        rows = torch.zeros(len(taken) + k, fit.m, dtype=torch.float64, device=fit.dev)
        rows[: len(taken)] = conditioning_rows(fit, taken)
        n = len(taken)
        # dense: R kept up to date by rank-one updates, one (M, M) buffer for every prefix; streamed: the rows themselves
        R = None if streamed else _explained_cov(fit, rows[:n])
        for _step in range(k):
            gain, var = _gain(fit, rows[:n] if n else None)
            score = torch.where(allowed_t, omega @ gain, torch.full_like(var, -float("inf")))
            if bool(torch.isnan(score).any()):
                day = int(torch.nonzero(torch.isnan(score))[0])
                raise ValueError(f"design: the score of {pd.Timestamp(fit.time[day]).date()} (point {int(fit.order[day])}) is NaN: "
                                 "the posterior covariance or the weights hold a NaN")
            c = int(torch.nonzero(score == score.max())[0])  # ties: the lowest index
            rows[n] = _next_row(fit, rows[:n], c, var=var[c])
            if not streamed:
                R[: fit.m, : fit.m].addr_(rows[n], rows[n])
            n += 1
            picks.append(c)
            scores.append(float(score[c]))
            if not replicates:
                allowed_t[c] = False
            values.append(np.diagonal(_explained_rows(fit, rows[:n]) if streamed else _explained(fit, R)).copy())
    picks = np.asarray(picks, dtype=np.int64)
    var_now = np.clip(np.diagonal(fit.cov_now), 0.0, None)
    ve = np.stack(values)
    attrs = _target_attrs(model.dm)
    return Dataset(
        {
            "time": ("pick", fit.time[picks]),
            "index": ("pick", fit.order[picks]),
            "score": ("pick", np.asarray(scores)),
            "variance_explained": (("pick", "period"), ve, attrs),
            "se_expected": (("pick", "period"), _se(var_now[None, :] - ve), attrs),
            "se_now": ("period", _se(var_now), attrs),
            "n_points": ("period", fit.n_points),
        },
        coords={"pick": np.arange(k), "period": fit.labels},
        attrs=dict(attrs, freq=freq, objective=str(objective), nterms=fit.nterms, n_given=len(taken)),
    )


__all__ = ["sample_value", "design_value", "design", "conditioning_rows", "default_sample_var", "MAX_ROWS"]
