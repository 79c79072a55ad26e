"""Exceedance-count distributions of a fitted model's posterior: P(N <= k) for the number N of a period's points on the wrong
side of a criterion, and P(R <= r) for the longest spell R of consecutive such points -- the frequency rules water-quality
criteria are written as ("no more than one exceedance in the period", "no more than 10 % of days", "not more than k
consecutive days below the limit").

``exceedance`` gives the exact mean and variance of N and guesses the shape from them; ``extreme_probability`` gives P(N = 0).
The distribution of N, and anything about runs, has neither a closed form nor a separation of variables: joint paths of the
period's block of the latent posterior are drawn, compared and counted on the device (``dgp_path_counts``,
csrc/dgp_counts.hip), over the randomly shifted quasi-Monte-Carlo rules of the orthant sweep.  The device returns two INTEGER
histograms per (level, shift); every floating-point step after that is this module's.

Like the period extremes this product is NOT EXACT.  It is unbiased and carries its own standard errors: every functional
(a value of the distribution function, the mean, the variance) is formed per shift, and its error is the sample standard
deviation over the ``nshifts`` independently shifted rules divided by sqrt(nshifts).  Everything before the draws -- the
covariance, the threshold's exact monotone map to model space, the window's W C W^T, the float64 factors of the periods'
blocks -- is what ``extremes._Periods`` prepares, as exact as there; censored and EP fits hold an ordinary latent posterior
(Gaussian BY APPROXIMATION) and take the same path.

Spells are runs of consecutive points WITHIN a period: a spell that crosses a period boundary is cut there and counted as two.
A gap in the record also breaks a spell: point i continues the run of the kept point before it only if the time step between
them is at most 1.5 times the record's median step.
"""
from __future__ import annotations

import numpy as np

from . import extremes as X
from .backend import MODE_LOG
from .exceedance import model_space_threshold
from .loads import DEFAULT_MAX_BYTES, target_transform
from .xr_compat import Dataset

LINK_FACTOR = 1.5  # a step of more than this many median steps breaks a spell

REFUSALS = {
    "streamed": X.REFUSALS["streamed"],
    "pred_noise": "pred_noise=True is not implemented for exceedance-count distributions: the counts of hypothetical noisy "
                  "observations are not the counts of the target",
    "flux": "kind='flux' is not implemented for exceedance-count distributions: a daily load has a different threshold on every "
            "day; pass the per-day concentration thresholds as threshold_series",
    "statistic": "counts of the arithmetic rolling mean of a log target are not implemented: that mean is a sum of "
                 "lognormals, not a Gaussian; use the model-space statistic (the geometric mean)",
}


def _check_request(model, kind, pred_noise, streamed, window, statistic):
    """The refusals of a count distribution, each saying why; -> nothing."""
    if kind == "flux":
        raise NotImplementedError(REFUSALS["flux"])
    if kind is not None:
        raise ValueError(f"kind must be None (the target itself) here, not {kind!r}; the side is chosen with above=")
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


def spell_links(time):
    """``link`` flags of points in the order given: ``link[i]`` = the step from point i - 1 to point i is positive and at most
    ``LINK_FACTOR`` times the median step of the whole (sorted, finite, distinct) record; ``link[0]`` = 0.  -> (flags int32,
    the median step as an integer of the record's time unit).  The caller cuts the flags at period boundaries by slicing."""
    t = np.asarray(time).reshape(-1).astype("datetime64[ns]").astype(np.int64)
    link = np.zeros(t.size, dtype=np.int32)
    steps = np.diff(np.unique(t))
    if steps.size == 0:
        return link, 0
    med = float(np.median(steps))
    d = np.diff(t)
    link[1:] = (d > 0) & (d <= LINK_FACTOR * med)
    return link, med


def histogram_statistics(hist, n_p, npoints):
    """The host half of the estimator for ONE (level, period): ``hist`` (nshifts, >= n_p + 1) integer histogram of a count in
    0 .. n_p over ``npoints`` points per shift.  Every functional is formed per shift; its value is the mean over the shifts and
    its error their sample standard deviation / sqrt(nshifts).  The variance is taken about the pooled mean, so that the mean of
    the shifts' values IS the variance of the pooled pmf.
    -> dict: ``pmf``, ``cdf``, ``cdf_error`` (n_p + 1,), ``mean``, ``mean_error``, ``variance``, ``variance_error``."""
    h = np.asarray(hist, dtype=np.float64)[:, :n_p + 1] / float(npoints)
    S = h.shape[0]
    k = np.arange(n_p + 1, dtype=np.float64)
    err = lambda v: v.std(axis=0, ddof=1) / np.sqrt(S)  # noqa: E731
    cdf_s = np.cumsum(h, axis=1)
    mean_s = h @ k
    mean = mean_s.mean()
    var_s = h @ (k - mean) ** 2
    cdf = cdf_s.mean(axis=0)
    cdf[-1] = 1.0  # every path has a count in 0 .. n_p: the integers say so exactly
    return dict(pmf=h.mean(axis=0), cdf=cdf, cdf_error=err(cdf_s), mean=mean, mean_error=err(mean_s), variance=var_s.mean(),
                variance_error=err(var_s))


def _sweep(periods, time, u, above, npoints, nshifts, seed):
    """Model-space thresholds ``u`` (L, kept outputs) -> per non-empty period (g, n_p, count_hist, spell_hist), the histograms
    (L, nshifts, n_p + 1) int32 numpy arrays."""
    u = np.asarray(u, dtype=np.float64)
    link_all, _med = spell_links(np.asarray(time)[periods.order])
    out = []
    for g, idx, Lbuf in periods.blocks:
        c = u[:, idx] - periods.mu[idx][None, :]
        link = link_all[idx].copy()
        link[1:] &= (np.diff(idx) == 1).astype(np.int32)  # a kept output between them that does not qualify breaks the run too
        link[0] = 0
        ch, sh = periods.plan.path_counts(Lbuf, int(idx.size), c, above=above, link=link, npoints=npoints, nshifts=nshifts, seed=seed,
                                          max_bytes=periods.sweep_bytes)
        out.append((g, int(idx.size), ch.cpu().numpy(), sh.cpu().numpy()))
    return out


def _attrs(model, above, window, align, npoints, nshifts, seed, jitter):
    attrs = X._attrs(model, "count", window, align, npoints, nshifts, seed, jitter)
    del attrs["kind"]
    attrs["above"] = bool(above)
    return attrs


def exceedance_distribution(model, covariates, threshold=None, threshold_series=None, freq="YE", above=True, window=None,
                            align="right", min_periods=None, npoints=4096, nshifts=16, seed=0, max_bytes: int = DEFAULT_MAX_BYTES,
                            pred_noise=False, streamed=False, kind=None, statistic=None):
    """``MarginalHIP.exceedance_distribution``: per period of ``freq`` the DISTRIBUTION of the number N of points at which the
    target lies above (``above=False``: below) a data-space threshold, and of the longest spell R of consecutive such points.

    ``threshold`` / ``threshold_series``, the exact map to model space, the periods and the dropped points: as for
    ``exceedance``.  ``window`` (with ``align``, ``min_periods``): the counts of the ROLLING mean over that window (the geometric
    mean for a log target).  ``npoints`` x ``nshifts`` joint paths per period, one sweep for all levels.
    -> Dataset; on (``level``, ``time``, ``count``), ``count`` = 0 .. the longest period's points: ``pmf``, ``cdf`` = P(N <= count),
    ``cdf_error``, ``spell_pmf``, ``spell_cdf`` = P(R <= count), ``spell_cdf_error``; on (``level``, ``time``): ``mean``,
    ``mean_error``, ``variance``, ``variance_error``; on ``time``: ``n_points``.  Entries with ``count`` beyond the points of their
    period are NaN, and so is an empty period.  The errors are standard errors of the estimate (NOT exact: see the module's
    text); the attrs carry ``npoints``, ``nshifts``, ``seed``, ``jitter``, ``above``, ``exact=False`` and, with a window, the
    window attrs of ``extreme_probability``.
    Spells are cut at period boundaries (a spell across New Year counts as two) and at gaps of the record: a point continues
    the run of the kept point before it only if their time step is at most 1.5 median steps of the record.
    Refused, each with its reason: ``streamed=True`` and a record whose dense footprint exceeds ``max_bytes``,
    ``pred_noise=True``, ``kind="flux"``, the arithmetic ``statistic="mean"`` of a log target, a period of more than
    ``backend.ORTHANT_MAX_DIM`` points."""
    _check_request(model, kind, pred_noise, streamed, window, statistic)
    time = np.asarray(covariates.coords["time"].values).reshape(-1)
    levels, series = X._threshold_rows(threshold, threshold_series, len(time))
    periods = X._Periods(model, covariates, freq, window, align, min_periods, max_bytes)
    u = model_space_threshold(model.dm, series[:, periods.order])
    L, P = len(levels), len(periods.labels)
    K = int(periods.n_points.max()) + 1 if P else 1
    big = {k: np.full((L, P, K), np.nan) for k in ("pmf", "cdf", "cdf_error", "spell_pmf", "spell_cdf", "spell_cdf_error")}
    flat = {k: np.full((L, P), np.nan) for k in ("mean", "mean_error", "variance", "variance_error")}
    for g, n_p, ch, sh in _sweep(periods, time, u, above, npoints, nshifts, seed):
        for l in range(L):
            st, sp = histogram_statistics(ch[l], n_p, npoints), histogram_statistics(sh[l], n_p, npoints)
            for k in ("pmf", "cdf", "cdf_error"):
                big[k][l, g, :n_p + 1] = st[k]
                big["spell_" + k][l, g, :n_p + 1] = sp[k]
            for k in flat:
                flat[k][l, g] = st[k]
    attrs = _attrs(model, above, window, align, npoints, nshifts, seed, periods.jitter)
    data = {k: (("level", "time", "count"), v, attrs) for k, v in big.items()}
    data.update({k: (("level", "time"), v, attrs) for k, v in flat.items()})
    data["n_points"] = ("time", periods.n_points)
    return Dataset(data, coords={"level": levels, "time": periods.labels, "count": np.arange(K)}, attrs=dict(attrs, freq=freq))


def _allowed_counts(n_points, allowed, allowed_fraction):
    """The allowed count of every period from exactly one of a count and a fraction of the period's points (rounded down)."""
    if (allowed is None) == (allowed_fraction is None):
        raise ValueError("give exactly one of allowed and allowed_fraction")
    n = np.asarray(n_points, dtype=np.int64)
    if allowed is not None:
        if isinstance(allowed, (bool, np.bool_)) or int(allowed) != allowed or int(allowed) < 0:
            raise ValueError(f"allowed must be a whole number of points >= 0, not {allowed!r}")
        return np.full(n.shape, int(allowed), dtype=np.int64)
    f = float(allowed_fraction)
    if not 0.0 <= f <= 1.0:
        raise ValueError(f"allowed_fraction must lie in [0, 1], not {allowed_fraction!r}")
    return np.floor(f * n + 1e-9).astype(np.int64)  # (0.1 x 30 is 3, not 2: the product's rounding must not cost a day)


def compliance_probability(model, covariates, threshold=None, threshold_series=None, allowed=None, allowed_fraction=None,
                           max_spell=None, **kw):
    """``MarginalHIP.compliance_probability``: per period the probability that a frequency rule is met -- ``prob`` =
    P(N <= ``allowed``), or P(N <= floor(``allowed_fraction`` x the period's points)); with ``max_spell`` also ``prob_spell`` =
    P(R <= ``max_spell``).  Exactly one of ``allowed`` / ``allowed_fraction``; every other argument, the refusals and the
    caveats (NOT exact; spells cut at period boundaries and gaps) are ``exceedance_distribution``'s, whose sweep this reads.
    -> Dataset on (``level``, ``time``) with ``prob``, ``error``, (``prob_spell``, ``error_spell``), and on ``time``
    ``allowed_count`` and ``n_points``.  An empty period holds NaN."""
    _allowed_counts([1], allowed, allowed_fraction)  # the argument checks, before any device work
    if max_spell is not None and (isinstance(max_spell, (bool, np.bool_)) or int(max_spell) != max_spell or int(max_spell) < 0):
        raise ValueError(f"max_spell must be a whole number of points >= 0, not {max_spell!r}")
    ds = exceedance_distribution(model, covariates, threshold=threshold, threshold_series=threshold_series, **kw)
    n_points = np.asarray(ds["n_points"].values)
    count = _allowed_counts(n_points, allowed, allowed_fraction)

    def at(name, k):  # the distribution function at the periods' own counts; at or beyond n_p it is 1 exactly
        v = np.asarray(ds[name].values)
        kk = np.minimum(np.minimum(k, n_points), v.shape[2] - 1)
        out = np.take_along_axis(v, np.broadcast_to(kk[None, :, None], v.shape[:2] + (1,)), axis=2)[:, :, 0]
        return np.where((n_points == 0)[None, :], np.nan, out)

    attrs = dict(ds.attrs)
    if allowed is not None:
        attrs["allowed"] = int(allowed)
    else:
        attrs["allowed_fraction"] = float(allowed_fraction)
    dims = ("level", "time")
    data = {"prob": (dims, at("cdf", count), attrs), "error": (dims, at("cdf_error", count), attrs)}
    if max_spell is not None:
        attrs["max_spell"] = int(max_spell)
        spell = np.full(n_points.shape, int(max_spell), dtype=np.int64)
        data.update({"prob_spell": (dims, at("spell_cdf", spell), attrs), "error_spell": (dims, at("spell_cdf_error", spell), attrs)})
    data.update({"allowed_count": ("time", count), "n_points": ("time", n_points)})
    return Dataset(data, coords={"level": ds.coords["level"].values, "time": ds.coords["time"].values}, attrs=attrs)


__all__ = ["exceedance_distribution", "compliance_probability", "histogram_statistics", "spell_links", "REFUSALS", "LINK_FACTOR"]
