"""loadest-gp (concentration from time and streamflow) on the MI355X engine.

The model is the reference's (``src/loadest_gp/models/gpytorch.py:24-128``): constant mean, fixed observation noise
0.1^2 in model space, and a covariance of three scaled terms over the design-matrix columns (time first):

    seasonal    sigma^2 * Periodic(t) * Matern52(t)          sigma^2 ~ HalfNormal(1),   period ~ N(1, 0.01)
    covariates  sigma^2 * RBF_ARD(x_1 .. x_{d-1})            sigma^2 ~ HalfNormal(2),   l ~ Gamma(2, 3)
    residual    sigma^2 * Matern32_ARD(t, x_1 .. x_{d-1})    sigma^2 ~ HalfNormal(0.2), l ~ Gamma(2, 10)

The module tree (and so every ``state_dict`` key) is the reference's: ``covar_module`` is the sum of three
``ScaleKernel``s in that order, which is also what ``gp.lowering`` recognises and maps onto the fused device kernel.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import gp
from ..engines.base import DataMixin, ModelConfig, is_fitted
from ..engines.hip import MarginalHIP
from ..gp import kernels as K
from ..gp.priors import GammaPrior, HalfNormalPrior, NormalPrior
from ..pipeline import LogStandardPipeline, TimePipeline

MODEL_SPACE_NOISE = 0.1 ** 2  # fixed observation variance (gpytorch.py:51-54)


def censoring_from_bounds(low, high):
    """A record of (low, high) pairs -- EGRET's ``ConcLow`` / ``ConcHigh``: the truth of sample i lies in [low_i, high_i] --
    as the three arguments of ``LoadestGP.fit``: -> (target, censored, target_upper).  Per row:

        low missing (NaN) or <= 0          censored -1 at high   (a non-detect: "< high")
        high missing (NaN) or infinite     censored +1 at low    ("> low")
        low == high                        observed
        otherwise                          censored 2, target = low, target_upper = high   (the truth lies in the bracket)

    ``target`` has the type of ``high`` (a labelled array keeps its dims, coords, name and attrs; anything else gives a
    numpy array); ``censored`` is an int32 array and ``target_upper`` a float64 array that is NaN off the bracketed rows
    (None when there is no bracketed row).  A row with both ends missing, or with low > high, is an error."""
    lo = np.asarray(getattr(low, "values", low), dtype=np.float64).reshape(-1)
    hi = np.asarray(getattr(high, "values", high), dtype=np.float64).reshape(-1)
    if lo.shape != hi.shape:
        raise ValueError(f"low and high must align: {lo.shape} against {hi.shape}")
    below = np.isnan(lo) | (lo <= 0.0)
    above = np.isnan(hi) | np.isposinf(hi)
    if np.any(below & above):
        raise ValueError("a row has neither a lower nor an upper bound")
    both = ~below & ~above
    if np.any(both & (lo > hi)):
        raise ValueError("a row has low > high")
    bracket = both & (lo < hi)
    censored = np.where(below, -1, np.where(above, 1, np.where(bracket, 2, 0))).astype(np.int32)
    values = np.where(below, hi, lo)
    upper = np.where(bracket, hi, np.nan) if bracket.any() else None
    template = high if hasattr(high, "dims") else (low if hasattr(low, "dims") else None)
    if template is not None:
        values = type(template)(values, dims=template.dims, coords=template.coords, name=template.name, attrs=template.attrs)
    return values, censored, upper


def loadest_covariance(n_columns: int):
    """seasonal + covariates + residual for a design matrix with ``n_columns`` columns, time in column 0."""
    time, others, everything = [0], list(range(1, n_columns)), list(range(n_columns))
    seasonal = K.ScaleKernel(
        K.PeriodicKernel(active_dims=time, period_length_prior=NormalPrior(loc=1, scale=0.01))
        * K.MaternKernel(nu=2.5, active_dims=time),
        outputscale_prior=HalfNormalPrior(scale=1))
    covariates = K.ScaleKernel(
        K.RBFKernel(active_dims=others, ard_num_dims=len(others), lengthscale_prior=GammaPrior(concentration=2, rate=3)),
        outputscale_prior=HalfNormalPrior(scale=2))
    residual = K.ScaleKernel(
        K.MaternKernel(nu=1.5, active_dims=everything, ard_num_dims=n_columns,
                       lengthscale_prior=GammaPrior(concentration=2, rate=10)),
        outputscale_prior=HalfNormalPrior(scale=0.2))
    return seasonal + covariates + residual


class ExactGPModel(gp.ExactGP):
    def __init__(self, train_x, train_y, likelihood):
        super().__init__(train_x, train_y, likelihood)
        self.mean_module = gp.means.ConstantMean()
        self.covar_module = loadest_covariance(train_x.shape[1])


class LoadestDataMixin(DataMixin):
    """Design matrix columns (time, flow) -- ``src/loadest_gp/models/base.py:14-17``."""

    def build_datamanager(self, model_config: ModelConfig | None = None):
        self._build_datamanager({"time": TimePipeline, "flow": LogStandardPipeline}, model_config)


class LoadestGPMarginalHIP(LoadestDataMixin, MarginalHIP):
    """LOAD ESTimation as an exact GP (marginal likelihood) on the MI355X engine.  The reference class also mixes in
    its plotting helpers; they sit outside the hot path and would compose in the same MRO slot, before the engine."""

    component_names = ("seasonal", "covariates", "residual")  # the covariance's additive parts, in ``decompose``'s order

    def __init__(self, model_config: ModelConfig | None = None):
        config = model_config or ModelConfig()
        super().__init__(model_config=config)
        self.build_datamanager(config)

    def build_model(self, X, y):
        fixed = torch.full((1, y.shape[0]), MODEL_SPACE_NOISE, dtype=y.dtype)
        self.likelihood = gp.likelihoods.FixedNoiseGaussianLikelihood(noise=fixed, learn_additional_noise=False)
        return ExactGPModel(X, y, self.likelihood)

    @is_fitted
    def annual_flux(self, covariates, freq="YE", ci=0.95, pred_noise=False, return_cov=False, max_bytes=None,
                    hyperparameters=False, prior=True, interval="lognormal"):
        """Exact period loads in kilograms -- sum over each period of concentration (mg/l) x flow (m^3/s) x time step --
        with their standard errors and approximate ``ci`` intervals; ``covariates`` on a regular time grid (an irregular
        one raises ``ValueError``), ``freq`` a resample alias ("YE", "YE-SEP" for water years, "QE", "ME").  Replaces
        ``concentration_to_flux(model.sample(daily, n), daily["flow"]).resample(time="YE").sum()``
        (src/loadest_gp/utils.py:14-103) without its sampling noise; see ``MarginalHIP.aggregate`` (also for
        ``max_bytes``, and for ``hyperparameters=True``: ``se_hyper`` / ``se_total`` with the hyperparameters' uncertainty
        propagated to first order, and for ``interval="three-moment"``: the loads' exact ``skewness`` and intervals fitted
        to three exact moments)."""
        from ..loads import DEFAULT_MAX_BYTES, annual_flux

        return annual_flux(self, covariates, freq=freq, ci=ci, pred_noise=pred_noise, return_cov=return_cov,
                           max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes, hyperparameters=hyperparameters,
                           prior=prior, interval=interval)

    @is_fitted
    def exceedance(self, covariates, threshold=None, threshold_series=None, kind="concentration", freq="YE", above=True,
                   fraction=False, ci=0.95, pred_noise=False, return_cov=False, max_bytes=None, streamed=False, window=None,
                   align="right", min_periods=None, statistic=None):
        """Days per period above a criterion, with exact uncertainty (``MarginalHIP.exceedance``).  ``kind="concentration"``:
        the threshold is a concentration; ``kind="flux"``: ``threshold`` is a daily load in kg per day (a number or a list),
        turned into the per-day concentration threshold limit / w_i with the flux weights of ``annual_flux`` (regular time
        grid; a day with a non-positive or missing flow is excluded).  ``window`` (``kind="concentration"`` only): days on
        which the rolling geometric mean over that averaging period exceeds the criterion (``MarginalHIP.exceedance``)."""
        if kind not in ("concentration", "flux"):
            raise ValueError(f"kind must be 'concentration' or 'flux', not {kind!r}")
        if kind == "concentration":
            return super().exceedance(covariates, threshold=threshold, threshold_series=threshold_series, freq=freq, above=above,
                                      fraction=fraction, ci=ci, pred_noise=pred_noise, return_cov=return_cov, max_bytes=max_bytes,
                                      streamed=streamed, window=window, align=align, min_periods=min_periods, statistic=statistic)
        if window is not None:
            from ..exceedance import WINDOW_REFUSALS

            raise NotImplementedError(WINDOW_REFUSALS["flux"])
        if threshold is None or threshold_series is not None:
            raise ValueError("kind='flux' takes threshold = the daily load limit in kg per day")
        from ..exceedance import flux_exceedance
        from ..loads import DEFAULT_MAX_BYTES

        return flux_exceedance(self, covariates, threshold, freq=freq, above=above, fraction=fraction, ci=ci, pred_noise=pred_noise,
                               return_cov=return_cov, max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes,
                               streamed=streamed)

    @is_fitted
    def excess_load(self, daily, criterion=None, limit=None, freq="YE", above=True, ci=0.95, pred_noise=False, return_cov=False,
                    max_bytes=None, streamed=False):
        """The mass per period (kg) carried ABOVE an allowable load -- the load reduction a TMDL asks for -- with its exact
        standard error.  Exactly one of ``criterion`` (a concentration, mg/l: the allowable load of a day is criterion x
        flow) and ``limit`` (kg per day); each a number, a list of levels or a per-day series.  ``above=False``: the mass by
        which the load stays below it.  ``max_bytes`` / ``streamed``: as for ``MarginalHIP.excess``.  See
        ``discontinuum_amd.excess.excess_load``."""
        from ..excess import excess_load
        from ..loads import DEFAULT_MAX_BYTES

        return excess_load(self, daily, criterion=criterion, limit=limit, freq=freq, above=above, ci=ci, pred_noise=pred_noise,
                           return_cov=return_cov, max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes,
                           streamed=streamed)

    def _flux_weights(self, daily):
        from ..loads import _target_attrs, flux_weights

        return flux_weights(daily, _target_attrs(self.dm))

    @is_fitted
    def sample_value(self, daily, freq="YE", sample_var=None, given=None, ci=0.95, max_bytes=None, streamed=False):
        """By how much one more concentration sample on each day of ``daily`` is expected to reduce the variance of each
        period's LOAD (kg; the flux weights of ``annual_flux``): ``MarginalHIP.sample_value``."""
        return super().sample_value(daily, self._flux_weights(daily), freq=freq, sample_var=sample_var, given=given, ci=ci,
                                    max_bytes=max_bytes, streamed=streamed)

    @is_fitted
    def sample_influence(self, daily, folds="loo", freq="YE", max_bytes=None):
        """What the samples in hand were worth: the exact change of every period's LOAD (kg; the flux weights of
        ``annual_flux``) had each fold of observations not been sampled -- ``MarginalHIP.influence``, named to mirror
        ``sample_value``."""
        self._refuse_censored("sample_influence")
        return super().influence(daily, self._flux_weights(daily), folds=folds, freq=freq, max_bytes=max_bytes)

    @is_fitted
    def design_value(self, daily, samples, freq="YE", sample_var=None, return_cov=False, max_bytes=None, streamed=False):
        """The exact expected value of sampling the days ``samples`` for the period loads (kg): ``MarginalHIP.design_value``."""
        return super().design_value(daily, self._flux_weights(daily), samples, freq=freq, sample_var=sample_var,
                                    return_cov=return_cov, max_bytes=max_bytes, streamed=streamed)

    @is_fitted
    def design(self, daily, k, objective="relative", candidates=None, replicates=False, given=None, freq="YE", sample_var=None,
               max_bytes=None, streamed=False):
        """Greedy choice of ``k`` sampling days for the period loads (kg): ``MarginalHIP.design``."""
        return super().design(daily, self._flux_weights(daily), k, objective=objective, candidates=candidates,
                              replicates=replicates, given=given, freq=freq, sample_var=sample_var, max_bytes=max_bytes,
                              streamed=streamed)

    @is_fitted
    def flux_bias(self, cv=None, folds="loo", laplace=None):
        """WRTDS's flux bias statistic on the sampled days, (sum P - sum O) / sum P with O the observed and P the
        cross-validated mean concentration x flow; ``cv``: a Dataset from ``cross_validate`` (default: run it with
        ``folds``).  A fit with censored observations needs ``laplace="cavity"`` (approximate; O of a censored row is then
        the expected concentration inside its bracket).  See ``discontinuum_amd.validation.flux_bias``."""
        from ..validation import flux_bias

        return flux_bias(self, cv=cv, folds=folds, laplace=laplace)

    def flow_normalized_flux(self, daily, freq="YE", flow_window=None, ci=0.95, pred_noise=False, return_cov=False,
                             max_bytes=None):
        """Flow-normalized period loads (kg) with exact uncertainty -- WRTDS's FN flux: each day's load averaged over
        every flow seen on its calendar day in the record (or in ``flow_window``, an inclusive (start, end) pair).
        ``daily`` on a daily grid; see ``loads.flow_normalized`` and, for trends, ``loads.period_change``."""
        from ..loads import DEFAULT_MAX_BYTES, flow_normalized

        return flow_normalized(self, daily, kind="flux", freq=freq, flow_window=flow_window, ci=ci, pred_noise=pred_noise,
                               return_cov=return_cov, max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes)

    def flow_normalized_concentration(self, daily, freq="YE", flow_window=None, ci=0.95, pred_noise=False,
                                      return_cov=False, max_bytes=None):
        """Flow-normalized period mean concentration (the target's units) with exact uncertainty; see
        ``flow_normalized_flux``."""
        from ..loads import DEFAULT_MAX_BYTES, flow_normalized

        return flow_normalized(self, daily, kind="concentration", freq=freq, flow_window=flow_window, ci=ci,
                               pred_noise=pred_noise, return_cov=return_cov,
                               max_bytes=DEFAULT_MAX_BYTES if max_bytes is None else max_bytes)

