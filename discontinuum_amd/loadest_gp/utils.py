"""Load helpers of loadest-gp (``src/loadest_gp/utils.py``); the plotting helpers stay with the reference."""
from __future__ import annotations

from warnings import warn

import numpy as np

from ..xr_compat import DataArray


def _broadcast(values, dims, to_dims):
    """``values`` with dimensions ``dims`` laid out along ``to_dims`` (size-1 axes where it has none) -- the by-name
    broadcast xarray applies to ``concentration * flow``."""
    missing = [d for d in dims if d not in to_dims]
    if missing:
        raise ValueError(f"flow has dimensions {missing} that concentration lacks")
    values = np.transpose(np.asarray(values), [dims.index(d) for d in to_dims if d in dims])
    return values.reshape([values.shape[[d for d in to_dims if d in dims].index(d)] if d in dims else 1 for d in to_dims])


def concentration_to_flux(concentration, flow):
    """Convert concentration (mg/l) to flux (kg): concentration x flow (m^3/s) x time step (s) x 1e-3, with the
    reference's warnings and attributes (src/loadest_gp/utils.py:14-56).  ``concentration`` may carry a ``draw``
    dimension (``model.sample(daily, n)``); ``flow`` broadcasts against it by dimension name."""
    time = np.asarray(concentration.coords["time"].values).astype("datetime64[ns]")
    time_delta = np.unique(np.diff(time).astype("timedelta64[ns]").astype(np.int64) / 1e9)
    mg_l_to_kg_m3 = 1e-3

    if len(time_delta) != 1:
        warn("Time delta is not constant", UserWarning, stacklevel=2)

    if flow.attrs.get("units") != "cubic meters per second":
        warn(
            "Check that flow is 'cubic meters per second'. Set flow.units = 'cubic meters per second' to silence.",
            UserWarning,
            stacklevel=2,
        )

    if "mg/l" not in str(concentration.attrs.get("units", "")):
        warn(
            "Check that concentration is in 'mg/l'. Set concentration.units = 'mg/l' to silence.",
            UserWarning,
            stacklevel=2,
        )

    dims = tuple(concentration.dims)
    q = _broadcast(flow.values, tuple(flow.dims), dims)
    values = np.asarray(concentration.values) * q * time_delta * mg_l_to_kg_m3
    attrs = dict(concentration.attrs)
    attrs["units"] = "kilograms"
    attrs["standard_name"] = "flux"
    coords = {k: np.asarray(v.values) for k, v in concentration.coords.items()}
    return DataArray(values, coords=coords, dims=dims, attrs=attrs, name=concentration.name)
