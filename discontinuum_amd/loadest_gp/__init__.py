"""LOADEST-GP on the MI355X engine (counterpart of ``src/loadest_gp/__init__.py``)."""
from ..loads import annual_flux_many  # noqa: F401
from .models import LoadestGPMarginalHIP, censoring_from_bounds  # noqa: F401
from .utils import concentration_to_flux  # noqa: F401

LoadestGP = LoadestGPMarginalHIP
