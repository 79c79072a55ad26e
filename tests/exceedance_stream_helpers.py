"""The oracle-backed plan double of the streamed exceedance tests (tests/test_exceedance_stream_cpu.py):
``posterior_exceedance_moments`` answered densely -- the oracle's posterior covariance and
``exceedance_helpers.dense_exceedance_moments`` -- with the panel choice of ``GPPlan.posterior_exceedance_moments``
(``backend.stream_panel_rows`` on the work area's bytes).  Pure numpy / scipy / torch on the CPU."""
from __future__ import annotations

import torch

from discontinuum_amd import backend
from discontinuum_amd.exceedance import _work_bytes
from discontinuum_amd.loads import DEFAULT_MAX_BYTES
from oracle import gp_oracle as orc
from tests.exceedance_helpers import ExceedOraclePlan, dense_exceedance_moments


def stream_bytes(n, m, d, P, L, esz, panel_rows):
    """The host's copy of ``dgp_posterior_exceedance_moments_workspace_bytes`` for one site: the prediction's (coordinates, cross Gram, V,
    three vectors, 64 rows of partial sums), the covariance panel of min(panel_rows, M) x M elements, and ``_work_bytes``."""
    N, M = -(-n // 128) * 128, -(-m // 128) * 128
    up = lambda b: -(-b // 256) * 256  # noqa: E731
    return (up(esz * M * d) + 2 * up(esz * N * M) + 3 * up(esz * M) + up(esz * 64 * M) + up(esz * min(panel_rows, M) * M)
            + _work_bytes(m, P, L))


class StreamOraclePlan(ExceedOraclePlan):
    """``ExceedOraclePlan`` with ``posterior_exceedance_moments`` by the dense reference (unbatched).  Every call of the
    streamed and of the dense entry is appended to the class lists ``streamed_calls`` / ``dense_calls``."""

    streamed_calls: list = []
    dense_calls: list = []

    def exceedance_moments(self, cov, m, mu, thresh, w, groups, ngroups, extra_var=None):
        StreamOraclePlan.dense_calls.append(dict(m=m, levels=int(torch.as_tensor(thresh).shape[0])))
        return super().exceedance_moments(cov, m, mu, thresh, w, groups, ngroups, extra_var)

    def exceedance_panel_rows(self, m, ngroups, nlevels, max_bytes=None):
        M = -(-m // 128) * 128
        esz = torch.empty((), dtype=self.dtype).element_size()
        size = lambda R: stream_bytes(self.n, m, self.d, int(ngroups), int(nlevels), esz, R)  # noqa: E731
        return backend.stream_panel_rows(size(128), size(256) - size(128) if M > 128 else 0, M,
                                         DEFAULT_MAX_BYTES if max_bytes is None else max_bytes)

    def posterior_exceedance_moments(self, theta, Xs, mu, thresh, w, groups, ngroups, extra_var=None, panel_rows=None,
                                     max_bytes=None):
        def arr(t):
            return None if t is None else torch.as_tensor(t).detach().cpu().double().numpy()

        m, L = int(Xs.shape[0]), int(torch.as_tensor(thresh).shape[0])
        esz = torch.empty((), dtype=self.dtype).element_size()
        size = lambda R: stream_bytes(self.n, m, self.d, int(ngroups), L, esz, R)  # noqa: E731
        if panel_rows is None:
            panel_rows = self.exceedance_panel_rows(m, ngroups, L, max_bytes)
        if panel_rows <= 0 or panel_rows % 128:
            raise ValueError(f"panel_rows must be a positive multiple of 128, not {panel_rows}")
        StreamOraclePlan.streamed_calls.append(dict(m=m, levels=L, panel_rows=int(panel_rows), max_bytes=max_bytes,
                                                    bytes=size(panel_rows)))
        th, r, noise = self._state
        _kmean, cov = orc.posterior(self.model, self.X, r, noise, th, Xs.double(), full_cov=True)
        C = cov.numpy()
        mean, pc = dense_exceedance_moments(0.5 * (C + C.T), arr(mu), arr(thresh), arr(w), arr(groups), ngroups, arr(extra_var))
        return torch.tensor(mean), torch.tensor(pc)
