"""Shared by the streamed rolling-mean tests (tests/test_window_stream_cpu.py, tests/test_gpu_window_stream.py): the
oracle-backed plan double that answers the three new plan entries and records every call it receives, and the work-area
formula of ``dgp_posterior_window_variances`` on the host."""
from __future__ import annotations

import numpy as np
import torch

from oracle import gp_oracle as orc
from tests.window_helpers import WindowOraclePlan, dense_window_moments


def _host(t):
    return None if t is None else torch.as_tensor(t).detach().cpu().double().numpy().copy()


class WindowStreamOraclePlan(WindowOraclePlan):
    """``WindowOraclePlan`` with ``posterior_window_variances``, ``posterior_cov_block`` and ``window_variances`` from the
    oracle's symmetric posterior covariance and ``dense_window_moments`` (unbatched).  ``calls`` lists (name, details) of
    every inference call, the dense pair included."""

    calls: list = []

    def _oracle_cov(self, Xs):
        theta, r, noise = self._state
        _kmean, cov = orc.posterior(self.model, self.X, r, noise, theta, Xs.double(), full_cov=True)
        C = cov.numpy()
        return np.tril(C) + np.tril(C, -1).T  # the lower triangle mirrored, as ``WindowOraclePlan.window_moments`` reads it

    def posterior_cov(self, theta, Xs):
        WindowStreamOraclePlan.calls.append(("posterior_cov", dict(m=int(Xs.shape[0]))))
        return super().posterior_cov(theta, Xs)

    def predict_mean(self, theta, Xs):
        WindowStreamOraclePlan.calls.append(("predict_mean", dict(m=int(Xs.shape[0]))))
        return super().predict_mean(theta, Xs)

    def window_moments(self, cov, m, mu, lo, hi, a=None, mode=0, scale2=None):
        WindowStreamOraclePlan.calls.append(("window_moments", dict(m=m, mode=mode)))
        return super().window_moments(cov, m, mu, lo, hi, a=a, mode=mode, scale2=scale2)

    def window_variances(self, cov, m, mu, lo, hi, a=None, mode=0, scale2=None):
        WindowStreamOraclePlan.calls.append(("window_variances", dict(m=m, mode=mode)))
        C = _host(cov)[:m, :m]
        C = np.tril(C) + np.tril(C, -1).T
        mean, S = dense_window_moments(C, _host(mu), _host(lo), _host(hi), _host(a), mode, scale2)
        return torch.tensor(mean), torch.tensor(np.diagonal(S).copy())

    def posterior_cov_block(self, theta, Xs, row0, row1, col0):
        WindowStreamOraclePlan.calls.append(("posterior_cov_block", dict(m=int(Xs.shape[0]), block=(row0, row1, col0))))
        m = int(Xs.shape[0])
        M = -(-m // 128) * 128
        full = np.eye(M)
        full[:m, :m] = self._oracle_cov(Xs)
        return torch.tensor(full[row0:row1, col0:row1].copy()).to(self.dtype)

    def posterior_window_variances(self, theta, Xs, mu, lo, hi, a=None, mode=0, scale2=None, panel_rows=None, max_bytes=None):
        WindowStreamOraclePlan.calls.append(("posterior_window_variances", dict(
            m=int(Xs.shape[0]), mu=_host(mu), lo=_host(lo).astype(np.int64), hi=_host(hi).astype(np.int64), a=_host(a), mode=mode,
            scale2=scale2, panel_rows=panel_rows, max_bytes=max_bytes)))
        mean, S = dense_window_moments(self._oracle_cov(Xs), _host(mu), _host(lo), _host(hi), _host(a), mode, scale2)
        return torch.tensor(mean), torch.tensor(np.diagonal(S).copy())


def window_stream_bytes(n, m, d, q, reach, esz, panel_rows, batch=1):
    """``dgp_posterior_window_variances_workspace_bytes`` by the documented formula: per site the prediction's layout (every
    area rounded up to 256 bytes), one band of R x (R + round_up(reach, 128)) elements, R = min(panel_rows, M), then 3 M + 3 Q
    doubles per site and one int per site."""
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    N, M, Q = -(-n // 128) * 128, -(-m // 128) * 128, -(-q // 128) * 128
    predict = up(esz * M * d) + 2 * up(esz * N * M) + 3 * up(esz * M) + up(esz * 64 * M)  # (64 rows of partial sums)
    R = min(panel_rows, M)
    band = up(esz * R * (R + -(-reach // 128) * 128))
    return batch * (predict + band) + up(8 * batch * (3 * M + 3 * Q)) + up(4 * batch)
