"""Shared by the streamed threshold-excess tests (tests/test_excess_stream_cpu.py, tests/test_gpu_excess_stream.py)."""
from __future__ import annotations


def excess_stream_bytes(n, m, d, P, L, esz, panel_rows):
    """The host's copy of ``dgp_posterior_excess_moments_workspace_bytes`` for one site: the prediction's layout (coordinates,
    cross Gram, V, three vectors, 64 rows of partial sums), the covariance panel of min(panel_rows, M) x M elements, each
    rounded up to 256 bytes, and M (3 + 6 L + P min(L, 8)) + P doubles."""
    N, M = -(-n // 128) * 128, -(-m // 128) * 128
    up = lambda b: -(-b // 256) * 256  # noqa: E731
    return (up(esz * M * d) + 2 * up(esz * N * M) + 3 * up(esz * M) + up(esz * 64 * M) + up(esz * min(panel_rows, M) * M)
            + 8 * (M * (3 + 6 * L + P * min(L, 8)) + P))
