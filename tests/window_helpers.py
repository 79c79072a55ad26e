"""References shared by the rolling-window tests (tests/test_window_cpu.py, tests/test_gpu_window.py): the dense moments of
rolling-window means in plain numpy, the window layouts of the kernel tests, a brute-force ``time_windows`` and the
oracle-backed plan double."""
from __future__ import annotations

import numpy as np
import torch

from tests.exceedance_helpers import ExceedOraclePlan


def window_matrix(lo, hi, a, m):
    """The dense (q, m) row-stochastic W: W_ij = a_j / sum_{k in window i} a_k for lo[i] <= j < hi[i]; a zero row for an
    empty window or a zero weight sum."""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    a = np.ones(m) if a is None else np.asarray(a, np.float64)
    W = np.zeros((len(lo), m))
    for i in range(len(lo)):
        d = a[lo[i]:hi[i]].sum()
        if hi[i] > lo[i] and d > 0:
            W[i, lo[i]:hi[i]] = a[lo[i]:hi[i]] / d
    return W


def dense_window_moments(cov, mu, lo, hi, a=None, mode=0, scale2=None):
    """The formulas of ``dgp_window_moments`` on a dense SYMMETRIC fp64 covariance (m, m), with an explicit W:
    mode 0: mean = W mu, cov = W C W^T;  mode 1: e = exp(mu + s2 diag(C) / 2), mean = W e,
    cov = (W * e) expm1(s2 C) (W * e)^T.  -> (mean (q,), cov (q, q))."""
    C = np.asarray(cov, np.float64)
    mu = np.asarray(mu, np.float64)
    W = window_matrix(lo, hi, a, len(mu))
    if mode == 0:
        return W @ mu, W @ C @ W.T
    s2 = float(scale2)
    e = np.exp(mu + 0.5 * s2 * np.diagonal(C))
    We = W * e[None, :]
    return W @ e, We @ np.expm1(s2 * C) @ We.T


def trailing(m, w, step=1):
    """Trailing windows of w points ending at every ``step``-th point: [max(0, i + 1 - w), i + 1)."""
    i = np.arange(0, m, step)
    return np.maximum(i + 1 - w, 0).astype(np.int32), (i + 1).astype(np.int32)


def centred(m, w):
    i = np.arange(m)
    return np.maximum(i - w // 2, 0).astype(np.int32), np.minimum(i + w // 2 + 1, m).astype(np.int32)


def irregular_times(m, seed=0):
    """m sorted time stamps (datetime64[ns]) with irregular spacing -- runs of 40 samples at one or two a day, then 40 at one
    every few days -- and gaps of two months, so that 30-day windows hold 1 to about 40 points."""
    rng = np.random.default_rng(seed)
    step = np.where((np.arange(m) // 40) % 2 == 0, rng.uniform(0.3, 1.2, m), rng.uniform(2.0, 9.0, m))
    step[rng.choice(m, max(1, m // 60), replace=False)] += 60.0
    days = np.cumsum(step)
    return (np.datetime64("2012-01-01", "ns") + (days * 86400e9).astype(np.int64).astype("timedelta64[ns]")).astype("datetime64[ns]")


def ragged(m, seed=0):
    """Time-based trailing 30-day windows over an irregular record with gaps, evaluated on m evenly spaced output times
    between the first and the last sample: 0 (inside a gap) to about 40 points per window, both ends non-decreasing."""
    t = irregular_times(m, seed).astype(np.int64)
    out = np.linspace(t[0], t[-1], m).astype(np.int64)
    W = 30 * 86400 * 10 ** 9
    lo, hi = np.searchsorted(t, out - W, side="right"), np.searchsorted(t, out, side="right")
    return lo.astype(np.int32), hi.astype(np.int32)


def window_cases(m, seed=0):
    """{name: (lo, hi, a)} -- the window layouts of the kernel tests at m points."""
    rng = np.random.default_rng(seed + m)
    a = rng.uniform(0.2, 3.0, m)
    a[rng.choice(m, min(m, max(1, m // 40)), replace=False)] = 0.0
    cases = {
        "w1": (*trailing(m, 1), None),
        "w30": (*trailing(m, 30), None),
        "w200": (*trailing(m, 200), None),
        "wm": (*trailing(m, m), None),
        "centred31": (*centred(m, 31), None),
        "every7th": (*trailing(m, 30, step=7), None),
        "ragged": (*ragged(m, seed), None),
        "weights": (*trailing(m, 30), a),
    }
    return cases


def brute_time_windows(t, window_ns, align):
    """(lo, hi) by a loop over all pairs: the sorted int64 time stamps ``t`` inside (t_i - W, t_i] ("right") or
    [t_i - W/2, t_i + W/2) ("center"), as index ranges."""
    t = np.asarray(t, np.int64)
    m = len(t)
    lo, hi = np.zeros(m, np.int64), np.zeros(m, np.int64)
    for i in range(m):
        if align == "right":
            inside = [j for j in range(m) if t[i] - window_ns < t[j] <= t[i]]
        else:
            inside = [j for j in range(m) if 2 * t[i] - window_ns <= 2 * t[j] < 2 * t[i] + window_ns]
        if inside:
            assert inside == list(range(inside[0], inside[-1] + 1))
            lo[i], hi[i] = inside[0], inside[-1] + 1
        else:  # an empty window: where it would start
            lo[i] = hi[i] = int(np.searchsorted(t, t[i] - (window_ns if align == "right" else window_ns // 2), side="left"))
    return lo, hi


class WindowOraclePlan(ExceedOraclePlan):
    """``ExceedOraclePlan`` with ``window_moments`` by the dense reference (unbatched): -> float64 tensors, mean (q,) and an
    unpadded (q, q) covariance."""

    def window_moments(self, cov, m, mu, lo, hi, a=None, mode=0, scale2=None):
        def arr(t):
            return None if t is None else torch.as_tensor(t).detach().cpu().double().numpy()

        C = arr(cov)[:m, :m]
        C = np.tril(C) + np.tril(C, -1).T
        mean, S = dense_window_moments(C, arr(mu), arr(lo), arr(hi), arr(a), mode, scale2)
        return torch.tensor(mean), torch.tensor(S)
