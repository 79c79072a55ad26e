"""The oracle-backed plan double with the BATCHED censored entry points of ``backend.GPPlan`` (TEST INFRASTRUCTURE):
``OraclePlan``'s batch surface with one ``LaplaceOraclePlan`` per site, the batched ``laplace_*`` methods answered by
``censored_helpers.laplace`` site by site.  ``laplace_calls`` (class-wide) counts the batched and single-site Laplace calls."""
from __future__ import annotations

import numpy as np
import torch

from discontinuum_amd import _lib
from tests.censored_helpers import LaplaceOraclePlan


class BatchedLaplaceOraclePlan(LaplaceOraclePlan):
    laplace_calls_total = 0  # every instance adds here: fit_many builds its plan itself

    def __init__(self, model, n, d, dtype=torch.float64, device="cpu", lookahead=True, batch=1):
        super().__init__(model, n, d, dtype=dtype, device=device, lookahead=lookahead, batch=batch)
        if self.batch > 1:
            self._sites = [LaplaceOraclePlan(model, n, d, dtype) for _ in range(self.batch)]

    def _laplace(self, with_grad, theta, y, mean, noise, side, f, maxit, tol):
        BatchedLaplaceOraclePlan.laplace_calls_total += 1
        if not self._sites:
            return super()._laplace(with_grad, theta, y, mean, noise, side, f, maxit, tol)
        self.laplace_calls = getattr(self, "laplace_calls", 0) + 1
        B, n = self.batch, self.n
        outs, drs, fs, stats, open_site = [], [], [], [], None
        for b, p in enumerate(self._sites):
            nb = self._sizes[b]
            pad = lambda v, fill=0.0: torch.cat([v, torch.full((n - v.shape[0],), fill, dtype=v.dtype)])  # noqa: E731
            f0 = None if f is None else f[b, :nb]
            try:
                res = p._laplace(with_grad, theta[b], y[b, :nb], mean[b, :nb], noise[b, :nb], side[b, :nb], f0, maxit, tol)
            except _lib.DGPError as e:
                assert e.code == _lib.E_NOCONV
                open_site = b if open_site is None else open_site
                res = (torch.zeros(_lib.OUT_LEN, dtype=self.dtype),) + ((torch.zeros(nb, dtype=self.dtype),) if with_grad else ()) + (
                    mean[b, :nb].detach().clone(), p.laplace_stat)
            stat = res[-1]
            if not np.any(np.asarray(side[b, :nb]) != 0):
                stat = (0.0, 0.0, 0.0, 0.0)
            outs.append(res[0])
            if with_grad:
                drs.append(pad(res[1]))
            tail = mean[b, nb:] if f is None else f[b, nb:]
            fs.append(torch.cat([res[-2], tail.detach().to(res[-2].dtype)]))
            stats.append(tuple(float(v) for v in stat))
        self.laplace_stat = tuple(stats)
        if open_site is not None:
            raise _lib.DGPError(_lib.E_NOCONV, "dgp_laplace_batched_fit_step", f"the mode search of site {open_site} did not converge")
        out, f_hat = torch.stack(outs), torch.stack(fs)
        return (out, torch.stack(drs), f_hat, self.laplace_stat) if with_grad else (out, f_hat, self.laplace_stat)

    def factorize(self, theta, r, noise):
        if not self._sites:
            return super().factorize(theta, r, noise)
        return torch.stack([p.factorize(theta[b], r[b, : self._sizes[b]], noise[b, : self._sizes[b]]) for b, p in enumerate(self._sites)])

    def predict(self, theta, Xs, chunk=4096):
        if not self._sites:
            return super().predict(theta, Xs, chunk)
        rows = [p.predict(theta[b], Xs[b]) for b, p in enumerate(self._sites)]
        return torch.stack([mu for mu, _ in rows]), torch.stack([var for _, var in rows])
