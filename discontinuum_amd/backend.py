"""Device-side exact-GP plan: torch owns memory and streams, libdgp_hip.so does the arithmetic.

``GPPlan`` is the thin host object the engine (``discontinuum_amd.engines.hip``) drives; it is the
MI355X replacement for what gpytorch's ``ExactGP`` + ``ExactMarginalLogLikelihood`` +
``DefaultPredictionStrategy`` do underneath the reference loop
(``src/discontinuum/engines/gpytorch.py:318, 350-384, 599-626``).  No CPU fallback exists.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

MODELS = {"loadest": _lib.MODEL_LOADEST, "rating": _lib.MODEL_RATING}


def model_id(model: str) -> int:
    """``"loadest"`` / ``"rating"`` (the fused evaluators) or ``"composite:<id>"`` (a generic model registered through
    ``dgp_composite_define``; ``gp.lowering.lower`` returns such names)."""
    if model in MODELS:
        return MODELS[model]
    if isinstance(model, str) and model.startswith("composite:") and model[10:].isdigit():
        return int(model[10:])
    raise ValueError(f"unknown model {model!r}; expected one of {sorted(MODELS)} or 'composite:<id>'")
_DTYPES = {torch.float64: _lib.F64, torch.float32: _lib.F32}


def _theta_array(theta, ntheta):
    if torch.is_tensor(theta):
        theta = theta.detach().to("cpu", torch.float64).reshape(-1).tolist()
    vals = [float(v) for v in theta]
    if len(vals) != ntheta:
        raise ValueError(f"expected {ntheta} kernel hyperparameters, got {len(vals)}")
    return (C.c_double * ntheta)(*vals)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _call(name, *args):
    """The checked call ``name(*args, stream)`` of a library entry that takes no plan, on the current stream."""
    _lib.check(getattr(_lib.load(), name)(*args, _stream()), name)


class GPPlan:
    """Fixed (model, dtype, n, d) exact-GP problem resident on one GPU."""

    def __init__(self, model: str, n: int, d: int, dtype=torch.float64, device="cuda", lookahead=True, batch: int = 1):
        """``lookahead``: False / 0 = one stream; 1 = bulk updates beside the panel chain (use this when several
        plans share one GPU); True / 2 = also the early inverse on a third stream (best for one plan per GPU).
        ``batch`` > 1: the plan carries that many independent sites in lockstep (one launch per kernel for all of
        them); ``set_inputs`` / ``fit_step`` / ``factorize`` then take batch-major arrays -- X (batch, n, d),
        theta (batch, ntheta), r / noise (batch, n) -- and return (batch, 32), (batch, n), (batch, n)."""
        mid = model_id(model)
        if dtype not in _DTYPES:
            raise ValueError("dtype must be torch.float64 or torch.float32")
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("discontinuum_amd requires a ROCm GPU (MI355X); there is no CPU fallback")
        self.model, self.n, self.d, self.dtype = model, int(n), int(d), dtype
        self.device = torch.device(device)
        self.ntheta = self.lib.dgp_model_ntheta(mid, self.d)
        if self.ntheta < 0:
            raise ValueError(f"model {model!r} does not support d={d}")
        self.N = int(self.lib.dgp_padded_n(self.n))
        self.nterms = int(self.lib.dgp_model_nterms(mid, self.d))  # additive parts of the covariance (predict_terms)
        handle = C.c_void_p()
        _lib.check(self.lib.dgp_plan_create(mid, _DTYPES[dtype], self.n, self.d, C.byref(handle)), "dgp_plan_create")
        self._h = handle
        self.batch = int(batch)
        self._lead = () if self.batch == 1 else (self.batch,)  # the batch dimensions every result starts with
        self._site_sizes = [self.n] * self.batch  # rows every site uses (``set_site_sizes``)
        if self.batch != 1:
            self._host("dgp_plan_set_batch", self.batch)
        nbytes = int(self.lib.dgp_plan_workspace_bytes(self._h))
        with torch.cuda.device(self.device):
            self._ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
            off = (-self._ws.data_ptr()) % 256
            self._host("dgp_plan_set_workspace", C.c_void_p(self._ws.data_ptr() + off), nbytes)
        self.set_lookahead(lookahead)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                torch.cuda.synchronize(self.device)
            except Exception:  # noqa: BLE001
                pass
            self.lib.dgp_plan_destroy(h)
            self._h = None

    # ------------------------------------------------------------------ helpers
    def set_lookahead(self, level):
        level = 2 if level is True else int(level)
        self._host("dgp_plan_set_lookahead", level)

    def set_option(self, key: int, value: int):
        """Plan-level option (``_lib.OPT_*``; include/dgp_hip.h ``dgp_plan_set_option``): tile-shape selectors of the
        O(n^3) stages and the float32 refinement switch."""
        self._host("dgp_plan_set_option", int(key), int(value))

    def get_option(self, key: int) -> int:
        v = C.c_int64()
        self._host("dgp_plan_get_option", int(key), C.byref(v))
        return int(v.value)

    def _check_vec(self, t, name, length=None):
        length = (self.n if length is None else length) * self.batch
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == self.dtype and t.is_contiguous() and t.numel() == length):
            raise ValueError(f"{name} must be a contiguous {self.dtype} CUDA tensor with {length} elements")

    def _host(self, name, *args):
        """The checked library call ``name(plan, *args)`` of an entry that takes no stream."""
        _lib.check(getattr(self.lib, name)(self._h, *args), name)

    def _call(self, name, *args):
        """The checked library call ``name(plan, *args, stream)`` on the current stream."""
        _lib.check(getattr(self.lib, name)(self._h, *args, _stream()), name)

    def _empty(self, *tail, dtype=None):
        """An uninitialised result of shape ``self._lead + tail`` on the plan's device, in the plan's dtype unless given."""
        return torch.empty(self._lead + tail, dtype=dtype or self.dtype, device=self.device)

    def _theta(self, theta):
        return _theta_array(theta, self.ntheta * self.batch)

    def _check_xs(self, Xs):
        """The test points of an inference call: (m, d) -- (batch, m, d) for a batched plan -- in the plan's dtype, on the
        device.  -> m."""
        lead = self._lead
        if not (torch.is_tensor(Xs) and Xs.is_cuda and Xs.dtype == self.dtype and Xs.dim() == 2 + len(lead)
                and Xs.shape[-1] == self.d and tuple(Xs.shape[:-2]) == lead):
            raise ValueError(f"Xs must be a {lead + ('m', self.d)} {self.dtype} CUDA tensor")
        return int(Xs.shape[-2])

    def _work_area(self, attr, need, what, check_free=False):
        """256-byte aligned base of the entry point's cached work area ``self.<attr>``, grown to ``need`` bytes: an area
        that is too small is released BEFORE its replacement is allocated, and one that does not fit the device raises a
        ``RuntimeError`` that names ``what`` and the bytes.  ``check_free``: raise before trying when the free device memory
        (torch's cache included) cannot hold it."""
        ws = getattr(self, attr, None)
        if ws is None or ws.numel() < need + 256:
            setattr(self, attr, None)
            del ws  # (its bytes return to torch's cache, which counts as free here)
            if check_free:
                dev = self.device
                free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
                if need + 256 > free:
                    raise RuntimeError(f"{what} needs a work area of {need} bytes; {free} bytes of device memory are free")
            try:
                ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
            except torch.OutOfMemoryError as e:
                raise RuntimeError(f"{what} work area of {need} bytes does not fit the device") from e
            setattr(self, attr, ws)
        base = ws.data_ptr()
        return C.c_void_p(base + (-base) % 256)

    def _sized_work(self, attr, what, query, *sizes):
        """(base, bytes) of the work area ``self.<attr>`` at the size the library's ``query(plan, *sizes)`` reports: the
        ``work_dev, work_bytes`` pair of the entry point."""
        need = int(getattr(self.lib, query)(self._h, *sizes))
        return self._work_area(attr, need, what), need

    def _stream_work(self, attr, name, sizes, panel_rows, pick, bad_size):
        """(R, base, bytes) for the streamed entry point ``name``: the panel height -- ``panel_rows``, or ``pick()`` when it
        is None --, which must be a positive multiple of 128, and the cached work area ``self.<attr>`` at the size
        ``<name>_workspace_bytes(plan, *sizes, R)`` reports; a ``ValueError`` with the text ``bad_size`` when that is 0."""
        R = pick() if panel_rows is None else int(panel_rows)
        if R <= 0 or R % 128:
            raise ValueError(f"panel_rows must be a positive multiple of 128, not {panel_rows}")
        need = int(getattr(self.lib, name + "_workspace_bytes")(self._h, *sizes, R))
        if need == 0:
            raise ValueError(bad_size)
        return R, self._work_area(attr, need, name, check_free=True), need

    def _panel_sizes(self, name, sizes, max_bytes, bad_size):
        """(size, max_bytes) for the ``*_panel_rows`` methods: ``size(R)`` = ``<name>_workspace_bytes(plan, *sizes, R)``, the
        budget with its default ``loads.DEFAULT_MAX_BYTES``; a ``ValueError`` with the text ``bad_size`` when ``size(128)`` is 0."""
        if max_bytes is None:
            from .loads import DEFAULT_MAX_BYTES as max_bytes
        query = getattr(self.lib, name + "_workspace_bytes")
        sizes = tuple(int(v) for v in sizes)
        size = lambda R: int(query(self._h, *sizes, R))  # noqa: E731
        if size(128) == 0:
            raise ValueError(bad_size)
        return size, max_bytes

    def _linear_panel_rows(self, name, sizes, max_bytes, bad_size, what):
        """``stream_panel_rows`` on the sizes ``<name>_workspace_bytes`` reports for ``sizes`` (m first): a work area that
        grows linearly in the panel height."""
        size, max_bytes = self._panel_sizes(name, sizes, max_bytes, bad_size)
        M = int(self.lib.dgp_padded_n(int(sizes[0])))
        return stream_panel_rows(size(128), size(256) - size(128) if M > 128 else 0, M, max_bytes, what)

    def buffer(self, which: int, site: int = 0) -> torch.Tensor:
        """Tensor view of a plan buffer (tests / profiling); ``site``: which site's copy of a batched plan."""
        p, ld = C.c_void_p(), C.c_int64()
        self._host("dgp_plan_buffer", which, C.byref(p), C.byref(ld))
        if not 0 <= site < self.batch:
            raise ValueError(f"site must be in 0..{self.batch - 1}")
        esz = torch.empty((), dtype=self.dtype).element_size()
        off = p.value - self._ws.data_ptr() + site * int(self.lib.dgp_plan_site_stride_bytes(self._h))
        N = self.N
        count = {_lib.BUF_XT: self.d * N, _lib.BUF_Z: N, _lib.BUF_ALPHA: N}.get(which, N * N)
        flat = self._ws[off:off + count * esz].view(self.dtype)
        if which == _lib.BUF_XT:
            return flat.view(self.d, N)
        return flat if count == N else flat.view(N, N)

    def set_site_sizes(self, sizes):
        """Ragged batch: site b uses the first ``sizes[b]`` (<= n) rows of its slots; call before ``set_inputs``."""
        vals = [int(v) for v in sizes]
        if len(vals) != self.batch:
            raise ValueError(f"expected {self.batch} site sizes")
        arr = (C.c_int64 * self.batch)(*vals)
        with torch.cuda.device(self.device):
            self._call("dgp_plan_set_site_sizes", arr)
        self._site_sizes = vals

    # ------------------------------------------------------------------ hot path
    def set_dr_weights(self, w):
        """Two device vectors (2, n) -- (batch, 2, n) for a batched plan -- for which every following fit step also
        returns sum_i dNLL/dr_i w_k[i] in ``out[..., OUT_DR_W0 + k]`` (None clears).  The plan keeps the tensor alive."""
        if w is not None:
            shape = self._lead + (2, self.n)
            if not (torch.is_tensor(w) and w.is_cuda and w.dtype == self.dtype and tuple(w.shape) == shape
                    and w.is_contiguous()):
                raise ValueError(f"dr weights must be a contiguous {shape} {self.dtype} CUDA tensor")
        self._dr_w = w
        self._host("dgp_plan_set_dr_weights", _ptr(w))

    def set_inputs(self, X: torch.Tensor):
        self._check_vec(X, "X", self.n * self.d)
        with torch.cuda.device(self.device):
            self._call("dgp_set_inputs", _ptr(X))
        self._X = X  # keep alive until the async pack has certainly run

    def _fit(self, name, theta, r, noise, ws_query=None, grads=True, extra=()):
        """The one shape of a fit step: ``name(plan, theta, r, noise, *extra[, work, bytes], out[, dr, dnoise], stream)`` ->
        (out[32],) or (out[32], dr[n], dnoise[n]).  ``ws_query``: the size query of an entry that takes a work area (kept in
        ``self._loo_ws``): a name, or (name, *sizes) when the query takes sizes."""
        self._check_vec(r, "r")
        self._check_vec(noise, "noise")
        th = self._theta(theta)
        with torch.cuda.device(self.device):
            query = (ws_query,) if isinstance(ws_query, str) else ws_query
            work = () if query is None else self._sized_work("_loo_ws", name, *query)
            res = (self._empty(_lib.OUT_LEN),) + ((self._empty(self.n), self._empty(self.n)) if grads else ())
            self._call(name, th, _ptr(r), _ptr(noise), *extra, *work, *map(_ptr, res))
        return res

    def fit_step(self, theta, r: torch.Tensor, noise: torch.Tensor):
        """-> (out[32], alpha[n], dnoise[n]) device tensors; see include/dgp_hip.h DGP_OUT_*."""
        return self._fit("dgp_fit_step", theta, r, noise)

    def factorize(self, theta, r: torch.Tensor, noise: torch.Tensor):
        return self._fit("dgp_factorize", theta, r, noise, grads=False)[0]

    # ------------------------------------------------------------------ leave-one-out training objective
    def loo_fit_step(self, theta, r: torch.Tensor, noise: torch.Tensor):
        """The fit step of the leave-one-out predictive likelihood L_LOO = -elpd of ``cross_validate`` with folds of one:
        -> (out, dr, dnoise) with exactly the shapes and slots of ``fit_step``, ``out[OUT_NLL]`` = L_LOO and every gradient
        slot that of L_LOO; QUAD, LOGDET, INFO are the factorisation's.  The plan holds afterwards what ``fit_step`` with the
        same arguments leaves.  float64 plans (include/dgp_hip.h ``dgp_loo_fit_step``)."""
        return self._fit("dgp_loo_fit_step", theta, r, noise, ws_query="dgp_loo_workspace_bytes")

    def loo_value(self):
        """(L_LOO, info) -- (batch, 2) for a batched plan -- as float64 device tensor, from the factorisation the plan holds
        when the last step left K^^-1 in it (``fit_step`` / ``loo_fit_step``)."""
        with torch.cuda.device(self.device):
            work = self._sized_work("_loo_ws", "dgp_loo_value", "dgp_loo_value_workspace_bytes")
            out = self._empty(2, dtype=torch.float64)
            self._call("dgp_loo_value", *work, _ptr(out))
        return out

    # ------------------------------------------------------------------ leave-group-out training objective
    def set_folds(self, groups):
        """The folds of ``lgo_fit_step`` / ``lgo_value``: fold ids per observation as ``cross_validate`` takes them -- (n,),
        or (batch, n) for a batched plan, integers >= 0, -1 = never held out; a site's folds may be empty.  Validated and
        sorted on the host as there; the plan keeps ``order`` / ``start`` on the device, with ``ngroups`` and ``max_group``.
        None clears them."""
        if groups is None:
            self._folds = None
            return

        def keep(order, start, ngroups, max_group):
            dev = lambda t: t.contiguous().to(self.device)  # noqa: E731
            return dev(order), dev(start), int(ngroups), int(max_group)

        self._folds = cross_validate_folds(self, groups, keep)

    def _lgo_folds(self, what):
        folds = getattr(self, "_folds", None)
        if folds is None:
            raise ValueError(f"{what}: no folds in the plan (call set_folds first)")
        order, start, ngroups, max_group = folds
        return (_ptr(order), _ptr(start), ngroups, max_group), (ngroups, max_group)

    def lgo_fit_step(self, theta, r: torch.Tensor, noise: torch.Tensor):
        """The fit step of the leave-group-out predictive likelihood L_LGO = -sum of ``cross_validate``'s ``lpd`` on the
        folds of ``set_folds``: -> (out, dr, dnoise) with exactly the shapes and slots of ``fit_step``, ``out[OUT_NLL]`` =
        L_LGO and every gradient slot that of L_LGO; QUAD, LOGDET, INFO are the factorisation's.  The plan holds afterwards
        what ``fit_step`` with the same arguments leaves.  float64 plans (include/dgp_hip_ext2.h ``dgp_lgo_fit_step``)."""
        extra, sizes = self._lgo_folds("lgo_fit_step")
        return self._fit("dgp_lgo_fit_step", theta, r, noise, ws_query=("dgp_lgo_workspace_bytes", *sizes), extra=extra)

    def lgo_value(self):
        """(L_LGO, info) -- (batch, 2) for a batched plan -- as float64 device tensor, from the factorisation the plan holds
        when the last step left K^^-1 in it, on the folds of ``set_folds``."""
        extra, sizes = self._lgo_folds("lgo_value")
        with torch.cuda.device(self.device):
            work = self._sized_work("_loo_ws", "dgp_lgo_value", "dgp_lgo_value_workspace_bytes", *sizes)
            out = self._empty(2, dtype=torch.float64)
            self._call("dgp_lgo_value", *extra, *work, _ptr(out))
        return out

    # ------------------------------------------------------------------ censored observations (Laplace)
    def _check_side(self, side):
        if not (torch.is_tensor(side) and side.is_cuda and side.dtype == torch.int32 and side.is_contiguous()
                and side.numel() == self.n * self.batch):
            raise ValueError(f"side must be a contiguous int32 CUDA tensor with {self.n * self.batch} elements")

    def _check_censored(self, side, **vectors):
        """``side`` and the named per-row vectors of a censored fit; only ``upper`` may be None."""
        for what, t in vectors.items():
            if not (what == "upper" and t is None):
                self._check_vec(t, what)
        self._check_side(side)

    def _laplace(self, with_grad, theta, y, mean, noise, side, f, maxit, tol, upper=None):
        B = self.batch
        name = ("dgp_laplace_fit_step" if with_grad else "dgp_laplace_factorize") if B == 1 else (
            "dgp_laplace_batched_fit_step" if with_grad else "dgp_laplace_batched_factorize")
        if upper is not None:  # rows of side 2 (the truth in [y, upper]): one pair of entries for every float64 plan
            name = "dgp_laplace_interval_fit_step" if with_grad else "dgp_laplace_interval_factorize"
        if self.dtype != torch.float64:
            raise ValueError(f"{name}: censored fits need a float64 " + ("single-site plan" if B == 1 else "plan"))
        self._check_censored(side, y=y, mean=mean, noise=noise, upper=upper)
        if f is None:
            f = mean.clone()  # cold start
        else:
            self._check_vec(f, "f")
            f = f.clone()
        th = self._theta(theta)
        stat = (C.c_double * (4 * B))()
        with torch.cuda.device(self.device):
            work = self._sized_work("_laplace_ws", name, "dgp_laplace_workspace_bytes" if B == 1 else "dgp_laplace_batched_workspace_bytes")
            out = self._empty(_lib.OUT_LEN)
            dr = self._empty(self.n) if with_grad else None
            try:
                self._call(name, th, *(_ptr(t) for t in (y, mean, noise, side, upper, f) if t is not None), int(maxit), float(tol), *work,
                           *(_ptr(t) for t in (out, dr) if t is not None), stat)
            finally:  # kept for a caller that catches E_NOCONV; a batched plan: one 4-tuple per site
                vals = [float(v) for v in stat]
                self.laplace_stat = tuple(vals) if B == 1 else tuple(tuple(vals[4 * b:4 * b + 4]) for b in range(B))
        return (out, dr, f, self.laplace_stat) if with_grad else (out, f, self.laplace_stat)

    def laplace_fit_step(self, theta, y, mean, noise, side, f=None, maxit=50, tol=1e-10, upper=None):
        """One fit step with censored rows (``side`` int32: -1 the truth is below the limit in ``y``, 0 observed, +1 above) by
        the Laplace approximation: Newton's mode search from ``f`` (None: the prior mean), then the step at the mode.
        -> (out[32], dr[n], f_hat[n], stat) with ``out[OUT_NLL]`` the Laplace NLL, ``out[OUT_DTHETA:]`` its gradient,
        dr = alpha - u and stat = (Newton iterations, final max |df|, halvings, capped rows); the plan holds the
        pseudo-data system's factorisation.  ``DGPError`` with code ``E_NOCONV`` when ``maxit`` does not suffice
        (``self.laplace_stat`` is set either way).
        A batched plan (``batch`` > 1, ragged or not) takes batch-major arrays -- theta (batch, ntheta), y / mean / noise / f
        (batch, n), side int32 (batch, n) -- and returns out (batch, 32), dr (batch, n), f_hat (batch, n) and stat as a tuple of
        ``batch`` 4-tuples: Newton's iterations run in lockstep, a finished site is frozen, and every site's mode, iteration
        count and halvings are its own (``dgp_laplace_batched_fit_step``).  ``E_NOCONV`` when any censored site is not
        converged after ``maxit``; a site that is not positive definite reports it in its own ``out[b, OUT_INFO]``.
        ``upper`` (shaped like ``y``): the upper ends of the INTERVAL-censored rows, side 2 -- the truth of such a row lies in
        [y, upper] -- read on those rows only (``dgp_laplace_interval_fit_step``, every float64 plan).  None: the entries
        above, for which 2 is a bad side value; with ``upper`` and no row of side 2 the results are bitwise theirs."""
        return self._laplace(True, theta, y, mean, noise, side, f, maxit, tol, upper)

    def laplace_factorize(self, theta, y, mean, noise, side, f=None, maxit=50, tol=1e-10, upper=None):
        """The same without gradients (the prediction-time cache build) -> (out[32], f_hat[n], stat)."""
        return self._laplace(False, theta, y, mean, noise, side, f, maxit, tol, upper)

    # ------------------------------------------------------------------ censored observations (expectation propagation)
    def _ep(self, with_grad, theta, y, mean, noise, side, sites, maxit, tol, damping, upper):
        name = "dgp_ep_fit_step" if with_grad else "dgp_ep_factorize"
        if self.dtype != torch.float64 or self.batch != 1:
            raise ValueError(f"{name}: expectation propagation needs a float64 single-site plan")
        self._check_censored(side, y=y, mean=mean, noise=noise, upper=upper)
        if sites is None:  # cold start
            yt, nt = torch.empty_like(y), torch.empty_like(noise)
        else:
            yt, nt = sites
            self._check_vec(yt, "sites[0]")
            self._check_vec(nt, "sites[1]")
            yt, nt = yt.clone(), nt.clone()
        th = self._theta(theta)
        stat = (C.c_double * 6)()
        with torch.cuda.device(self.device):
            work = self._sized_work("_ep_ws", name, "dgp_ep_workspace_bytes")
            out = self._empty(_lib.OUT_LEN)
            dr = self._empty(self.n) if with_grad else None
            aux = self._empty(3, self.n)
            try:
                self._call(name, th, _ptr(y), _ptr(mean), _ptr(noise), _ptr(side), _ptr(upper), _ptr(yt), _ptr(nt), int(sites is None),
                           int(maxit), float(tol), float(damping), *work, *(_ptr(t) for t in (out, dr) if t is not None), stat,
                           _ptr(aux[0]), _ptr(aux[1]), _ptr(aux[2]))
            finally:  # kept for a caller that catches E_NOCONV
                self.ep_stat = tuple(float(v) for v in stat)
                self.ep_aux = {"cav_mean": aux[0], "cav_var": aux[1], "logz": aux[2]}
                self.ep_sites = (yt, nt)
        return (out, dr, (yt, nt), self.ep_stat) if with_grad else (out, (yt, nt), self.ep_stat)

    def ep_fit_step(self, theta, y, mean, noise, side, sites=None, maxit=100, tol=1e-10, damping=1.0, upper=None):
        """One fit step with censored rows (``side`` / ``upper`` as for ``laplace_fit_step``) by EXPECTATION PROPAGATION
        (``dgp_ep_fit_step``): parallel sweeps of moment matching from ``sites`` = (y~, n~) (None: cold, from the Laplace terms at
        the prior mean), each one factorisation, then the step at the final sites.  -> (out[32], dr[n], (y~, n~), stat) with
        ``out[OUT_NLL]`` = -log Z_EP, ``out[OUT_DTHETA:]`` its gradient (the engine's explicit gradient at the fixed point),
        dr = alpha and stat = (sweeps, final max |dmu|, final max v |dtau|, capped rows, rows held back, censored rows).  The plan
        holds the factorisation of the pseudo-data system (y~ - mean, n~), and ``self.ep_aux`` the cavities and log Z^ of that
        state.  ``DGPError`` with code ``E_NOCONV`` when ``maxit`` sweeps do not suffice (``self.ep_stat`` / ``self.ep_sites`` are set
        either way).  float64 single-site plans only."""
        return self._ep(True, theta, y, mean, noise, side, sites, maxit, tol, damping, upper)

    def ep_factorize(self, theta, y, mean, noise, side, sites=None, maxit=100, tol=1e-10, damping=1.0, upper=None):
        """The same without gradients (the prediction-time cache build) -> (out[32], (y~, n~), stat)."""
        return self._ep(False, theta, y, mean, noise, side, sites, maxit, tol, damping, upper)

    def ep_diag(self):
        """diag((K^)^-1) (n,) of the factorisation the plan holds, as an EP sweep computes it from L^-1 (``dgp_ep_diag``)."""
        with torch.cuda.device(self.device):
            work = self._sized_work("_ep_ws", "dgp_ep_diag", "dgp_ep_workspace_bytes")
            k = self._empty(self.n)
            self._call("dgp_ep_diag", _ptr(k), *work)
        return k

    def interval_terms(self, za: torch.Tensor, delta: torch.Tensor):
        """(4, count): log P, sigma g, W v, sigma^3 d3 of the brackets [za, za + delta] as the interval-censored fit evaluates
        them (P = Phi(zb) - Phi(za))."""
        for t in (za, delta):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.dim() == 1 and t.numel() > 0):
                raise ValueError("za and delta must be non-empty contiguous 1-d float64 CUDA tensors")
        if za.numel() != delta.numel() or za.device != delta.device:
            raise ValueError("za and delta must have the same length and device")
        with torch.cuda.device(za.device):
            out = torch.empty((4, za.numel()), dtype=torch.float64, device=za.device)
            _call("dgp_debug_interval_terms", _ptr(za), _ptr(delta), za.numel(), _ptr(out))
        return out

    def censored_terms(self, z: torch.Tensor):
        """(4, count): log Phi(z), h = phi / Phi, h (z + h), h [1 - (z + h)(z + 2 h)] as the censored fit evaluates them."""
        if not (torch.is_tensor(z) and z.is_cuda and z.dtype == torch.float64 and z.is_contiguous() and z.dim() == 1 and z.numel() > 0):
            raise ValueError("z must be a non-empty contiguous 1-d float64 CUDA tensor")
        with torch.cuda.device(z.device):
            out = torch.empty((4, z.numel()), dtype=torch.float64, device=z.device)
            _call("dgp_debug_censored_terms", _ptr(z), z.numel(), _ptr(out))
        return out

    def bilinear(self, theta, u: torch.Tensor, alpha: torch.Tensor):
        """sum_ij u_i dK_ij/dtheta_p alpha_j for every p (ntheta,): the censored fit's pair sweep alone (tests).  A batched plan:
        u, alpha (batch, n), theta (batch, ntheta) -> (batch, ntheta)."""
        self._check_vec(u, "u")
        self._check_vec(alpha, "alpha")
        B = self.batch
        th = self._theta(theta)
        name = "dgp_debug_bilinear" if B == 1 else "dgp_debug_bilinear_batched"
        with torch.cuda.device(self.device):
            work = self._sized_work("_laplace_ws", name, "dgp_laplace_workspace_bytes" if B == 1 else "dgp_laplace_batched_workspace_bytes")
            out = self._empty(self.ntheta)
            self._call(name, th, _ptr(u), _ptr(alpha), *work, _ptr(out))
        return out

    def _chunks(self, Xs, outs, chunk, planes, ws_attr, what, ws_query, sizes, call):
        """The chunk loop of every per-point product.  ``outs``: the result tensors, the m test points their last dimension,
        None for a result that was not asked for (a null pointer for the library).  For every ``chunk`` points -- None:
        16384 // (batch planes) rounded down to a multiple of 128, at least 128; the work areas are batch x 2 planes N x
        chunk elements -- the work area ``self.<ws_attr>`` is grown to ``ws_query(plan, points, *sizes)`` bytes and
        ``call(xs, points, work, bytes, *pointers)`` makes the checked library call.  A chunk's columns ``out[..., lo:hi]``
        are written in place where they are contiguous (the whole range; a range of an unbatched (m,) result) and staged in
        a fresh tensor and copied back otherwise.  -> ``outs``."""
        if chunk is None:
            chunk = max(128, (16384 // (self.batch * planes)) // 128 * 128)
        m = int(Xs.shape[-2])
        with torch.cuda.device(self.device):
            for lo in range(0, m, chunk):
                hi = min(lo + chunk, m)
                xs = Xs[..., lo:hi, :].contiguous()
                work = self._sized_work(ws_attr, what, ws_query, hi - lo, *sizes)
                cols = [None if t is None else t[..., lo:hi] for t in outs]
                stage = [c if c is None or c.is_contiguous() else torch.empty(c.shape, dtype=c.dtype, device=c.device) for c in cols]
                call(xs, hi - lo, *work, *map(_ptr, stage))
                for c, s in zip(cols, stage):
                    if s is not c:
                        c.copy_(s)
        return outs

    def predict(self, theta, Xs: torch.Tensor, chunk: int | None = None):
        """Latent posterior (K*^T alpha, diag(K** - K*^T K^^-1 K*)) at Xs (m, d) from the held factorisation.
        Batched plans: Xs (batch, m, d), theta (batch, ntheta) -> mean, var (batch, m); every site predicts at its own
        points from the factorisation the last ``fit_step`` / ``factorize`` left in its slice of the workspace.
        ``chunk`` = prediction points per launch sequence.  The work area is batch x 2 N x chunk elements (cross Gram and
        V = L^-1 K* per site), so the default is 16384 // batch rounded down to a multiple of 128 (at least 128): a
        batched prediction then needs no more work memory than a single site's (n = 8192 fp64: 2.1 GB)."""
        m, th = self._check_xs(Xs), self._theta(theta)

        def call(xs, k, work, need, mean_ptr, var_ptr):
            self._call("dgp_predict", th, _ptr(xs), k, work, need, mean_ptr, var_ptr)

        return self._chunks(Xs, (self._empty(m), self._empty(m)), chunk, 1, "_pred_ws", "prediction", "dgp_predict_workspace_bytes", (), call)

    def predict_terms(self, theta, Xs: torch.Tensor, chunk: int | None = None, return_cov: bool = True):
        """Latent posterior of every ADDITIVE PART of the covariance at Xs (m, d) from the held factorisation
        (``dgp_predict_terms``): -> (mean (C, m), cov (C (C + 1) / 2, m)) with C = ``self.nterms`` parts in the model's
        order (loadest: seasonal, covariates, residual; rating: shift_1, shift_2, bend, base, periodic; composite: its
        terms).  ``cov[c (c + 1) / 2 + c']`` (c' <= c) is the posterior covariance of parts c and c' at each point; the
        means sum to ``predict``'s mean and the full C x C covariance to its variance.  Batched plans: Xs (batch, m, d),
        theta (batch, ntheta) -> (batch, C, m), (batch, C (C + 1) / 2, m).  ``return_cov=False`` -> (mean, None).
        ``chunk`` = points per launch sequence; the work area is batch x 2 C N x chunk elements, so the default is
        16384 // (batch C) rounded down to a multiple of 128 (at least 128)."""
        Cn, m, th = self.nterms, self._check_xs(Xs), self._theta(theta)
        outs = self._empty(Cn, m), self._empty(Cn * (Cn + 1) // 2, m) if return_cov else None

        def call(xs, k, work, need, mean_ptr, cov_ptr):
            self._call("dgp_predict_terms", th, _ptr(xs), k, work, need, mean_ptr, cov_ptr)

        return self._chunks(Xs, outs, chunk, Cn, "_terms_ws", "prediction", "dgp_predict_terms_workspace_bytes", (), call)

    def predict_slopes(self, theta, Xs: torch.Tensor, cols, chunk: int | None = None, return_cov: bool = True):
        """Latent posterior of the fit and of its DERIVATIVES with respect to the raw input columns ``cols`` (distinct, in
        0 .. d - 1) at Xs (m, d) from the held factorisation (``dgp_predict_slopes``): -> (mean (P, m), cov (P (P + 1) / 2,
        m)) with P = 1 + len(cols) planes -- plane 0 the value (``predict``'s mean and variance), plane q + 1 the slope in
        column ``cols[q]`` per unit of that model-space input.  ``cov[a (a + 1) / 2 + b]`` (b <= a) is the posterior covariance
        of planes a and b at each point.  Batched plans: Xs (batch, m, d), theta (batch, ntheta) -> (batch, P, m), (batch,
        P (P + 1) / 2, m).  ``return_cov=False`` -> (mean, None).  A column the covariance is not differentiable in (a
        Matern-1/2 factor of a composite) raises.  ``chunk`` = points per launch sequence; the work area is batch x 2 P N x
        chunk elements, so the default is 16384 // (batch P) rounded down to a multiple of 128 (at least 128)."""
        cols = [int(c) for c in cols]
        if not 1 <= len(cols) <= self.d or len(set(cols)) != len(cols) or min(cols) < 0 or max(cols) >= self.d:
            raise ValueError(f"cols must be 1 .. {self.d} distinct columns in 0 .. {self.d - 1}, got {cols}")
        mid = model_id(self.model)
        for c in cols:
            if int(self.lib.dgp_model_input_differentiable(mid, self.d, c)) != 1:
                raise ValueError(f"the covariance is not differentiable in column {c} (Matern-1/2 factor)")
        Pn, carr = 1 + len(cols), (C.c_int * len(cols))(*cols)
        m, th = self._check_xs(Xs), self._theta(theta)
        outs = self._empty(Pn, m), self._empty(Pn * (Pn + 1) // 2, m) if return_cov else None

        def call(xs, k, work, need, mean_ptr, cov_ptr):
            self._call("dgp_predict_slopes", th, _ptr(xs), k, carr, len(cols), work, need, mean_ptr, cov_ptr)

        return self._chunks(Xs, outs, chunk, Pn, "_slopes_ws", "prediction", "dgp_predict_slopes_workspace_bytes", (len(cols),), call)

    # ------------------------------------------------------------------ cross-validation
    def cross_validate(self, groups, max_group=None):
        """Exact leave-group-out cross-validation at the hyperparameters of the factorisation the plan holds
        (``dgp_cross_validate``; no fold is refitted).  ``groups``: an integer tensor / array (n,) -- (batch, n) for a
        batched plan -- of fold ids >= 0, -1 for an observation that is never held out; a site of a ragged batch uses its
        first ``sizes[b]`` entries.  -> (resid, var, lpd, info): held-out residual y_i - E[y_i | other folds] and held-out
        predictive variance of the OBSERVATION (its own noise included), both (n,) fp64 in model space and 0 where
        ``groups`` is -1; ``lpd`` (ngroups,) the joint log predictive density of every fold (0 for a fold id nobody uses);
        ``info`` (ngroups,) int32, 0 or the failing pivot.  ngroups = 1 + the largest fold id of any site.
        ``max_group``: an upper bound of the fold sizes handed to the library instead of the largest fold found -- the
        bound selects the device route and its block order, so results are bitwise comparable between calls (a site alone
        and the same site inside a batch) only under the same bound."""
        return cross_validate_folds(self, groups, self._cv_launch, max_group)

    def _cv_launch(self, order, start, ngroups, max_group):
        need = int(self.lib.dgp_cross_validate_workspace_bytes(self._h, ngroups, max_group))
        if need == 0:
            raise ValueError(f"bad size: ngroups = {ngroups}, max_group = {max_group} (both in 1..n)")
        with torch.cuda.device(self.device):
            work = self._work_area("_cv_ws", need, "cross-validation")
            order = order.to(self.device).contiguous()
            start = start.to(self.device).contiguous()
            resid, var = self._empty(self.n, dtype=torch.float64), self._empty(self.n, dtype=torch.float64)
            lpd, info = self._empty(ngroups, dtype=torch.float64), self._empty(ngroups, dtype=torch.int32)
            self._call("dgp_cross_validate", _ptr(order), _ptr(start), ngroups, max_group, work, need, _ptr(resid), _ptr(var),
                       _ptr(lpd), _ptr(info))
        return resid, var, lpd, info

    def laplace_cross_validate(self, theta, y, mean, noise, side, f, groups, upper=None, shift=0.0, max_group=None):
        """Cross-validation of a CENSORED fit by Laplace cavity folds (``dgp_laplace_cross_validate``), from the factorisation
        of the pseudo-data system that ``laplace_factorize`` / ``laplace_fit_step`` left in the plan; no fold is refitted.
        ``y`` / ``mean`` / ``noise`` / ``side`` / ``upper``: what the fit was given; ``f``: the mode it returned; ``groups`` /
        ``max_group``: as for ``cross_validate``.  -> dict of (n,) fp64 tensors ``mu`` / ``var`` (the held-out predictive of
        the OBSERVATION, as ``cross_validate``'s y - resid / var), ``lpd`` (pointwise: the Gaussian density of an observed
        row, the probability of a censored row's bracket), ``pit_lower`` / ``pit_upper``, ``dlp`` (d lpd / d mu) and ``tilt``
        (log of the bracket's probability with both ends shifted by -``shift`` sd, minus lpd; 0 on observed rows) -- all 0
        where ``groups`` is -1 -- plus ``info`` (ngroups,) int32.  The pseudo-data of the rows that stay are held at the
        full-data mode: an approximation on top of Laplace's.  float64 single-site plans only."""
        if self.batch != 1:
            raise NotImplementedError("laplace_cross_validate: batched plans are not supported (validate each site on its own plan)")
        if self.dtype != torch.float64:
            raise ValueError("laplace_cross_validate: censored fits need a float64 single-site plan")
        self._check_censored(side, y=y, mean=mean, noise=noise, f=f, upper=upper)
        th = self._theta(theta)

        def launch(order, start, ngroups, mg):
            need = int(self.lib.dgp_laplace_cross_validate_workspace_bytes(self._h, ngroups, mg))
            if need == 0:
                raise ValueError(f"bad size: ngroups = {ngroups}, max_group = {mg} (both in 1..n)")
            with torch.cuda.device(self.device):
                work = self._work_area("_lcv_ws", need, "cross-validation of a censored fit")
                order = order.to(self.device).contiguous()
                start = start.to(self.device).contiguous()
                out = self._empty(len(_lib.LCV_PLANE_NAMES), self.n, dtype=torch.float64)
                info = self._empty(ngroups, dtype=torch.int32)
                self._call("dgp_laplace_cross_validate", th, _ptr(y), _ptr(mean), _ptr(noise), _ptr(side), _ptr(upper), _ptr(f),
                           _ptr(order), _ptr(start), ngroups, mg, float(shift), work, need, _ptr(out), _ptr(info))
            res = {name: out[k] for k, name in enumerate(_lib.LCV_PLANE_NAMES)}
            res["info"] = info
            return res

        return cross_validate_folds(self, groups, launch, max_group)

    # ------------------------------------------------------------------ Fisher information of the hyperparameters
    def fisher(self, theta, diag=None, max_bytes: int | None = None):
        """Exact Fisher information F_ab = 1/2 tr(K^^-1 D_a K^^-1 D_b) of the hyperparameters at the factorisation the plan
        holds (``dgp_fisher``; nothing is refactored, the plan is only read).  Directions: first the ``ntheta`` kernel
        directions dK/dtheta_p at ``theta`` (constrained values, as for ``fit_step``), then the E rows of ``diag`` -- (E, n),
        or (batch, E, n) for a batched plan, E <= 8, in the plan's dtype on the device -- as diagonal directions diag(d_e)
        (derivatives of learned noise terms; None: none).  -> (P + E, P + E) -- (batch, P + E, P + E) -- float64 device
        tensor, bitwise symmetric, in un-normalised log-likelihood units.  The work area of (P + E + 1) N^2 elements per
        site is kept between calls; ``max_bytes``: raise ``ValueError`` naming the bytes instead of allocating more."""
        th = self._theta(theta)
        diag, E = self._check_columns(diag, "diag")
        need = int(self.lib.dgp_fisher_workspace_bytes(self._h, E))
        if max_bytes is not None and need > int(max_bytes):
            raise ValueError(f"the Fisher information of {self.ntheta + E} directions at n = {self.n} (batch {self.batch}) needs a "
                             f"work area of {need} bytes, which exceeds max_bytes = {int(max_bytes)}")
        nd = self.ntheta + E
        with torch.cuda.device(self.device):
            work = self._work_area("_fisher_ws", need, "dgp_fisher")
            out = self._empty(nd, nd, dtype=torch.float64)
            self._call("dgp_fisher", th, _ptr(diag), E, work, need, _ptr(out))
        return out

    # ------------------------------------------------------------------ Jacobians of the prediction w.r.t. the hyperparameters
    def _check_columns(self, cols, name):
        """A (K, n) -- (batch, K, n) -- device tensor of per-training-row columns in the plan's dtype, K <= 8 -> (tensor or None, K)."""
        if cols is None:
            return None, 0
        lead = self._lead
        if not (torch.is_tensor(cols) and cols.is_cuda and cols.dtype == self.dtype and cols.dim() == 2 + len(lead)
                and tuple(cols.shape[:-2]) == lead and cols.shape[-1] == self.n):
            raise ValueError(f"{name} must be a {lead + ('K', self.n)} {self.dtype} CUDA tensor")
        K = int(cols.shape[-2])
        if K > 8:
            raise ValueError(f"at most 8 rows of {name}, got {K}")
        return (cols.contiguous() if K else None), K

    def predict_sensitivity(self, theta, Xs: torch.Tensor, diag=None, rhs=None, chunk: int | None = None, return_var: bool = True):
        """Exact Jacobians of the latent posterior mean and variance at Xs (m, d) with respect to the hyperparameter
        DIRECTIONS, from the factorisation the plan holds (``dgp_predict_sensitivity``; the plan is only read): first the
        P = ``ntheta`` kernel directions at ``theta`` (constrained values), then the E rows of ``diag`` as diagonal
        directions diag(d_e) of K^ (learned noise terms), then -- for the mean only -- the C rows of ``rhs`` as directions
        g_c of the prior mean at the training rows (the caller adds the prior mean's own derivative at the test rows).
        ``diag`` (E, n) / ``rhs`` (C, n), (batch, ., n) for a batched plan, E, C <= 8, plan dtype, on the device; None: none.
        -> (dmean (P + E + C, m), dvar (P + E, m) or None with ``return_var=False``) in float64; batched plans: Xs
        (batch, m, d), theta (batch, ntheta) and a leading batch dimension on both results.  The Jacobians are exact; what a
        caller builds from them and a covariance of the hyperparameters is first order in that covariance (delta method).
        ``chunk`` = points per launch sequence: the chunks' results are independent, so their concatenation is exact.  The
        work area is batch x (P N^2 + 3 N chunk) elements; default chunk as for ``predict``."""
        m, th = self._check_xs(Xs), self._theta(theta)
        diag, E = self._check_columns(diag, "diag")
        rhs, Cn = self._check_columns(rhs, "rhs")
        dmean = self._empty(self.ntheta + E + Cn, m, dtype=torch.float64)
        dvar = self._empty(self.ntheta + E, m, dtype=torch.float64) if return_var else None

        def call(xs, k, work, need, dmean_ptr, dvar_ptr):
            self._call("dgp_predict_sensitivity", th, _ptr(xs), k, _ptr(diag), E, _ptr(rhs), Cn, work, need, dmean_ptr, dvar_ptr)

        return self._chunks(Xs, (dmean, dvar), chunk, 1, "_sens_ws", "dgp_predict_sensitivity",
                            "dgp_predict_sensitivity_workspace_bytes", (E, Cn), call)

    # ------------------------------------------------------------------ influence of the held samples on the period sums
    def deletion_influence(self, theta, Xs: torch.Tensor, groups, a, scale, periods, nperiods: int, mode: int, inv_sd=None,
                           max_bytes: int | None = None, max_group=None):
        """Exact change of every period sum when a fold of training observations is deleted, for all folds at once, at the
        hyperparameters of the factorisation the plan holds (``dgp_deletion_influence``; nothing is refitted, the plan is only
        read).  ``groups``: fold ids per observation as ``cross_validate`` takes them ((n,) / (batch, n) integers >= 0, -1 =
        in no fold); ``max_group``: as there, an upper bound of the fold sizes handed to the library in place of the largest fold
        found -- a ROUTE SELECTOR (1: leave-one-out, <= 64: LDS, larger: blocks of that order rounded up to 128), for callers that
        compare a site alone with the same site in a batch; ``Xs`` (m, d) / (batch, m, d) the test points, ``theta`` as for ``predict``;
        ``a`` (m,) / (batch, m): w_j exp(s mu_j + t + s^2 C_jj / 2) for a log target (``mode`` = MODE_LOG), s w_j for a linear
        one; ``scale``: s, a number or (batch,) values; ``periods`` int32 ids (m,) / (batch, m) in 0 .. nperiods - 1,
        non-decreasing, -1 = excluded; ``inv_sd`` None or (m,) / (batch, m): 1 / sigma_j of the posterior at the test points.
        -> (dload (F, P), dvar (F, P) for a linear target else None, shift (F,) = max_j |dmu_Fj| inv_sd_j or None without
        ``inv_sd``, info (F,) int32: 0 or the failing pivot of the fold's block, whose results are NaN), F = 1 + the largest
        fold id, with a leading batch dimension for a batched plan; float64.  Sign: the sum WITHOUT the fold minus the sum with
        it.  The call is never cut into chunks of test points (sums over chunks would not be bitwise chunk-invariant): a work
        area above ``max_bytes`` raises ``ValueError`` naming the bytes."""
        lead, m, th = self._lead, self._check_xs(Xs), self._theta(theta)
        P, mode = int(nperiods), int(mode)
        if mode not in (MODE_LINEAR, MODE_LOG):
            raise ValueError(f"mode must be {MODE_LINEAR} (linear) or {MODE_LOG} (log)")

        def launch(order, start, nfolds, max_fold):
            need = int(self.lib.dgp_deletion_influence_workspace_bytes(self._h, m, nfolds, max_fold, P))
            if need == 0:
                raise ValueError(f"bad size: m = {m}, nfolds = {nfolds}, max_fold = {max_fold}, nperiods = {P} "
                                 "(1 <= m <= 2^20, 1 <= nfolds, max_fold <= n, 1 <= nperiods <= 65535)")
            if max_bytes is not None and need > int(max_bytes):
                raise ValueError(f"the influence of {nfolds} folds on m = {m} points at n = {self.n} (batch {self.batch}) needs a "
                                 f"work area of {need} bytes, which exceeds max_bytes = {int(max_bytes)}")
            dev = self.device
            with torch.cuda.device(dev):
                _mu, a_t, g_t, _ev, s_t = _moment_inputs(dev, self.dtype, lead, m, None, a, periods, None, scale)
                sd_t = None if inv_sd is None else torch.as_tensor(inv_sd).to(dev, torch.float64).contiguous()
                if sd_t is not None and tuple(sd_t.shape) != lead + (m,):
                    raise ValueError(f"inv_sd must have shape {lead + (m,)}")
                work = self._work_area("_influence_ws", need, "dgp_deletion_influence", check_free=True)
                order, start, xs = order.to(dev).contiguous(), start.to(dev).contiguous(), Xs.contiguous()
                dload = self._empty(nfolds, P, dtype=torch.float64)
                dvar = torch.empty_like(dload) if mode == MODE_LINEAR else None
                shift = self._empty(nfolds, dtype=torch.float64) if sd_t is not None else None
                info = self._empty(nfolds, dtype=torch.int32)
                self._call("dgp_deletion_influence", th, _ptr(xs), m, _ptr(order), _ptr(start), nfolds, max_fold, mode, _ptr(a_t),
                           _ptr(s_t), _ptr(g_t), P, _ptr(sd_t), work, need, _ptr(dload), _ptr(dvar), _ptr(shift), _ptr(info))
            return dload, dvar, shift, info

        return cross_validate_folds(self, groups, launch, max_group)

    def whiten(self, cols: torch.Tensor, site: int = 0):
        """L^-1 cols through the inverse factor T the plan holds, for the few columns of a prior-mean Jacobian:
        (L^-1 J)^T (L^-1 J) = J^T K^^-1 J, the mean block of the Fisher information.  ``cols`` (n_site, k) on the device
        -> (n_site, k) float64.  One triangular n x n by n x k product; reads T only."""
        ns = self._site_sizes[site]
        if not (torch.is_tensor(cols) and cols.is_cuda and cols.dim() == 2 and cols.shape[0] == ns):
            raise ValueError(f"cols must be a ({ns}, k) CUDA tensor")
        with torch.cuda.device(self.device):
            T = torch.tril(self.buffer(_lib.BUF_T, site)[:ns, :ns]).double()
            return T @ cols.double()

    # ------------------------------------------------------------------ sample(): posterior covariance, factor, draws
    def _jitter_ladder(self):
        """linear_operator's ``psd_safe_cholesky`` policy: first no jitter at all, then the
        dtype's default (1e-8 fp64 / 1e-6 fp32), then 10x and 100x that; after that it raises."""
        base = 1e-8 if self.dtype == torch.float64 else 1e-6
        return (0.0, base, 10 * base, 100 * base)

    def posterior_cov(self, theta, Xs: torch.Tensor):
        """(K*^T alpha, latent posterior covariance K** - V^T V) at Xs (m, d): the covariance as an (M, M) tensor,
        M = padded m, lower triangle valid (diagonal 128-blocks complete), identity pad -- ``dgp_posterior_cov``.
        Batched plans: Xs (batch, m, d), theta (batch, ntheta) -> mean (batch, m), cov (batch, M, M), one launch sequence."""
        m, th = self._check_xs(Xs), self._theta(theta)
        M = int(self.lib.dgp_padded_n(m))
        with torch.cuda.device(self.device):
            xs = Xs.contiguous()
            work = self._sized_work("_pred_ws", "prediction", "dgp_predict_workspace_bytes", m)
            mean, cov = self._empty(m), self._empty(M, M)
            self._call("dgp_posterior_cov", th, _ptr(xs), m, *work, _ptr(mean), _ptr(cov))
        return mean, cov

    def psd_safe_factor(self, cov: torch.Tensor, m: int, ladder=None):
        """Lower Cholesky factor of the (M, M) matrix ``cov`` (layout of ``posterior_cov``; left untouched) by the
        blocked HIP potrf of an order-m plan, with ``psd_safe_cholesky``'s jitter policy: the matrix itself first, then
        + 1e-8 I, 1e-7 I, 1e-6 I (fp32: 1e-6 .. 1e-4), each attempt restarting from the kept matrix; raises after the
        last.  -> (Lbuf, jitter): Lbuf is that plan's (M, M) buffer -- zeros above the diagonal inside the diagonal
        128-blocks, identity pad, blocks above the block diagonal undefined -- valid until the next call.  ``ladder``: other
        jitters to try in order (``extremes`` factors a float32 plan's covariance in float64 with the float32 ladder: the
        matrix carries float32 rounding, which 1e-6 does not cover)."""
        M = int(self.lib.dgp_padded_n(m))
        if tuple(cov.shape) != (M, M) or cov.dtype != self.dtype or not cov.is_cuda or not cov.is_contiguous():
            raise ValueError(f"cov must be a contiguous ({M}, {M}) {self.dtype} CUDA tensor")
        fac = getattr(self, "_fac", None)  # the order-m plan whose potrf factors the covariance; kept between calls
        if fac is None or fac.n != m:
            self._fac = None
            self._fac = fac = GPPlan(self.model, m, self.d, dtype=self.dtype, device=self.device)
        Lbuf = fac.buffer(_lib.BUF_A)
        info = -1
        with torch.cuda.device(self.device):
            for jitter in (self._jitter_ladder() if ladder is None else tuple(ladder)):
                Lbuf.copy_(cov)
                if jitter:
                    Lbuf.diagonal()[:m].add_(jitter)
                fac.stage_potrf()
                info = fac.potrf_info()
                if info == 0:
                    return Lbuf, jitter
        raise RuntimeError(f"posterior covariance not positive definite after jitter {jitter:g} (pivot {info})")

    def posterior_factor(self, theta, Xs: torch.Tensor):
        """-> (K*^T alpha, Lbuf, jitter): ``posterior_cov`` followed by ``psd_safe_factor``."""
        mean, cov = self.posterior_cov(theta, Xs)
        Lbuf, jitter = self.psd_safe_factor(cov, Xs.shape[0])
        return mean, Lbuf, jitter

    def sample_draws(self, Lbuf: torch.Tensor, m: int, mean, ndraw: int, generator=None):
        """(ndraw, m) draws mean + L z, z ~ N(0, I), through ``dgp_sample_draws`` (one MFMA launch on the factor as
        ``psd_safe_factor`` leaves it).  The normals come from torch's generator (plumbing); ``self._last_z`` keeps
        them for the tests."""
        M = int(self.lib.dgp_padded_n(m))
        Q = int(self.lib.dgp_padded_n(ndraw))
        if tuple(Lbuf.shape) != (M, M) or Lbuf.dtype != self.dtype or not Lbuf.is_contiguous():
            raise ValueError(f"Lbuf must be the contiguous ({M}, {M}) factor buffer")
        with torch.cuda.device(self.device):
            z = torch.randn(M, Q, dtype=self.dtype, device=self.device, generator=generator)
            out = torch.empty(ndraw, m, dtype=self.dtype, device=self.device)
            mp = _ptr(mean.contiguous() if mean is not None else None)
            _call("dgp_sample_draws", _DTYPES[self.dtype], _ptr(Lbuf), m, _ptr(z), ndraw, mp, _ptr(out))
        self._last_z = z
        return out

    def period_moments(self, cov, m: int, mu, scale2, w, groups, ngroups: int, mode: int, extra_var=None):
        """The module-level ``period_moments``."""
        return period_moments(cov, m, mu, scale2, w, groups, ngroups, mode, extra_var)

    def period_third_moments(self, cov, m: int, mu, scale2, w, groups, ngroups: int, extra_var=None, tile: int = 0):
        """The module-level ``period_third_moments``."""
        return period_third_moments(cov, m, mu, scale2, w, groups, ngroups, extra_var, tile)

    def exceedance_moments(self, cov, m: int, mu, thresh, w, groups, ngroups: int, extra_var=None):
        """The module-level ``exceedance_moments``."""
        return exceedance_moments(cov, m, mu, thresh, w, groups, ngroups, extra_var)

    def excess_moments(self, cov, m: int, mu, scale2, thresh, w, groups, ngroups: int, above: bool = True, extra_var=None):
        """The module-level ``excess_moments``."""
        return excess_moments(cov, m, mu, scale2, thresh, w, groups, ngroups, above, extra_var)

    def window_moments(self, cov, m: int, mu, lo, hi, a=None, mode: int = 0, scale2=None):
        """The module-level ``window_moments``."""
        return window_moments(cov, m, mu, lo, hi, a=a, mode=mode, scale2=scale2)

    def window_variances(self, cov, m: int, mu, lo, hi, a=None, mode: int = 0, scale2=None):
        """The module-level ``window_variances``."""
        return window_variances(cov, m, mu, lo, hi, a=a, mode=mode, scale2=scale2)

    def orthant_probability(self, L, m: int, lo, hi, npoints: int = 4096, nshifts: int = 16, seed: int = 0, max_bytes=None):
        """The module-level ``orthant_probability``; ``self._orthant_hook``, when set, is its ``hook`` (the tests capture the
        device's own factor and limits through it, the way ``sample_draws`` keeps ``_last_z``)."""
        return orthant_probability(L, m, lo, hi, npoints=npoints, nshifts=nshifts, seed=seed, max_bytes=max_bytes,
                                   hook=getattr(self, "_orthant_hook", None))

    def path_counts(self, L, m: int, thr, above: bool = True, link=None, npoints: int = 4096, nshifts: int = 16, seed: int = 0,
                    max_bytes=None):
        """The module-level ``path_counts``; ``self._counts_hook``, when set, is its ``hook``."""
        return path_counts(L, m, thr, above=above, link=link, npoints=npoints, nshifts=nshifts, seed=seed, max_bytes=max_bytes,
                           hook=getattr(self, "_counts_hook", None))

    def sample_value(self, cov, m: int, a, scale2, groups, ngroups: int, obs_var=None, rows=None, nterms=None):
        """The module-level ``sample_value``."""
        return sample_value(cov, m, a, scale2, groups, ngroups, obs_var=obs_var, rows=rows, nterms=nterms)

    def posterior_period_moments(self, theta, Xs: torch.Tensor, mu, scale2, w, groups, ngroups: int, mode: int, extra_var=None):
        """``period_moments`` of the posterior at Xs straight from the held factorisation (``dgp_posterior_period_moments``):
        the (M, M) covariance is never formed.  Xs (m, d) -- (batch, m, d) for a batched plan, theta (batch, ntheta) --; the
        other arguments as for ``period_moments``.  The work area (2 N M plan-dtype elements + M P doubles per site) is kept
        between calls; a ``RuntimeError`` names its bytes when it exceeds the free device memory."""
        lead, m, th = self._lead, self._check_xs(Xs), self._theta(theta)
        P = int(ngroups)
        need = int(self.lib.dgp_posterior_period_moments_workspace_bytes(self._h, m, P))
        if need == 0:
            raise ValueError(f"bad size: m = {m}, ngroups = {P} (1 <= m <= 2^20, 1 <= ngroups <= 65535)")
        dev = self.device
        with torch.cuda.device(dev):
            mu_t, w_t, g_t, ev_t, s2 = _moment_inputs(dev, self.dtype, lead, m, mu, w, groups, extra_var, scale2)
            work = self._work_area("_ppm_ws", need, "dgp_posterior_period_moments", check_free=True)
            xs = Xs.contiguous()
            mean_out, cov_out = self._empty(P, dtype=torch.float64), self._empty(P, P, dtype=torch.float64)
            self._call("dgp_posterior_period_moments", th, _ptr(xs), m, int(mode), _ptr(mu_t), _ptr(s2), _ptr(w_t), _ptr(g_t), P,
                       _ptr(ev_t), work, need, _ptr(mean_out), _ptr(cov_out))
        return mean_out, cov_out

    def posterior_exceedance_moments(self, theta, Xs: torch.Tensor, mu, thresh, w, groups, ngroups: int, extra_var=None,
                                     panel_rows=None, max_bytes=None):
        """``exceedance_moments`` of the posterior at Xs straight from the held factorisation
        (``dgp_posterior_exceedance_moments``): the covariance is produced ``panel_rows`` rows at a time and the (M, M) matrix
        is never formed.  Xs (m, d) -- (batch, m, d) for a batched plan, theta (batch, ntheta) --; ``mu``, ``thresh`` (L, m)
        with 1 <= L <= 64, ``w``, ``groups``, ``ngroups``, ``extra_var`` and the results as for ``exceedance_moments``.
        ``panel_rows``: a positive multiple of 128, or None: ``exceedance_panel_rows`` of ``max_bytes`` -- the largest panel,
        at most M rows, whose work area fits; a ``ValueError`` names the bytes when 128 rows do not.  Short panels cost time:
        every chunk of 8 levels produces all panels again (N m^2 matrix-core flop per chunk), and a panel launch only has the
        parallelism of its own rows -- measured 3 x the dense path's time with 512-row panels at m = 14 610 (EXPERIMENTS.md) --
        so give ``max_bytes`` what the device can spare, above all with many levels.  The work area (2 N M + R M plan-dtype elements and M P min(L, 8) + 2 M (L + 1) doubles per
        site) is kept between calls; a ``RuntimeError`` names its bytes when it exceeds the free device memory."""
        lead, m, th = self._lead, self._check_xs(Xs), self._theta(theta)
        P = int(ngroups)
        dev = self.device
        with torch.cuda.device(dev):
            mu_t, w_t, g_t, ev_t, _ = _moment_inputs(dev, self.dtype, lead, m, mu, w, groups, extra_var)
            u_t = _row_matrix(thresh, "thresh", "L", lead, m, dev)
            L = int(u_t.shape[-2])
            R, work, need = self._stream_work("_pex_ws", "dgp_posterior_exceedance_moments", (m, P, L), panel_rows,
                                              lambda: self.exceedance_panel_rows(m, P, L, max_bytes), _levels_bad_size(m, P, L))
            xs = Xs.contiguous()
            mean_out, cov_out = self._empty(L, P, dtype=torch.float64), self._empty(L, P, P, dtype=torch.float64)
            self._call("dgp_posterior_exceedance_moments", th, _ptr(xs), m, _ptr(mu_t), _ptr(u_t), L, _ptr(w_t), _ptr(g_t), P,
                       _ptr(ev_t), R, work, need, _ptr(mean_out), _ptr(cov_out))
        return mean_out, cov_out

    def exceedance_panel_rows(self, m: int, ngroups: int, nlevels: int, max_bytes=None) -> int:
        """The panel height ``posterior_exceedance_moments`` picks for m points, ``ngroups`` groups and ``nlevels`` levels under
        ``max_bytes`` (default ``loads.DEFAULT_MAX_BYTES``): ``stream_panel_rows`` on the sizes
        ``dgp_posterior_exceedance_moments_workspace_bytes`` reports."""
        return self._linear_panel_rows("dgp_posterior_exceedance_moments", (m, ngroups, nlevels), max_bytes,
                                       _levels_bad_size(m, ngroups, nlevels), "the streamed exceedance pass")

    def posterior_excess_moments(self, theta, Xs: torch.Tensor, mu, scale2, thresh, w, groups, ngroups: int, above: bool = True,
                                 extra_var=None, panel_rows=None, max_bytes=None):
        """``excess_moments`` of the posterior at Xs straight from the held factorisation (``dgp_posterior_excess_moments``):
        the covariance is produced ``panel_rows`` rows at a time and the (M, M) matrix is never formed.  Xs (m, d) --
        (batch, m, d) for a batched plan, theta (batch, ntheta) --; ``mu`` (the MAPPED mean), ``scale2``, ``thresh`` = ln tau
        (L, m) with 1 <= L <= 64, ``w``, ``groups``, ``ngroups``, ``above``, ``extra_var`` and the results (mean, cov, total) as
        for ``excess_moments``.  ``panel_rows``: a positive multiple of 128, or None: ``excess_panel_rows`` of ``max_bytes`` --
        the largest panel, at most M rows, whose work area fits; a ``ValueError`` names the bytes when 128 rows do not.  Short
        panels cost time: every group of 8 levels produces all panels again, and a panel launch only has the parallelism of its
        own rows, so give ``max_bytes`` what the device can spare.  The work area (2 N M + R M plan-dtype elements and
        M (3 + 6 L + P min(L, 8)) + P doubles per site) is kept between calls; a ``RuntimeError`` names its bytes when it
        exceeds the free device memory."""
        lead, m, th = self._lead, self._check_xs(Xs), self._theta(theta)
        P = int(ngroups)
        dev = self.device
        with torch.cuda.device(dev):
            mu_t, w_t, g_t, ev_t, s2 = _moment_inputs(dev, self.dtype, lead, m, mu, w, groups, extra_var, scale2)
            a_t = _row_matrix(thresh, "thresh", "L", lead, m, dev)
            L = int(a_t.shape[-2])
            R, work, need = self._stream_work("_pxs_ws", "dgp_posterior_excess_moments", (m, P, L), panel_rows,
                                              lambda: self.excess_panel_rows(m, P, L, max_bytes), _levels_bad_size(m, P, L))
            xs = Xs.contiguous()
            mean_out, cov_out = self._empty(L, P, dtype=torch.float64), self._empty(L, P, P, dtype=torch.float64)
            total_out = self._empty(P, dtype=torch.float64)
            self._call("dgp_posterior_excess_moments", th, _ptr(xs), m, _ptr(mu_t), _ptr(s2), _ptr(a_t), L, _ptr(w_t), _ptr(g_t), P,
                       _ptr(ev_t), int(bool(above)), R, work, need, _ptr(mean_out), _ptr(cov_out), _ptr(total_out))
        return mean_out, cov_out, total_out

    def excess_panel_rows(self, m: int, ngroups: int, nlevels: int, max_bytes=None) -> int:
        """The panel height ``posterior_excess_moments`` picks for m points, ``ngroups`` groups and ``nlevels`` levels under
        ``max_bytes`` (default ``loads.DEFAULT_MAX_BYTES``): ``stream_panel_rows`` on the sizes
        ``dgp_posterior_excess_moments_workspace_bytes`` reports."""
        return self._linear_panel_rows("dgp_posterior_excess_moments", (m, ngroups, nlevels), max_bytes,
                                       _levels_bad_size(m, ngroups, nlevels), "the streamed excess pass")

    _SV_SIZES = ("(1 <= m <= 2^20, 1 <= ngroups <= 65535, 0 <= nrows <= 64, 1 <= nterms <= 64)")

    def posterior_sample_value(self, theta, Xs: torch.Tensor, a, scale2, groups, ngroups: int, obs_var=None, rows=None, nterms=None,
                               panel_rows=None, max_bytes=None):
        """``sample_value`` of the posterior at Xs straight from the held factorisation (``dgp_posterior_sample_value``): the
        covariance is produced ``panel_rows`` rows at a time and the (M, M) matrix is never formed.  Xs (m, d) -- (batch, m, d)
        for a batched plan, theta (batch, ntheta) --; ``a``, ``scale2``, ``groups``, ``ngroups``, ``obs_var`` (the plan's dtype),
        ``rows`` and the results (gain, var) as for ``sample_value``.  C_cc is the predicted variance, never a panel's diagonal.
        ``nterms``: the series length; None picks ``series_terms`` of s^2 max predicted variance over the included days (one
        ``predict``).  ``panel_rows``: a positive multiple of 128, or None: ``sample_value_panel_rows`` of ``max_bytes`` -- the
        largest panel, at most M rows, whose work area fits; a ``ValueError`` names the bytes when 128 rows do not.  The work
        area (2 N M + R M plan-dtype elements and M (2 + P K) + P doubles per site) is kept between calls; a ``RuntimeError``
        names its bytes when it exceeds the free device memory."""
        lead, m, th = self._lead, self._check_xs(Xs), self._theta(theta)
        P = int(ngroups)
        dev = self.device
        with torch.cuda.device(dev):
            _, a_t, g_t, ov_t, s2 = _moment_inputs(dev, self.dtype, lead, m, None, a, groups, obs_var, scale2)
            rows_t = None if rows is None else _row_matrix(rows, "rows", "nrows", lead, m, dev)
            nrows = 0 if rows_t is None else int(rows_t.shape[-2])
            if nrows == 0:
                rows_t = None
            if nterms is None:
                var = self.predict(theta, Xs)[1].double()
                top = torch.where(g_t >= 0, var, torch.zeros_like(var)).reshape(self.batch, -1).amax(dim=1)
                nterms = series_terms(float((s2 * top).max()))
            K = int(nterms)
            bad_size = f"bad size: m = {m}, ngroups = {P}, nrows = {nrows}, nterms = {K} {self._SV_SIZES}"
            if int(self.lib.dgp_posterior_sample_value_workspace_bytes(self._h, m, P, nrows, K, 128)) == 0:
                raise ValueError(bad_size)  # (before panel_rows is looked at)
            R, work, need = self._stream_work("_psv_ws", "dgp_posterior_sample_value", (m, P, nrows, K), panel_rows,
                                              lambda: self.sample_value_panel_rows(m, P, nrows, K, max_bytes), bad_size)
            xs = Xs.contiguous()
            gain, var_out = self._empty(P, m, dtype=torch.float64), self._empty(m, dtype=torch.float64)
            self._call("dgp_posterior_sample_value", th, _ptr(xs), m, _ptr(a_t), _ptr(s2), _ptr(g_t), P, _ptr(ov_t), _ptr(rows_t), nrows,
                       K, R, work, need, _ptr(gain), _ptr(var_out))
        return gain, var_out

    def sample_value_panel_rows(self, m: int, ngroups: int, nrows: int, nterms: int, max_bytes=None) -> int:
        """The panel height ``posterior_sample_value`` picks for m points, ``ngroups`` groups, ``nrows`` conditioning rows and
        ``nterms`` series terms under ``max_bytes`` (default ``loads.DEFAULT_MAX_BYTES``): ``stream_panel_rows`` on the sizes
        ``dgp_posterior_sample_value_workspace_bytes`` reports."""
        return self._linear_panel_rows("dgp_posterior_sample_value", (m, ngroups, nrows, nterms), max_bytes,
                                       f"bad size: m = {m}, ngroups = {ngroups}, nrows = {nrows}, nterms = {nterms} {self._SV_SIZES}",
                                       "the streamed value of samples")

    def posterior_cov_columns(self, theta, Xs: torch.Tensor, idx):
        """Columns C[:, idx] of the latent posterior covariance at Xs (``dgp_posterior_cov_columns``) as (ncols, m) float64 --
        (batch, ncols, m) for a batched plan, ``idx`` (batch, ncols) --, 1 <= ncols <= 64 indices in 0 .. m-1, from the held
        factorisation: the prediction's front end plus one read of V per column.  The dense matrix is never formed."""
        lead, m, th = self._lead, self._check_xs(Xs), self._theta(theta)
        idx_t = torch.as_tensor(idx).to(torch.int64).reshape(lead + (-1,)) if lead else torch.as_tensor(idx).to(torch.int64).reshape(-1)
        ncols = int(idx_t.shape[-1])
        if not 1 <= ncols <= 64:
            raise ValueError(f"posterior_cov_columns takes 1 .. 64 columns, not {ncols}")
        if int(idx_t.min()) < 0 or int(idx_t.max()) >= m:
            raise ValueError(f"column index out of range for {m} points")
        need = int(self.lib.dgp_posterior_cov_columns_workspace_bytes(self._h, m, ncols))
        if need == 0:
            raise ValueError(f"bad size: m = {m}, ncols = {ncols} (1 <= m <= 2^20, 1 <= ncols <= 64)")
        with torch.cuda.device(self.device):
            i32 = idx_t.to(self.device, torch.int32).contiguous()
            work = self._work_area("_pcc_ws", need, "dgp_posterior_cov_columns", check_free=True)
            xs = Xs.contiguous()
            cols = self._empty(ncols, m, dtype=torch.float64)
            self._call("dgp_posterior_cov_columns", th, _ptr(xs), m, _ptr(i32), ncols, work, need, _ptr(cols))
        return cols

    def posterior_cov_block(self, theta, Xs: torch.Tensor, row0: int, row1: int, col0: int):
        """Rows [row0, row1) x columns [col0, row1) of the latent posterior covariance at Xs (``dgp_posterior_cov_block``) as a
        (row1 - row0, row1 - col0) tensor in the plan's dtype -- with a leading batch dimension for a batched plan --, from the
        held factorisation: a block of the covariance of a record too long to hold whole.  ``row0``, ``row1``, ``col0``:
        multiples of 128 with 0 <= col0 <= row0 < row1 <= M (M = padded m).  Entry [r, c] is C[row0 + r, col0 + c] with the bits
        ``posterior_cov`` gives it (float64); 128 x 128 tiles above the diagonal are not written (they hold zeros here), and
        inside a diagonal tile the entries on and below the diagonal are valid."""
        m, th = self._check_xs(Xs), self._theta(theta)
        row0, row1, col0 = int(row0), int(row1), int(col0)
        need = int(self.lib.dgp_posterior_cov_block_workspace_bytes(self._h, m, row0, row1, col0))
        if need == 0:
            raise ValueError(f"bad block: rows [{row0}, {row1}), first column {col0} for m = {m} (multiples of 128 with "
                             "0 <= col0 <= row0 < row1 <= padded m, 1 <= m <= 2^20)")
        with torch.cuda.device(self.device):
            xs = Xs.contiguous()
            work = self._work_area("_pcb_ws", need, "dgp_posterior_cov_block", check_free=True)
            out = torch.zeros(self._lead + (row1 - row0, row1 - col0), dtype=self.dtype, device=self.device)
            self._call("dgp_posterior_cov_block", th, _ptr(xs), m, row0, row1, col0, work, need, _ptr(out))
        return out

    def posterior_window_variances(self, theta, Xs: torch.Tensor, mu, lo, hi, a=None, mode: int = 0, scale2=None, panel_rows=None,
                                   max_bytes=None):
        """``window_variances`` of the posterior at Xs straight from the held factorisation
        (``dgp_posterior_window_variances``): only a band of the covariance is produced, ``panel_rows`` rows at a time -- the
        panel of rows [p0, p1) holds the columns from 128 floor(max(0, p0 - reach + 1) / 128) on, ``reach`` = the largest point
        count of a window, computed here from ``lo`` / ``hi`` -- and the (M, M) matrix is never formed.  Xs (m, d) --
        (batch, m, d) for a batched plan, theta (batch, ntheta) --; ``mu`` (the plan's dtype; MODE_LOG: the MAPPED mean), ``lo``,
        ``hi``, ``a``, ``mode``, ``scale2`` and the results (mean, var) as for ``window_variances``.  C_jj is the predicted
        variance, never a panel's diagonal.  ``panel_rows``: a positive multiple of 128, or None: ``window_panel_rows`` of
        ``max_bytes`` -- the largest panel, at most M rows, whose work area fits; a ``ValueError`` names the bytes when 128 rows
        do not.  The work area (2 N M + R (R + round_up(reach, 128)) plan-dtype elements and 3 M + 3 Q doubles per site) is kept
        between calls; a ``RuntimeError`` names its bytes when it exceeds the free device memory."""
        lead, m, th = self._lead, self._check_xs(Xs), self._theta(theta)
        lo_h, hi_h, q = _window_bounds(lo, hi, lead, m)
        _window_mode(mode, scale2)
        reach = max(1, int((hi_h - lo_h).max()))
        dev = self.device
        with torch.cuda.device(dev):
            mu_t, a_t, _g, _ev, s2 = _moment_inputs(dev, self.dtype, lead, m, mu, a, None, None, scale2 if mode == MODE_LOG else None)
            R, work, need = self._stream_work("_pwv_ws", "dgp_posterior_window_variances", (m, q, reach), panel_rows,
                                              lambda: self.window_panel_rows(m, q, reach, max_bytes),
                                              f"bad size: m = {m}, q = {q} (1 <= m, q <= 2^20)")
            xs = Xs.contiguous()
            lo_t, hi_t = lo_h.to(dev), hi_h.to(dev)
            mean_out, var_out = self._empty(q, dtype=torch.float64), self._empty(q, dtype=torch.float64)
            self._call("dgp_posterior_window_variances", th, _ptr(xs), m, _ptr(mu_t), _ptr(s2), _ptr(a_t), _ptr(lo_t), _ptr(hi_t), q,
                       int(mode), reach, R, work, need, _ptr(mean_out), _ptr(var_out))
        return mean_out, var_out

    def window_panel_rows(self, m: int, q: int, reach: int, max_bytes=None) -> int:
        """The panel height ``posterior_window_variances`` picks for m points, q windows of at most ``reach`` points under
        ``max_bytes`` (default ``loads.DEFAULT_MAX_BYTES``).  The band of R x (R + round_up(reach, 128)) elements grows
        quadratically in R, so ``stream_panel_rows``' linear rule does not apply: a bisection on the sizes
        ``dgp_posterior_window_variances_workspace_bytes`` reports for the largest multiple of 128, at most the padded record
        length M, whose work area fits.  ``ValueError`` naming the bytes when 128 rows do not fit."""
        size, max_bytes = self._panel_sizes("dgp_posterior_window_variances", (m, q, reach), max_bytes,
                                            f"bad size: m = {m}, q = {q}, reach = {reach} (1 <= m, q, reach <= 2^20)")
        need128 = size(128)
        if need128 > max_bytes:
            raise ValueError(f"the streamed rolling-mean pass needs a work area of {need128} bytes with the smallest panel (128 "
                             f"rows), which exceeds max_bytes = {max_bytes}")
        good, bad = 1, int(self.lib.dgp_padded_n(int(m))) // 128 + 1  # in blocks of 128 rows: size(good) fits, size(bad) does not
        while bad - good > 1:
            mid = (good + bad) // 2
            if size(128 * mid) <= max_bytes:
                good = mid
            else:
                bad = mid
        return 128 * good

    def lowrank_period_moments(self, rows, m: int, mu, scale2, w, groups, ngroups: int, mode: int):
        """The module-level ``lowrank_period_moments``."""
        return lowrank_period_moments(rows, m, mu, scale2, w, groups, ngroups, mode)

    def predict_mean(self, theta, Xs: torch.Tensor):
        """K(X*, X) alpha from the held factorisation (no variance work).  Batched plans: Xs (batch, m, d) -> (batch, m)."""
        th, m = self._theta(theta), self._check_xs(Xs)
        with torch.cuda.device(self.device):
            xs = Xs.contiguous()
            work = self._sized_work("_vjp_ws", "mean / vjp", "dgp_mean_vjp_workspace_bytes", m)
            mean = self._empty(m)
            self._call("dgp_predict_mean", th, _ptr(xs), m, *work, _ptr(mean))
        return mean

    def mean_vjp(self, theta, Xs: torch.Tensor, w: torch.Tensor):
        """Vector-Jacobian product of ``predict_mean``: (dtheta[P], dr[n], dnoise[n]) for upstream w[m].  Batched plans:
        Xs (batch, m, d), w (batch, m) -> dtheta (batch, P), dr (batch, n), dnoise (batch, n), one launch sequence for all sites."""
        th, m = self._theta(theta), self._check_xs(Xs)
        self._check_vec(w, "w", m)
        with torch.cuda.device(self.device):
            xs = Xs.contiguous()
            work = self._sized_work("_vjp_ws", "mean / vjp", "dgp_mean_vjp_workspace_bytes", m)
            width = _lib.OUT_LEN if self.batch == 1 else self.ntheta
            dtheta = torch.zeros(self._lead + (width,), dtype=self.dtype, device=self.device)
            dr, dnoise = self._empty(self.n), self._empty(self.n)
            self._call("dgp_mean_vjp", th, _ptr(xs), m, _ptr(w), *work, _ptr(dtheta), _ptr(dr), _ptr(dnoise))
        return dtheta[..., : self.ntheta], dr, dnoise

    def potrf_info(self) -> int:
        """info of the last factorisation (0 = ok, k = first non-positive pivot), synchronising."""
        off = self._info_offset()
        return int(self._ws[off:off + 4].view(torch.int32)[0].item())

    def _info_offset(self):
        p, ld = C.c_void_p(), C.c_int64()
        self._host("dgp_plan_buffer", _lib.BUF_INFO, C.byref(p), C.byref(ld))
        return p.value - self._ws.data_ptr()

    def set_timing(self, enabled: bool):
        self._host("dgp_plan_set_timing", int(bool(enabled)))

    def get_timing(self):
        """Per-stage HIP-event milliseconds of the most recent fit step (include/dgp_hip.h DGP_TIME_*)."""
        ms = (C.c_double * _lib.TIME_COUNT)()
        self._host("dgp_plan_get_timing", ms)
        return list(ms)

    # ------------------------------------------------------------------ single stages (tests, profiling)
    def _stage(self, name, *args):
        with torch.cuda.device(self.device):
            self._call("dgp_stage_" + name, *args)

    def stage_gram(self, theta, noise):
        self._check_vec(noise, "noise")
        self._stage("gram", self._theta(theta), _ptr(noise))

    def stage_potrf(self):
        self._stage("potrf")

    def stage_trtri(self):
        self._stage("trtri")

    def stage_lauum(self):
        self._stage("lauum")

    def stage_solve(self, r):
        self._check_vec(r, "r")
        self._stage("solve", _ptr(r))

    def stage_grad(self, theta):
        with torch.cuda.device(self.device):
            out = torch.zeros(_lib.OUT_LEN, dtype=self.dtype, device=self.device)
            self._call("dgp_stage_grad", _theta_array(theta, self.ntheta), _ptr(out))
        return out[: self.ntheta]

    def cross_gram(self, theta, Xs):
        m = Xs.shape[0]
        M = int(self.lib.dgp_padded_n(m))
        with torch.cuda.device(self.device):
            work = torch.empty(self.d * M, dtype=self.dtype, device=self.device)
            Ks = torch.empty(self.N, M, dtype=self.dtype, device=self.device)
            xs = Xs.contiguous()
            self._call("dgp_cross_gram", _theta_array(theta, self.ntheta), _ptr(xs), m, _ptr(work), _ptr(Ks))
        return Ks[: self.n, :m]


MODE_LINEAR, MODE_LOG = 0, 1


def _moment_inputs(dev, dtype, lead, m, mu, w, groups, extra_var, scale2=None):
    """The per-point inputs of the moment passes as contiguous device tensors of shape ``lead + (m,)``: -> (mu in ``dtype``, w
    in float64, groups in int32, extra_var in ``dtype`` or None, scale2 as one float64 per site, or None when not given)."""

    def vec(t, name, dt):
        if t is None:
            return None
        t = torch.as_tensor(t).to(dev, dt).contiguous()
        if tuple(t.shape) != lead + (m,):
            raise ValueError(f"{name} must have shape {lead + (m,)}")
        return t

    mu_t, w_t = vec(mu, "mu", dtype), vec(w, "w", torch.float64)
    g_t, ev_t = vec(groups, "groups", torch.int32), vec(extra_var, "extra_var", dtype)
    s2 = None
    if scale2 is not None:
        B = lead[0] if lead else 1
        s2 = torch.as_tensor(scale2, dtype=torch.float64).reshape(-1).to(dev).contiguous()
        if s2.numel() != B:
            raise ValueError(f"scale2 must hold {B} value(s)")
    return mu_t, w_t, g_t, ev_t, s2


def _cov_layout(cov, m):
    """The covariance argument of the stateless moment passes, (M, M) or (B, M, M) with M = padded m: -> (lib, lead, B,
    dev), ``lead`` = () or (B,).  ``ValueError`` unless it is a contiguous float64 / float32 device tensor of that shape."""
    lib = _lib.load()
    lead = (cov.shape[0],) if cov.dim() == 3 else ()
    M = int(lib.dgp_padded_n(int(m)))
    if cov.dtype not in _DTYPES or not cov.is_cuda or not cov.is_contiguous() or tuple(cov.shape) != lead + (M, M):
        raise ValueError(f"cov must be a contiguous {lead + (M, M)} float64 / float32 CUDA tensor")
    return lib, lead, (lead[0] if lead else 1), cov.device


def _row_matrix(t, name, rows, lead, m, dev):
    """``t`` as a contiguous float64 device tensor of shape ``lead + (rows, m)``, any number of rows; ``ValueError`` otherwise."""
    t = torch.as_tensor(t).to(dev, torch.float64).contiguous()
    if t.dim() != len(lead) + 2 or tuple(t.shape[:-2]) != lead or t.shape[-1] != m:
        raise ValueError(f"{name} must have shape {lead + (rows, m)}")
    return t


def period_moments(cov: torch.Tensor, m: int, mu: torch.Tensor, scale2, w: torch.Tensor, groups: torch.Tensor, ngroups: int,
                   mode: int, extra_var: torch.Tensor | None = None):
    """Exact mean and covariance of the period sums L_g = sum_{i in g} w_i c_i of a transformed latent posterior
    f ~ N(mu, C) -- c_i = exp(f'_i) (``mode`` = MODE_LOG) or c_i = f'_i (MODE_LINEAR) with f' = s f + t -- through one
    ``dgp_period_moments`` call (no factorisation, no draws).

    ``cov``: what ``GPPlan.posterior_cov`` returns -- (M, M), M = padded m, lower triangle and diagonal blocks valid -- or
    (B, M, M) for B sites; ``mu``: the MAPPED mean s mu + t, (m,) / (B, m), the dtype of ``cov``; ``scale2``: s^2, a
    number, or (B,) values; ``w``: weights (m,) / (B, m); ``groups``: int32 ids (m,) / (B, m) in 0 .. ngroups-1,
    non-decreasing except for -1 (excluded) anywhere; ``extra_var``: None or (m,) / (B, m) added to the diagonal of C.
    -> (mean (P,), cov (P, P)) or ((B, P), (B, P, P)), float64 device tensors."""
    lib, lead, B, dev = _cov_layout(cov, m)
    m, P = int(m), int(ngroups)
    with torch.cuda.device(dev):
        mu_t, w_t, g_t, ev_t, s2 = _moment_inputs(dev, cov.dtype, lead, m, mu, w, groups, extra_var, scale2)
        need = int(lib.dgp_period_moments_workspace_bytes(m, P, B))
        work = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        mean_out = torch.empty(lead + (P,), dtype=torch.float64, device=dev)
        cov_out = torch.empty(lead + (P, P), dtype=torch.float64, device=dev)
        _call("dgp_period_moments", _DTYPES[cov.dtype], int(mode), _ptr(cov), m, B, _ptr(mu_t), _ptr(s2), _ptr(w_t), _ptr(g_t), P,
              _ptr(ev_t), _ptr(work), need, _ptr(mean_out), _ptr(cov_out))
    return mean_out, cov_out


def lowrank_period_moments(rows: torch.Tensor, m: int, mu: torch.Tensor, scale2, w: torch.Tensor, groups: torch.Tensor, ngroups: int,
                           mode: int):
    """``period_moments`` on the low-rank covariance R = rows^T rows without ever forming R (``dgp_lowrank_period_moments``):
    ``rows`` (nrows, m) or (B, nrows, m) float64 on the device, 1 <= nrows <= 64 -- the conditioning rows of a sampling
    design, whose R is the covariance the samples explain; ``mu`` (the MAPPED mean; float64), ``scale2``, ``w``, ``groups``,
    ``ngroups``, ``mode`` as for ``period_moments``.  -> (mean (P,), cov (P, P)) or ((B, P), (B, P, P)), float64 device
    tensors; cov is exactly symmetric."""
    if not (torch.is_tensor(rows) and rows.is_cuda and rows.dtype == torch.float64 and rows.dim() in (2, 3) and rows.shape[-1] == int(m)
            and 1 <= rows.shape[-2] <= 64):
        raise ValueError(f"rows must be a float64 CUDA tensor of shape (nrows, {int(m)}) or (B, nrows, {int(m)}) with 1 <= nrows <= 64")
    lib = _lib.load()
    lead = (rows.shape[0],) if rows.dim() == 3 else ()
    B, dev = (lead[0] if lead else 1), rows.device
    m, P, nrows = int(m), int(ngroups), int(rows.shape[-2])
    with torch.cuda.device(dev):
        mu_t, w_t, g_t, _, s2 = _moment_inputs(dev, torch.float64, lead, m, mu, w, groups, None, scale2)
        need = int(lib.dgp_period_moments_workspace_bytes(m, P, B))
        if need == 0:
            raise ValueError(f"bad size: m = {m}, ngroups = {P}, batch = {B} (1 <= m <= 2^20, 1 <= ngroups <= 65535, 1 <= batch <= 1024)")
        rows_t = rows.contiguous()
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        mean_out = torch.empty(lead + (P,), dtype=torch.float64, device=dev)
        cov_out = torch.empty(lead + (P, P), dtype=torch.float64, device=dev)
        _call("dgp_lowrank_period_moments", int(mode), _ptr(rows_t), nrows, m, B, _ptr(mu_t), _ptr(s2), _ptr(w_t), _ptr(g_t), P,
              _ptr(work), need, _ptr(mean_out), _ptr(cov_out))
    return mean_out, cov_out


def period_third_moments(cov: torch.Tensor, m: int, mu: torch.Tensor, scale2, w: torch.Tensor, groups: torch.Tensor, ngroups: int,
                         extra_var: torch.Tensor | None = None, tile: int = 0):
    """Exact third central moment k3_g = E[(L_g - E L_g)^3] of the period sums of a LOG-transformed posterior
    (``period_moments``' setting with ``mode`` = MODE_LOG, and its arguments) through one ``dgp_period_third_moments`` call:
    skewness_g = k3_g / cov_gg^1.5.  ``tile``: 0 picks the tile core by size, 64 / 128 force one.  The work area -- 2 M^2
    doubles per site -- is allocated for the call.  -> k3 (P,) or (B, P), a float64 device tensor."""
    lib, lead, B, dev = _cov_layout(cov, m)
    m, P = int(m), int(ngroups)
    with torch.cuda.device(dev):
        mu_t, w_t, g_t, ev_t, s2 = _moment_inputs(dev, cov.dtype, lead, m, mu, w, groups, extra_var, scale2)
        need = int(lib.dgp_period_third_moments_workspace_bytes(m, P, B))
        work = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        k3 = torch.empty(lead + (P,), dtype=torch.float64, device=dev)
        _call("dgp_period_third_moments", _DTYPES[cov.dtype], _ptr(cov), m, B, _ptr(mu_t), _ptr(s2), _ptr(w_t), _ptr(g_t), P,
              _ptr(ev_t), int(tile), _ptr(work), need, _ptr(k3))
    return k3


def _levels_bad_size(m, ngroups, nlevels):
    return (f"bad size: m = {m}, ngroups = {ngroups}, levels = {nlevels} (1 <= m <= 2^20, 1 <= ngroups <= 65535, "
            "1 <= levels <= 64)")


def stream_panel_rows(need128: int, step: int, M: int, max_bytes: int, what: str = "the streamed exceedance pass") -> int:
    """Rows of the covariance panel ``GPPlan.posterior_exceedance_moments`` (``posterior_excess_moments``, which names itself
    in ``what`` for the error text) picks for a byte budget: the work area is
    ``need128`` bytes with a panel of 128 rows and grows by ``step`` bytes per further 128 rows (one panel row block of
    every site), so the answer is 128 min(M / 128, 1 + (max_bytes - need128) // step) -- the largest multiple of 128, at
    most the padded record length ``M``, whose work area fits ``max_bytes``.  ``ValueError`` naming the bytes when
    ``need128`` itself exceeds the budget."""
    if need128 > max_bytes:
        raise ValueError(f"{what} needs a work area of {need128} bytes with the smallest panel (128 "
                         f"rows), which exceeds max_bytes = {max_bytes}")
    blocks = M // 128
    if step > 0:
        blocks = min(blocks, 1 + (int(max_bytes) - need128) // step)
    return 128 * blocks


def exceedance_moments(cov: torch.Tensor, m: int, mu: torch.Tensor, thresh: torch.Tensor, w: torch.Tensor, groups: torch.Tensor,
                       ngroups: int, extra_var: torch.Tensor | None = None):
    """Exact mean and covariance of the counts N_g = sum_{i in g} w_i 1[f_i > u_i] of a latent posterior f ~ N(mu, C), per
    threshold level, through one ``dgp_exceedance_moments`` call (no factorisation, no draws): E N_g = sum w_i Phi(z_i),
    Cov(N_g, N_h) = sum w_i w_j (Phi2(z_i, z_j; rho_ij) - Phi(z_i) Phi(z_j)), z = (mu - u) / sigma.

    ``cov``: what ``GPPlan.posterior_cov`` returns -- (M, M), M = padded m, lower triangle and diagonal blocks valid -- or
    (B, M, M) for B sites; ``mu``: the MODEL-space mean, (m,) / (B, m), the dtype of ``cov``; ``thresh``: model-space
    thresholds, (L, m) / (B, L, m) with 1 <= L <= 64, +-inf allowed; ``w``: weights (m,) / (B, m); ``groups``: int32 ids
    (m,) / (B, m) in 0 .. ngroups-1, non-decreasing except for -1 (excluded) anywhere; ``extra_var``: None or (m,) / (B, m)
    added to the variances (never to the covariances).
    -> (mean (L, P), cov (L, P, P)) or ((B, L, P), (B, L, P, P)), float64 device tensors; levels do not interact."""
    lib, lead, B, dev = _cov_layout(cov, m)
    m, P = int(m), int(ngroups)
    with torch.cuda.device(dev):
        mu_t, w_t, g_t, ev_t, _ = _moment_inputs(dev, cov.dtype, lead, m, mu, w, groups, extra_var)
        u_t = _row_matrix(thresh, "thresh", "L", lead, m, dev)
        L = int(u_t.shape[-2])
        need = int(lib.dgp_exceedance_moments_workspace_bytes(m, P, L, B))
        if need == 0:
            raise ValueError(f"bad size: m = {m}, ngroups = {P}, levels = {L}, batch = {B} "
                             "(1 <= m <= 2^20, 1 <= ngroups <= 65535, 1 <= levels <= 64, 1 <= batch <= 1024)")
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        mean_out = torch.empty(lead + (L, P), dtype=torch.float64, device=dev)
        cov_out = torch.empty(lead + (L, P, P), dtype=torch.float64, device=dev)
        _call("dgp_exceedance_moments", _DTYPES[cov.dtype], _ptr(cov), m, B, _ptr(mu_t), _ptr(u_t), L, _ptr(w_t), _ptr(g_t), P,
              _ptr(ev_t), _ptr(work), need, _ptr(mean_out), _ptr(cov_out))
    return mean_out, cov_out


def excess_moments(cov: torch.Tensor, m: int, mu: torch.Tensor, scale2, thresh: torch.Tensor, w: torch.Tensor, groups: torch.Tensor,
                   ngroups: int, above: bool = True, extra_var: torch.Tensor | None = None):
    """Exact mean and covariance of the period sums E_g = sum_{i in g} w_i (c_i - tau_i)^+ -- ``above=False``: the deficit
    sum w_i (tau_i - c_i)^+ -- of a LOG-transformed latent posterior, c_i = exp(s f_i + t), f ~ N(mu, C), per threshold level,
    through one ``dgp_excess_moments`` call (no factorisation, no draws): the per-point mean is of Black-Scholes type, the
    covariance of two points a combination of four bivariate normal orthant probabilities (``include/dgp_hip_ext.h``).

    ``cov``, ``mu`` (the MAPPED mean s mu + t), ``scale2``, ``w``, ``groups``, ``ngroups``, ``extra_var``: as for
    ``period_moments`` with ``mode`` = MODE_LOG; ``thresh``: ln tau, (L, m) / (B, L, m) with 1 <= L <= 64, -inf (tau = 0: the
    excess is c_i itself, the deficit 0) and +inf allowed.
    -> (mean (L, P), cov (L, P, P), total (P,)) or with a leading B, float64 device tensors; ``total`` is the period's expected
    sum of w_i c_i (``period_moments``' mean); levels do not interact."""
    lib, lead, B, dev = _cov_layout(cov, m)
    m, P = int(m), int(ngroups)
    with torch.cuda.device(dev):
        mu_t, w_t, g_t, ev_t, s2 = _moment_inputs(dev, cov.dtype, lead, m, mu, w, groups, extra_var, scale2)
        a_t = _row_matrix(thresh, "thresh", "L", lead, m, dev)
        L = int(a_t.shape[-2])
        need = int(lib.dgp_excess_moments_workspace_bytes(m, P, L, B))
        if need == 0:
            raise ValueError(f"bad size: m = {m}, ngroups = {P}, levels = {L}, batch = {B} "
                             "(1 <= m <= 2^20, 1 <= ngroups <= 65535, 1 <= levels <= 64, 1 <= batch <= 1024)")
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        mean_out = torch.empty(lead + (L, P), dtype=torch.float64, device=dev)
        cov_out = torch.empty(lead + (L, P, P), dtype=torch.float64, device=dev)
        total_out = torch.empty(lead + (P,), dtype=torch.float64, device=dev)
        _call("dgp_excess_moments", _DTYPES[cov.dtype], _ptr(cov), m, B, _ptr(mu_t), _ptr(s2), _ptr(a_t), _ptr(w_t), _ptr(g_t), P, L,
              _ptr(ev_t), int(bool(above)), _ptr(work), need, _ptr(mean_out), _ptr(cov_out), _ptr(total_out))
    return mean_out, cov_out, total_out


def _window_bounds(lo, hi, lead, m):
    """``lo`` / ``hi`` of ``window_moments`` checked on the host: int32, shape ``lead + (q,)``, 0 <= lo <= hi <= m, both
    non-decreasing along the windows.  -> (lo, hi) as contiguous host int32 tensors and q.  ``ValueError`` otherwise."""
    out = []
    for name, t in (("lo", lo), ("hi", hi)):
        t = torch.as_tensor(t)
        if t.dtype != torch.int32:
            raise ValueError(f"{name} must be int32, not {t.dtype}")
        if t.dim() != len(lead) + 1 or tuple(t.shape[:-1]) != lead or t.shape[-1] < 1:
            raise ValueError(f"{name} must have shape {lead + ('q',)}, not {tuple(t.shape)}")
        out.append(t.detach().cpu().contiguous())
    lo_h, hi_h = out
    if lo_h.shape != hi_h.shape:
        raise ValueError(f"lo and hi must have the same shape {lead + ('q',)}")
    if bool((lo_h < 0).any()) or bool((hi_h < lo_h).any()) or bool((hi_h > int(m)).any()):
        raise ValueError(f"window bounds out of range: they must satisfy 0 <= lo <= hi <= m = {int(m)}")
    if bool((lo_h[..., 1:] < lo_h[..., :-1]).any()) or bool((hi_h[..., 1:] < hi_h[..., :-1]).any()):
        raise ValueError("lo and hi must both be non-decreasing along the windows")
    return lo_h, hi_h, int(lo_h.shape[-1])


def window_moments(cov: torch.Tensor, m: int, mu: torch.Tensor, lo, hi, a=None, mode: int = MODE_LINEAR, scale2=None):
    """Exact mean and covariance of the rolling-window means sum_j W_ij f'_j of a latent posterior f ~ N(mu, C) --
    W_ij = a_j / sum_{k in window i} a_k over the window ``lo[i] <= j < hi[i]`` -- through one ``dgp_window_moments`` call (no
    factorisation, no draws).  MODE_LINEAR: f' = f, the statistic is exactly Gaussian, N(W mu, W C W^T) (``scale2`` unused);
    MODE_LOG: the arithmetic window mean of exp(f'), f' = s f + t, with ``mu`` the MAPPED mean s mu + t and ``scale2`` = s^2.

    ``cov``: what ``GPPlan.posterior_cov`` returns -- (M, M), M = padded m, lower triangle and diagonal blocks valid -- or
    (B, M, M) for B sites; ``mu``: (m,) / (B, m), the dtype of ``cov``; ``lo`` / ``hi``: int32 (q,) / (B, q), both
    non-decreasing with 0 <= lo <= hi <= m (checked here; ``ValueError``); ``a``: None (= 1) or non-negative weights (m,) /
    (B, m).  An empty window or a zero weight sum gives mean 0 and a zero row and column.
    -> (mean (q,), cov (Q, Q)) or ((B, q), (B, Q, Q)), float64 device tensors; ``cov`` has the layout of ``posterior_cov``
    (Q = padded q, lower triangle and diagonal 128-blocks valid, identity pad; blocks above the block diagonal hold zeros) and
    goes into ``exceedance_moments`` / ``period_moments`` / ``sample_value`` as a float64 covariance."""
    m = int(m)
    lo_h, hi_h, q = _window_bounds(lo, hi, tuple(cov.shape[:-2]), m)  # the windows are checked before the covariance
    if mode not in (MODE_LINEAR, MODE_LOG):
        raise ValueError(f"mode must be MODE_LINEAR or MODE_LOG, not {mode!r}")
    if mode == MODE_LOG and scale2 is None:
        raise ValueError("MODE_LOG needs scale2 = s^2")
    lib, lead, B, dev = _cov_layout(cov, m)
    with torch.cuda.device(dev):
        mu_t, a_t, _g, _ev, s2 = _moment_inputs(dev, cov.dtype, lead, m, mu, a, None, None, scale2 if mode == MODE_LOG else None)
        need = int(lib.dgp_window_moments_workspace_bytes(m, q, B))
        if need == 0:
            raise ValueError(f"bad size: m = {m}, q = {q}, batch = {B} (1 <= m, q <= 2^20, 1 <= batch <= 1024)")
        Q = int(lib.dgp_padded_n(q))
        lo_t, hi_t = lo_h.to(dev), hi_h.to(dev)
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        mean_out = torch.empty(lead + (q,), dtype=torch.float64, device=dev)
        cov_out = torch.zeros(lead + (Q, Q), dtype=torch.float64, device=dev)
        _call("dgp_window_moments", _DTYPES[cov.dtype], int(mode), _ptr(cov), m, B, _ptr(mu_t), _ptr(s2), _ptr(a_t), _ptr(lo_t),
              _ptr(hi_t), q, _ptr(work), need, _ptr(mean_out), _ptr(cov_out))
    return mean_out, cov_out


def _window_mode(mode, scale2):
    if mode not in (MODE_LINEAR, MODE_LOG):
        raise ValueError(f"mode must be MODE_LINEAR or MODE_LOG, not {mode!r}")
    if mode == MODE_LOG and scale2 is None:
        raise ValueError("MODE_LOG needs scale2 = s^2")


def window_variances(cov: torch.Tensor, m: int, mu: torch.Tensor, lo, hi, a=None, mode: int = MODE_LINEAR, scale2=None):
    """The means of ``window_moments`` and the DIAGONAL of its covariance -- the variance of every rolling-window mean --
    through one ``dgp_window_variances`` call: the same arguments and rules, a work area of 3 M + 3 Q doubles per site instead
    of M Q, and no (Q, Q) result.  Entries of ``cov`` on and below the diagonal are read, the diagonal included.
    -> (mean (q,), var (q,)) or ((B, q), (B, q)), float64 device tensors."""
    m = int(m)
    lo_h, hi_h, q = _window_bounds(lo, hi, tuple(cov.shape[:-2]), m)  # the windows are checked before the covariance
    _window_mode(mode, scale2)
    lib, lead, B, dev = _cov_layout(cov, m)
    with torch.cuda.device(dev):
        mu_t, a_t, _g, _ev, s2 = _moment_inputs(dev, cov.dtype, lead, m, mu, a, None, None, scale2 if mode == MODE_LOG else None)
        need = int(lib.dgp_window_variances_workspace_bytes(m, q, B))
        if need == 0:
            raise ValueError(f"bad size: m = {m}, q = {q}, batch = {B} (1 <= m, q <= 2^20, 1 <= batch <= 1024)")
        lo_t, hi_t = lo_h.to(dev), hi_h.to(dev)
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        mean_out = torch.empty(lead + (q,), dtype=torch.float64, device=dev)
        var_out = torch.empty(lead + (q,), dtype=torch.float64, device=dev)
        _call("dgp_window_variances", _DTYPES[cov.dtype], int(mode), _ptr(cov), m, B, _ptr(mu_t), _ptr(s2), _ptr(a_t), _ptr(lo_t),
              _ptr(hi_t), q, _ptr(work), need, _ptr(mean_out), _ptr(var_out))
    return mean_out, var_out


MAX_SERIES_TERMS = 64  # the largest ``nterms`` of ``dgp_sample_value``


def series_terms(beta: float) -> int:
    """Terms of the exponential series ``sample_value`` needs: the smallest K <= 64 with sum_{k>K} beta^k / k! <= 2^-53 beta,
    beta = s^2 max_i C_ii -- the truncation then stays below the rounding of the first term.  Raises ``ValueError`` naming
    beta when 64 terms do not suffice (beta above about 14.7, however large) or beta is not a finite number >= 0."""
    beta = float(beta)
    if not (beta >= 0.0) or beta == float("inf"):
        raise ValueError(f"sample_value: beta = s^2 max C_ii = {beta} is not a finite number >= 0")
    if beta == 0.0:
        return 1
    too_many = ValueError(f"sample_value: beta = s^2 max C_ii = {beta:.6g} needs more than {MAX_SERIES_TERMS} terms of the "
                          "exponential series")
    if beta > MAX_SERIES_TERMS:  # the terms beta^k / k! still grow at k = 64: decided without running the series
        raise too_many
    terms, t = [], 1.0
    for k in range(1, 5 * MAX_SERIES_TERMS + 1):  # beta <= 64: beta^k / k! < 1e-49 beta from k = 320 on
        t *= beta / k
        terms.append(t)
    tail = 0.0
    tails = [0.0] * (len(terms) + 1)  # tails[K] = sum_{k>K} beta^k / k!
    for k in range(len(terms), 0, -1):
        tails[k - 1] = tail = tail + terms[k - 1]
    for K in range(1, MAX_SERIES_TERMS + 1):
        if tails[K] <= 2.0 ** -53 * beta:
            return K
    raise too_many


def sample_value(cov: torch.Tensor, m: int, a: torch.Tensor, scale2, groups: torch.Tensor, ngroups: int,
                 obs_var: torch.Tensor | None = None, rows: torch.Tensor | None = None, nterms: int | None = None):
    """Expected reduction gain[p, c] = Var(E[L_p | y_c]) of the variance of every period sum L_p = sum_{i in p} w_i c_i
    (``period_moments``' setting) by ONE more sample y_c = f_c + eps on day c, for every day c at once, through one
    ``dgp_sample_value`` call: sum_k (s^2)^k / k! (sum_{i in p} A_i b_ic^k)^2 with b_ic = C'_ic / sqrt(v'_c),
    v'_c = C'_cc + obs_var_c and C' = C - rows^T rows the covariance after the samples already decided.

    ``cov``: what ``GPPlan.posterior_cov`` returns, (M, M) or (B, M, M), never modified; ``a``: A_i = w_i exp(s mu_i + t +
    s^2 C_ii / 2) for a log target, w_i for a linear one, (m,) / (B, m); ``scale2``: s^2, a number or (B,) values;
    ``groups``: int32 ids (m,) / (B, m) in 0 .. ngroups-1, non-decreasing except for -1 (excluded) anywhere -- excluded
    days are candidates too; ``obs_var``: None or (m,) / (B, m), the noise variance of the hypothetical sample;
    ``rows``: None or (nrows, m) / (B, nrows, m) float64 with nrows <= 64, the conditioning rows B of the pivoted-Cholesky
    recurrence; ``nterms``: the series length K (1 = a linear target, exactly); None picks ``series_terms`` of
    beta = s^2 max C_ii over the included days, read from the buffer's diagonal.
    -> (gain (P, m), var (m,)) or ((B, P, m), (B, m)), float64 device tensors; var is v'_c (0 where it is not > 0: such a
    candidate has gain 0)."""
    lib, lead, B, dev = _cov_layout(cov, m)
    m = int(m)
    with torch.cuda.device(dev):
        _, a_t, g_t, ov_t, s2 = _moment_inputs(dev, cov.dtype, lead, m, None, a, groups, obs_var, scale2)
        rows_t = None if rows is None else _row_matrix(rows, "rows", "nrows", lead, m, dev)
        nrows = 0 if rows_t is None else int(rows_t.shape[-2])
        if nrows == 0:
            rows_t = None
        if nterms is None:
            diag = torch.diagonal(cov, dim1=-2, dim2=-1)[..., :m].double()
            top = torch.where(g_t >= 0, diag, torch.zeros_like(diag)).reshape(B, -1).amax(dim=1)
            nterms = series_terms(float((s2 * top).max()))
        P, K = int(ngroups), int(nterms)
        need = int(lib.dgp_sample_value_workspace_bytes(m, P, nrows, K, B))
        if need == 0:
            raise ValueError(f"bad size: m = {m}, ngroups = {P}, nrows = {nrows}, nterms = {K}, batch = {B} (1 <= m <= 2^20, "
                             "1 <= ngroups <= 65535, 0 <= nrows <= 64, 1 <= nterms <= 64, 1 <= batch <= 1024)")
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        gain = torch.empty(lead + (P, m), dtype=torch.float64, device=dev)
        var = torch.empty(lead + (m,), dtype=torch.float64, device=dev)
        _call("dgp_sample_value", _DTYPES[cov.dtype], _ptr(cov), m, B, _ptr(a_t), _ptr(s2), _ptr(g_t), P, _ptr(ov_t), _ptr(rows_t),
              nrows, K, _ptr(work), need, _ptr(gain), _ptr(var))
    return gain, var


def bvn_excess(h: torch.Tensor, k: torch.Tensor, rho: torch.Tensor):
    """Phi2(h, k; rho) - Phi(h) Phi(k) pointwise on the device (``dgp_debug_bvn_excess``): the pair function of
    ``exceedance_moments``, for tests.  Float64 CUDA tensors of one shape."""
    if not (h.is_cuda and h.dtype == k.dtype == rho.dtype == torch.float64 and h.shape == k.shape == rho.shape):
        raise ValueError("h, k, rho must be float64 CUDA tensors of one shape")
    h, k, rho = h.contiguous(), k.contiguous(), rho.contiguous()
    out = torch.empty_like(h)
    with torch.cuda.device(h.device):
        _call("dgp_debug_bvn_excess", _ptr(h), _ptr(k), _ptr(rho), h.numel(), _ptr(out))
    return out


ORTHANT_MAX_DIM = 16384     # the largest m of ``dgp_orthant_probability``
ORTHANT_MAX_LEVELS = 64     # levels of one call; longer lists go in several
ORTHANT_DEFAULT_MAX_BYTES = 8 * 2 ** 30  # the work area ``orthant_probability`` allows itself when ``max_bytes`` is None
_orthant_ws = {}            # device -> the cached work area (grown, never shrunk)


def richtmyer_generators(m: int):
    """The generators g_i = frac(sqrt(p_i)), p_i the i-th prime, i = 0 .. m-1, of the Richtmyer rule ``orthant_probability``
    runs over (a numpy sieve; plumbing).  -> float64 numpy array (m,)."""
    import numpy as np

    m = int(m)
    if m < 1:
        raise ValueError("m must be at least 1")
    bound = 16
    while True:
        sieve = np.ones(bound + 1, dtype=bool)
        sieve[:2] = False
        for k in range(2, int(bound ** 0.5) + 1):
            if sieve[k]:
                sieve[k * k::k] = False
        primes = np.nonzero(sieve)[0]
        if primes.size >= m:
            break
        bound *= 2
    root = np.sqrt(primes[:m].astype(np.float64))
    return root - np.floor(root)


def orthant_shifts(m: int, nshifts: int, seed: int = 0):
    """The random shifts of ``orthant_probability``: (nshifts, m) float64 in [0, 1) from torch's CPU generator seeded with
    ``seed``.  One set serves every level of a call, so a level's shifts cannot depend on how the levels are chunked."""
    return torch.rand(int(nshifts), int(m), dtype=torch.float64, generator=torch.Generator().manual_seed(int(seed)))


def orthant_level_chunks(m: int, nlevels: int, nshifts: int, npoints: int, max_bytes=None):
    """How ``orthant_probability`` splits ``nlevels`` levels into calls: the most levels (at most 64) whose work area fits
    ``max_bytes`` (None: ``ORTHANT_DEFAULT_MAX_BYTES``).  -> (levels per call, bytes of one level's work area).  ``ValueError``
    naming the bytes when one level does not fit, or the sizes when they are out of range.  Needs no device."""
    lib = _lib.load()
    m, nlevels, nshifts, npoints = int(m), int(nlevels), int(nshifts), int(npoints)
    one = int(lib.dgp_orthant_probability_workspace_bytes(m, 1, nshifts, npoints))
    if one == 0 or nlevels < 1:
        raise ValueError(f"bad size: m = {m}, levels = {nlevels}, nshifts = {nshifts}, npoints = {npoints} "
                         f"(1 <= m <= {ORTHANT_MAX_DIM}, 1 <= levels, 2 <= nshifts <= 64, 1 <= npoints <= 2^20)")
    budget = ORTHANT_DEFAULT_MAX_BYTES if max_bytes is None else int(max_bytes)
    if one > budget:
        raise ValueError(f"orthant_probability needs a work area of {one} bytes for ONE level (m = {m}, {nshifts} shifts x "
                         f"{npoints} points), which exceeds max_bytes = {budget}")
    return min(nlevels, ORTHANT_MAX_LEVELS, budget // one), one


def orthant_probability(L: torch.Tensor, m: int, lo, hi, npoints: int = 4096, nshifts: int = 16, seed: int = 0, max_bytes=None,
                        hook=None):
    """Orthant probabilities P(lo_l <= f <= hi_l), f ~ N(0, L L^T) in ``m`` dimensions, one per level l, through
    ``dgp_orthant_probability``: Genz's separation of variables over ``nshifts`` randomly shifted Richtmyer rules of
    ``npoints`` points.  NOT exact: unbiased, with its own standard error.

    ``L``: the lower factor as ``GPPlan.psd_safe_factor`` leaves it -- (M, M) float64 CUDA, M = padded m; blocks above the
    block diagonal are never read; ``lo`` / ``hi``: the CENTRED limits, (m,) or (levels, m), +-inf allowed.  The generators
    (``richtmyer_generators``) and the shifts (``orthant_shifts``: torch's CPU generator with ``seed``) come from the host.
    The work area is cached per device; when it would exceed ``max_bytes`` the levels go in several calls
    (``orthant_level_chunks``) -- every level sees the same shifts either way.  ``hook``: called with a dict of the call's
    device inputs (``L``, ``m``, ``lo``, ``hi``, ``gen``, ``shifts``, ``npoints``) before the launches, for tests.
    -> (prob (levels,), se (levels,)) float64 device tensors."""
    m = int(m)
    if not (torch.is_tensor(L) and L.is_cuda and L.dtype == torch.float64 and L.dim() == 2 and L.stride(1) == 1):
        raise ValueError("L must be a 2-D float64 CUDA tensor with contiguous rows")
    dev = L.device
    lo_t = torch.as_tensor(lo, dtype=torch.float64).reshape(-1, m).to(dev).contiguous()
    hi_t = torch.as_tensor(hi, dtype=torch.float64).reshape(-1, m).to(dev).contiguous()
    if lo_t.shape != hi_t.shape:
        raise ValueError("lo and hi must have the same shape, (m,) or (levels, m)")
    nlev = int(lo_t.shape[0])
    per_call, one = orthant_level_chunks(m, nlev, nshifts, npoints, max_bytes)
    M = int(_lib.load().dgp_padded_n(m))
    if L.shape[0] < M or L.shape[1] < M:
        raise ValueError(f"L must hold the padded ({M}, {M}) factor")
    with torch.cuda.device(dev):
        gen = torch.from_numpy(richtmyer_generators(m)).to(dev)
        shifts = orthant_shifts(m, nshifts, seed).to(dev)
        if hook is not None:
            hook(dict(L=L, m=m, lo=lo_t, hi=hi_t, gen=gen, shifts=shifts, npoints=int(npoints)))
        need = one * per_call
        ws = _orthant_ws.get(dev)
        if ws is None or ws.numel() < need + 256:
            _orthant_ws[dev] = None
            _orthant_ws[dev] = ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
        off = (-ws.data_ptr()) % 256
        prob = torch.empty(nlev, dtype=torch.float64, device=dev)
        se = torch.empty(nlev, dtype=torch.float64, device=dev)
        for l0 in range(0, nlev, per_call):
            n = min(per_call, nlev - l0)
            _call("dgp_orthant_probability", _ptr(L), m, int(L.stride(0)), _ptr(lo_t[l0:l0 + n]), _ptr(hi_t[l0:l0 + n]), n, _ptr(gen),
                  _ptr(shifts), int(nshifts), int(npoints), C.c_void_p(ws.data_ptr() + off), one * n, _ptr(prob[l0:l0 + n]),
                  _ptr(se[l0:l0 + n]))
    return prob, se


PATH_COUNT_LEVEL_GROUP = 16  # levels that share one workgroup's draws in ``dgp_path_counts``: 1 .. 16 levels cost one work area
_counts_ws = {}              # device -> the cached work area of ``path_counts`` (grown, never shrunk)


def path_count_level_chunks(m: int, nlevels: int, nshifts: int, npoints: int, max_bytes=None):
    """How ``path_counts`` splits ``nlevels`` levels into calls: the most levels (at most 64) whose work area fits
    ``max_bytes`` (None: ``ORTHANT_DEFAULT_MAX_BYTES``).  The draws of a workgroup serve up to 16 levels, so the work area
    grows by one level's bytes per 16 levels.  -> (levels per call, bytes of one level's work area).  ``ValueError`` naming the
    bytes when one level does not fit, or the sizes when they are out of range.  Needs no device."""
    lib = _lib.load()
    m, nlevels, nshifts, npoints = int(m), int(nlevels), int(nshifts), int(npoints)
    one = int(lib.dgp_path_counts_workspace_bytes(m, 1, nshifts, npoints))
    if one == 0 or nlevels < 1:
        raise ValueError(f"bad size: m = {m}, levels = {nlevels}, nshifts = {nshifts}, npoints = {npoints} "
                         f"(1 <= m <= {ORTHANT_MAX_DIM}, 1 <= levels, 2 <= nshifts <= 64, 1 <= npoints <= 2^20)")
    budget = ORTHANT_DEFAULT_MAX_BYTES if max_bytes is None else int(max_bytes)
    if one > budget:
        raise ValueError(f"path_counts needs a work area of {one} bytes for ONE level (m = {m}, {nshifts} shifts x "
                         f"{npoints} points), which exceeds max_bytes = {budget}")
    return min(nlevels, ORTHANT_MAX_LEVELS, (budget // one) * PATH_COUNT_LEVEL_GROUP), one


def path_counts(L: torch.Tensor, m: int, thr, above: bool = True, link=None, npoints: int = 4096, nshifts: int = 16, seed: int = 0,
                max_bytes=None, hook=None):
    """Histograms of the exceedance count N and of the longest spell R of joint paths f ~ N(0, L L^T) in ``m`` dimensions
    through ``dgp_path_counts``: per level l and shift s, over the ``npoints`` points of the s-th randomly shifted Richtmyer
    rule, how many paths have N = k points beyond ``thr[l]`` (``above``: f_i > thr, else f_i < thr; a NaN threshold never
    counts) and how many have a longest run of R = k consecutive such points.  NOT exact: unbiased; the caller forms the pmf
    (hist / npoints), its functionals per shift and their standard errors over the shifts.

    ``L``: the lower factor as ``GPPlan.psd_safe_factor`` leaves it (see ``orthant_probability``); ``thr``: the CENTRED
    thresholds, (m,) or (levels, m); ``link``: (m,) flags, ``link[i] == 0`` breaks a run between points i - 1 and i (None: no
    breaks).  Generators, shifts, ``seed`` and ``hook`` (keys ``L``, ``m``, ``thr``, ``above``, ``link``, ``gen``, ``shifts``,
    ``npoints``) as for ``orthant_probability``.  The work area is cached per device; lists of more than 64 levels, or over
    ``max_bytes``, go in several calls on the same shifts (``path_count_level_chunks``): a level's integers do not change.
    -> (count_hist, spell_hist) int32 device tensors (levels, nshifts, m + 1)."""
    m = int(m)
    if not (torch.is_tensor(L) and L.is_cuda and L.dtype == torch.float64 and L.dim() == 2 and L.stride(1) == 1):
        raise ValueError("L must be a 2-D float64 CUDA tensor with contiguous rows")
    dev = L.device
    thr_t = torch.as_tensor(thr, dtype=torch.float64).reshape(-1, m).to(dev).contiguous()
    nlev = int(thr_t.shape[0])
    link_t = None
    if link is not None:
        link_t = (torch.as_tensor(link).reshape(-1) != 0).to(torch.int32).to(dev).contiguous()
        if link_t.numel() != m:
            raise ValueError(f"link must hold m = {m} flags")
    per_call, one = path_count_level_chunks(m, nlev, nshifts, npoints, max_bytes)
    M = int(_lib.load().dgp_padded_n(m))
    if L.shape[0] < M or L.shape[1] < M:
        raise ValueError(f"L must hold the padded ({M}, {M}) factor")
    with torch.cuda.device(dev):
        gen = torch.from_numpy(richtmyer_generators(m)).to(dev)
        shifts = orthant_shifts(m, nshifts, seed).to(dev)
        if hook is not None:
            hook(dict(L=L, m=m, thr=thr_t, above=bool(above), link=link_t, gen=gen, shifts=shifts, npoints=int(npoints)))
        need = one * (-(-per_call // PATH_COUNT_LEVEL_GROUP))
        ws = _counts_ws.get(dev)
        if ws is None or ws.numel() < need + 256:
            _counts_ws[dev] = None
            _counts_ws[dev] = ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
        off = (-ws.data_ptr()) % 256
        count = torch.empty(nlev, int(nshifts), m + 1, dtype=torch.int32, device=dev)
        spell = torch.empty(nlev, int(nshifts), m + 1, dtype=torch.int32, device=dev)
        for l0 in range(0, nlev, per_call):
            n = min(per_call, nlev - l0)
            _call("dgp_path_counts", _ptr(L), m, int(L.stride(0)), _ptr(thr_t[l0:l0 + n]), n, 1 if above else 0,
                  _ptr(link_t) if link_t is not None else None, _ptr(gen), _ptr(shifts), int(nshifts), int(npoints),
                  C.c_void_p(ws.data_ptr() + off), need, _ptr(count[l0:l0 + n]), _ptr(spell[l0:l0 + n]))
    return count, spell


def cross_validate_folds(plan, groups, launch, max_group_bound=None):
    """Host half of ``GPPlan.cross_validate``: validate the fold ids, sort every site's observations by fold (held-out
    ones first, stable) and hand ``launch(order, start, ngroups, max_group)`` the int32 CPU tensors ``order`` (batch, n)
    / ``start`` (batch, ngroups + 1) -- (n,) / (ngroups + 1,) for an unbatched plan."""
    g = torch.as_tensor(groups)
    if g.dtype.is_floating_point or g.dtype == torch.bool:
        raise ValueError("fold ids must be integers")
    g = g.detach().to("cpu", torch.int64)
    batch, n = plan.batch, plan.n
    if tuple(g.shape) != ((n,) if batch == 1 else (batch, n)):
        raise ValueError(f"groups must have shape {(n,) if batch == 1 else (batch, n)}, got {tuple(g.shape)}")
    g = g.reshape(batch, n).clone()
    for b in range(batch):
        g[b, int(plan._site_sizes[b]):] = -1
    if int(g.min()) < -1:
        raise ValueError("fold ids must be >= 0, or -1 for observations that are never held out")
    if int(g.max()) < 0:
        raise ValueError("no observation is held out")
    ngroups = int(g.max()) + 1
    if ngroups > n:
        raise ValueError(f"fold ids must be below n = {n}")
    order = torch.empty(batch, n, dtype=torch.int32)
    start = torch.empty(batch, ngroups + 1, dtype=torch.int32)
    max_group = 1
    for b in range(batch):
        key = torch.where(g[b] >= 0, g[b], torch.full_like(g[b], ngroups))
        order[b] = torch.argsort(key, stable=True).to(torch.int32)
        counts = torch.bincount(g[b][g[b] >= 0], minlength=ngroups)
        start[b, 0] = 0
        start[b, 1:] = torch.cumsum(counts, 0).to(torch.int32)
        max_group = max(max_group, int(counts.max()))
    if max_group_bound is not None:
        if not max_group <= int(max_group_bound) <= n:
            raise ValueError(f"max_group = {max_group_bound} must be between the largest fold ({max_group}) and n = {n}")
        max_group = int(max_group_bound)
    if batch == 1:
        order, start = order[0], start[0]
    return launch(order, start, ngroups, max_group)
