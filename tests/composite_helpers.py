"""Seeded random kernel trees for the GENERIC composite evaluator (``dgp_composite_define`` / ``csrc/dgp_models.h::Composite``),
their data and their dense references (TEST INFRASTRUCTURE; everything here runs on the CPU).

``CASES`` is a fixed list from one seed: 20 random trees (``random_spec`` / ``theta_for``, d drawn from 1 to 6) and the eight
hand-built trees of ``_hand_built``.  Every one of the five factor kinds (RBF, Matern 1/2, 3/2, 5/2, Periodic) stands alone
at d = 1 in one tree: four of them are hand-built, and the scaled Matern 3/2 alone at d = 1 is what the seed drew as
"random 12", so building it by hand as well would only register the same structure twice (tests/test_composite_cpu.py asserts
that it is there).  That makes 28 distinct structures, the most the sweep was planned with.

Registry budget.  The composite registry holds 64 structures per process and the suite runs in one process.  Counted when
this file was written, the other tests register 11 distinct structures (tests/test_terms_cpu.py 1, tests/test_slopes_cpu.py
2, tests/test_engine_cpu.py 2, tests/test_gpu_composite.py 4 -- its engine-level trend models repeat one of them, and
tests/test_gpu_fisher.py reuses its tree --, tests/test_gpu_terms.py 2; tests/test_gpu_slopes.py repeats three of those and
adds none; the fused models of tests/test_gpu_engine.py, tests/test_gpu_sample.py and the rest take no slot), one of which
(the scaled RBF at d = 1) is also in ``CASES``.  ``CASES`` adds 27 more, and nothing else in the new tests registers a
structure of its own: the lowering test builds its ``gp.kernels`` trees FROM descriptions of ``CASES`` (``tree_from_spec``),
the malformed descriptions are refused, and the registry-full test fills the registry of a child process.  Total: 38 of 64.
That count is not what the tests rely on: ids are handed out in order from ``COMPOSITE_BASE``, so ``define`` asserts on every
call that the slot it was given lies below ``REGISTRY_BUDGET`` = 56, whatever the rest of the suite registered before it.

References.  All of them come from ``orc.composite_gram`` on the same description and autograd -- fit step
``orc.nll_data_and_grads``, prediction ``orc.posterior``, slopes ``slopes_reference`` with ``composite_prior``, Fisher
``fisher_helpers.dense_fisher`` (the sweep calls it directly) -- and none from device code.  The additive parts are ``composite_gram`` of the ONE-TERM sub-description
with that term's slice of theta (``part_grams``), which covers unscaled terms as well.  ``tree_gram`` evaluates a
``gp.kernels`` module tree directly with ``orc.rbf`` / ``orc.matern`` / ``orc.periodic`` and does not go through
``composite_spec``: an independent check of the lowering's parameter order."""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass

import numpy as np
import torch

from oracle import gp_oracle as orc
from tests.slopes_helpers import composite_prior, slopes_reference
from tests.terms_helpers import terms_reference

RBF, MATERN, PERIODIC = 0, 1, 2
MAX_THETA = 24  # DGP_MAX_THETA
COMPOSITE_BASE = 16  # DGP_MODEL_COMPOSITE_BASE: the id of the process's first structure (the registry-full test checks it)
REGISTRY_BUDGET = 56  # of the 64 slots of a process, the most the whole suite may have taken once CASES are registered
SEED = 20240  # the one seed of CASES
NOISE = 0.05


# ---- descriptions ----------------------------------------------------------------------------------------------------
def build_spec(d, terms):
    """``terms``: [(scaled, [(kind, 2 nu, ard, columns), ...]), ...] -> the int list ``dgp_composite_define`` takes."""
    spec = [int(d), len(terms)]
    for scaled, factors in terms:
        spec += [int(bool(scaled)), len(factors)]
        for kind, nu2, ard, cols in factors:
            spec += [int(kind), int(nu2), int(bool(ard)), len(cols), *[int(c) for c in cols]]
    return spec


def parse_spec(spec):
    """-> (d, [(scaled, [(kind, 2 nu, ard, columns), ...]), ...]), the inverse of ``build_spec``."""
    spec = [int(v) for v in spec]
    terms, i = [], 2
    for _t in range(spec[1]):
        scaled, nfac = spec[i], spec[i + 1]
        i += 2
        factors = []
        for _f in range(nfac):
            kind, nu2, ard, nd = spec[i:i + 4]
            factors.append((kind, nu2, ard, tuple(spec[i + 4:i + 4 + nd])))
            i += 4 + nd
        terms.append((scaled, factors))
    assert i == len(spec)
    return spec[0], terms


def _factor_ntheta(factor):
    kind, _nu2, ard, cols = factor
    return (len(cols) if ard else 1) + (1 if kind == PERIODIC else 0)


def term_slices(spec):
    """[(first, last + 1) of every term's parameters in theta]: [outputscale], per factor [lengthscale(s)], [period]."""
    out, t = [], 0
    for scaled, factors in parse_spec(spec)[1]:
        k = int(scaled) + sum(_factor_ntheta(f) for f in factors)
        out.append((t, t + k))
        t += k
    return out


def ntheta(spec):
    return term_slices(spec)[-1][1]


def random_spec(rng, d):
    """One draw: 1 to 6 terms, each scaled with probability 0.75 and with 1 to 3 factors; factor kind from RBF / Matern /
    Matern / Periodic, nu from {1/2, 3/2, 5/2}; Periodic factors on one column, the others on a random sorted subset of 1 to
    d columns, ARD with probability 1/2 when the subset has more than one column.  May have more than 24 parameters."""
    terms = []
    for _t in range(int(rng.integers(1, 7))):
        scaled = bool(rng.random() < 0.75)
        factors = []
        for _f in range(int(rng.integers(1, 4))):
            kind = (RBF, MATERN, MATERN, PERIODIC)[int(rng.integers(0, 4))]
            nu2 = (1, 3, 5)[int(rng.integers(0, 3))] if kind == MATERN else 0
            if kind == PERIODIC:
                cols, ard = (int(rng.integers(0, d)),), False
            else:
                k = int(rng.integers(1, d + 1))
                cols = tuple(sorted(int(c) for c in rng.choice(d, size=k, replace=False)))
                ard = bool(k > 1 and rng.random() < 0.5)
            factors.append((kind, nu2, ard, cols))
        terms.append((scaled, factors))
    return build_spec(d, terms)


def theta_for(rng, spec):
    """Outputscales uniform in (0.3, 2.0), lengthscales in (0.5, 3.0), periods in (0.7, 2.5), in the description's order."""
    vals = []
    for scaled, factors in parse_spec(spec)[1]:
        if scaled:
            vals.append(rng.uniform(0.3, 2.0))
        for kind, _nu2, ard, cols in factors:
            vals += [rng.uniform(0.5, 3.0) for _ in range(len(cols) if ard else 1)]
            if kind == PERIODIC:
                vals.append(rng.uniform(0.7, 2.5))
    return torch.tensor(vals, dtype=torch.float64)


def _hand_built():
    m = lambda nu2, cols, ard=False: (MATERN, nu2, ard, cols)  # noqa: E731
    rbf = lambda cols, ard=False: (RBF, 0, ard, cols)  # noqa: E731
    per = lambda col: (PERIODIC, 0, False, (col,))  # noqa: E731
    return [
        # 6 terms x 3 factors, 3 outputscales + 18 first lengthscales + 1 ARD extra + 2 periods = 24 parameters; d = 4
        ("6x3 with 24 parameters", build_spec(4, [
            (True, [per(0), m(5, (0,)), rbf((1, 2), True)]),
            (True, [m(3, (0, 1, 2, 3)), rbf((3,)), m(1, (2,))]),
            (False, [per(1), m(5, (1,)), rbf((0,))]),
            (True, [m(3, (1,)), m(5, (2, 3)), rbf((0, 3))]),
            (False, [rbf((2,)), m(3, (3,)), m(5, (0,))]),
            (False, [m(5, (1,)), rbf((3,)), m(3, (0,))])])),
        ("one unscaled factor d=6", build_spec(6, [(False, [rbf((0, 1, 2, 3, 4, 5))])])),
        ("rbf alone d=1", build_spec(1, [(True, [rbf((0,))])])),
        ("matern12 alone d=1", build_spec(1, [(True, [m(1, (0,))])])),
        ("periodic alone d=1", build_spec(1, [(True, [per(0)])])),
        ("every term unscaled d=3", build_spec(3, [(False, [rbf((0, 1, 2), True)]), (False, [m(5, (0,)), per(0)]),
                                                   (False, [m(3, (1, 2))])])),
        # column 0 carries a Periodic, a Matern-1/2 and an ARD RBF factor in three different terms
        ("one column three kinds d=2", build_spec(2, [(True, [per(0), m(5, (1,))]), (True, [m(1, (0,))]),
                                                      (True, [rbf((0, 1), True)])])),
        # (Matern 3/2 alone at d = 1 is "random 12"; appended, so that the trees above keep their index and data)
        ("matern52 alone d=1", build_spec(1, [(True, [m(5, (0,))])])),
    ]


@dataclass(frozen=True)
class Case:
    name: str
    spec: tuple
    theta: torch.Tensor
    hand_built: bool

    @property
    def d(self):
        return self.spec[0]

    @property
    def terms(self):
        return parse_spec(self.spec)[1]

    @property
    def ntheta(self):
        return ntheta(self.spec)


N_RANDOM = 20


def _build_cases():
    rng = np.random.default_rng(SEED)
    cases, dropped = [], 0
    while len(cases) < N_RANDOM:
        d = int(rng.integers(1, 7))
        spec = random_spec(rng, d)
        if ntheta(spec) > MAX_THETA:
            dropped += 1
            continue
        cases.append(Case(f"random {len(cases)} d={d}", tuple(spec), theta_for(rng, spec), False))
    for name, spec in _hand_built():
        cases.append(Case(name, tuple(spec), theta_for(rng, spec), True))
    return cases, dropped


CASES, DROPPED = _build_cases()
HAND_BUILT = [i for i, c in enumerate(CASES) if c.hand_built]
RANDOM = [i for i, c in enumerate(CASES) if not c.hand_built]
BIGGEST = next(i for i in HAND_BUILT if CASES[i].ntheta == MAX_THETA)  # the 6 x 3 tree with 24 parameters


def by_name(name):
    """The index in ``CASES`` of the tree of that name."""
    return next(i for i, c in enumerate(CASES) if c.name == name)


# ---- the library's host side -------------------------------------------------------------------------------------------
def define_raw(spec):
    """``dgp_composite_define`` as it is: -> (return code, model id)."""
    from discontinuum_amd import _lib

    arr, mid = (C.c_int * max(len(spec), 1))(*[int(v) for v in spec]), C.c_int(-1)
    return int(_lib.load().dgp_composite_define(arr, len(spec), C.byref(mid))), int(mid.value)


def define(spec):
    """Register the description (an identical one is reused) and its oracle Gram: -> the model name for ``GPPlan``."""
    rc, mid = define_raw(spec)
    assert rc == 0, ("dgp_composite_define", rc, list(spec))
    assert 0 <= mid - COMPOSITE_BASE < REGISTRY_BUDGET, ("composite registry slots in use", mid - COMPOSITE_BASE + 1)
    name = f"composite:{mid}"
    orc.GRAMS[name] = orc.composite_gram(list(spec))
    return name


def differentiable_columns(spec):
    """The raw input columns the covariance is mean-square differentiable in: those no Matern-1/2 factor sees."""
    d, terms = parse_spec(spec)
    rough = {c for _s, factors in terms for kind, nu2, _a, cols in factors if kind == MATERN and nu2 == 1 for c in cols}
    return [c for c in range(d) if c not in rough]


def first_period(case):
    """The period of the description's first Periodic factor and its column, or None."""
    t = 0
    for scaled, factors in case.terms:
        t += int(scaled)
        for f in factors:
            if f[0] == PERIODIC:
                return float(case.theta[t + 1]), f[3][0]
            t += _factor_ntheta(f)
    return None


# ---- data, in the style of tests/test_gpu_composite.py -------------------------------------------------------------------
def points(rng, k, d):
    """Column 0 sorted uniform in (-4, 4), the others standard normal."""
    t = np.sort(rng.uniform(-4.0, 4.0, k))
    return torch.tensor(np.concatenate([t[:, None], rng.standard_normal((k, d - 1))], axis=1))


@functools.lru_cache(maxsize=None)
def data(index, n, edge=False, seed=0):
    """-> (X (n, d), r (n,), noise (n,)) of case ``index``; shared between tests, never modified.  ``edge`` (n >= 10): row 7
    is a copy of row 3 and X[9, c] = X[5, c] + period for the first Periodic factor (column c), when there is one."""
    case = CASES[index]
    rng = np.random.default_rng(1000 * (seed + 1) + index)
    X = points(rng, n, case.d)
    r = torch.tensor(rng.standard_normal(n))
    noise = torch.full((n,), NOISE, dtype=torch.float64)
    if edge:
        X[7] = X[3]
        per = first_period(case)
        if per is not None:
            X[9, per[1]] = X[5, per[1]] + per[0]
    return X, r, noise


@functools.lru_cache(maxsize=None)
def query_points(index, m, seed=0, coincide=0, n=0, edge=False):
    """(m, d) test points of case ``index``; ``coincide`` > 0: the first that many are training rows 2, 3, ... of
    ``data(index, n, edge)`` (the duplicated and the period-shifted rows among them)."""
    case = CASES[index]
    Xs = points(np.random.default_rng(5000 * (seed + 1) + index), m, case.d)
    if coincide:
        Xs[:coincide] = data(index, n, edge)[0][2:2 + coincide]
    return Xs


# ---- references ------------------------------------------------------------------------------------------------------------
def gram_of(case):
    return orc.composite_gram(list(case.spec))


def part_grams(spec):
    """One Gram function (X1, X2, theta) per additive part: ``composite_gram`` of the one-term sub-description at that
    term's slice of theta -- an unscaled term has no outputscale to zero."""
    d, terms = parse_spec(spec)

    def part(term, lo, hi):
        g = orc.composite_gram(build_spec(d, [term]))
        return lambda X1, X2, theta: g(X1, X2, theta[lo:hi])

    return [part(term, lo, hi) for term, (lo, hi) in zip(terms, term_slices(spec))]


def parts_reference(case, X, r, noise, Xs, theta=None):
    theta = case.theta if theta is None else theta
    return terms_reference(gram_of(case), part_grams(case.spec), X, r, noise, theta, Xs)


def slopes_ref(case, X, r, noise, Xs, cols, theta=None):
    theta = case.theta if theta is None else theta
    return slopes_reference(gram_of(case), composite_prior(list(case.spec)), X, r, noise, theta, Xs, cols)


def plane_errors(mean, cov, ref_mean, ref_cov, scales):
    """``slopes_helpers.errors`` for trees that leave a column unused: the prior variance of that slope is 0, so the plane
    has no scale -- its mean and every covariance with it must then be EXACTLY 0 (error 0, otherwise inf)."""
    from tests.terms_helpers import unpack_cov

    mean, cov = mean.cpu().double(), unpack_cov(cov.cpu().double())
    P = ref_mean.shape[0]
    e_m = max(((mean[a] - ref_mean[a]).abs().max() / ref_mean[a].abs().max().clamp(min=1.0)).item() for a in range(P))
    e_c = 0.0
    for a in range(P):
        for b in range(P):
            diff, den = (cov[a, b] - ref_cov[a, b]).abs().max().item(), float(scales[a] * scales[b])
            e_c = max(e_c, diff / den if den > 0 else (0.0 if diff == 0.0 else float("inf")))
    return e_m, e_c


# ---- gp.kernels trees --------------------------------------------------------------------------------------------------------
def tree_from_spec(spec, theta):
    """The ``gp.kernels`` module tree of a description, its raw parameters set so that the constrained values are ``theta``
    (up to the rounding of softplus and its inverse)."""
    from discontinuum_amd.gp import kernels as K

    d, terms = parse_spec(spec)
    vals = [float(v) for v in theta]
    pos, built = 0, []

    def take(k):
        nonlocal pos
        out = torch.tensor(vals[pos:pos + k], dtype=torch.float64)
        pos += k
        return out

    def fill(param, constraint, value):
        with torch.no_grad():
            param.copy_(constraint.inverse_transform(value).reshape(param.shape))

    for scaled, factors in terms:
        os = take(1) if scaled else None
        mods = []
        for kind, nu2, ard, cols in factors:
            kw = dict(active_dims=list(cols), ard_num_dims=len(cols) if ard else None)
            mod = (K.RBFKernel(**kw) if kind == RBF else K.MaternKernel(nu=nu2 / 2.0, **kw) if kind == MATERN
                   else K.PeriodicKernel(**kw))
            fill(mod.raw_lengthscale, mod.raw_lengthscale_constraint, take(len(cols) if ard else 1))
            if kind == PERIODIC:
                fill(mod.raw_period_length, mod.raw_period_length_constraint, take(1))
            mods.append(mod)
        base = mods[0] if len(mods) == 1 else K.ProductKernel(*mods)
        if scaled:
            base = K.ScaleKernel(base)
            fill(base.raw_outputscale, base.raw_outputscale_constraint, os)
        built.append(base)
    assert pos == len(vals)
    return built[0] if len(built) == 1 else K.AdditiveKernel(*built)


def tree_gram(cov):
    """Gram function (X1, X2) of a ``gp.kernels`` module tree at its own constrained parameter values, by walking the
    modules with ``orc.rbf`` / ``orc.matern`` / ``orc.periodic``; ``composite_spec`` is not involved."""
    from discontinuum_amd.gp import kernels as K

    def walk(k, X1, X2):
        if isinstance(k, K.AdditiveKernel):
            return sum(walk(c, X1, X2) for c in k.kernels)
        if isinstance(k, K.ProductKernel):
            out = 1.0
            for c in k.kernels:
                out = out * walk(c, X1, X2)
            return out
        if isinstance(k, K.ScaleKernel):
            return k.outputscale.detach() * walk(k.base_kernel, X1, X2)
        cols = list(range(X1.shape[1])) if k.active_dims is None else [int(c) for c in k.active_dims]
        a, b, ls = X1[:, cols], X2[:, cols], k.lengthscale.detach().reshape(-1)
        if isinstance(k, K.RBFKernel):
            return orc.rbf(a, b, ls)
        if isinstance(k, K.MaternKernel):
            return orc.matern(a, b, ls, k.nu)
        if isinstance(k, K.PeriodicKernel):
            return orc.periodic(a, b, ls, k.period_length.detach().reshape(()))
        raise TypeError(type(k))

    return lambda X1, X2: walk(cov, X1, X2)
