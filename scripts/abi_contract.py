"""Record what the engine's host layer promises without a device: every workspace size and every refusal.

    python scripts/abi_contract.py --write tests/abi_contract.json      # from the build whose behaviour is the contract
    python scripts/abi_contract.py --compare tests/abi_contract.json    # (tests/test_abi_contract.py does the same)

Two tables, from whatever libdgp_hip.so the package loads:

  sizes      every *_workspace_bytes query of _lib.SIGNATURES, dgp_plan_workspace_bytes and dgp_plan_site_stride_bytes, on plans
             that were created but never given a workspace (dgp_plan_create / dgp_plan_set_batch make no device call), over GRID,
             plus one out-of-range value per size parameter and the plans a query answers with 0.  Host arithmetic only.
  refusals   for every int-returning entry: a null plan (stateless entries: a bad dtype), a plan without workspace with every
             other argument null, and the same with one out-of-range size per integer parameter -> (return code, error text).

Every argument that stands for a device address is None and every recorded call must be refused: the recorder stops at a call
that returns 0.  record_refusals() is for a machine WITHOUT a GPU (a wrongly accepted call then cannot become a launch); the
caller checks that.
"""
from __future__ import annotations

import argparse
import ctypes as C
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from discontinuum_amd import _lib  # noqa: E402

MODELS = ((_lib.MODEL_LOADEST, 3), (_lib.MODEL_RATING, 2))
GRID = {
    "dtype": (_lib.F64, _lib.F32),
    "n": (129, 300, 1000),
    "batch": (1, 3, 9),  # 9 brings in the hyperparameter scratch
    "m": (1, 200, 257),
    "ngroups": (1, 4),
    "nlevels": (1, 2),
    "panel_rows": (128, 256),
    "ndiag": (0, 2),
    "nrhs": (0, 2),
    "nrows": (0, 2),
}
# values a query must answer with 0 (or, for an entry point, refuse): one at a time against the first valid value of the others
BAD = {
    "m": (0, (1 << 20) + 1),
    "q": (0, (1 << 20) + 1),
    "ngroups": (0, 65536),
    "nlevels": (0, 65),
    "nterms": (0, 65),
    "panel_rows": (0, 100),
    "ndiag": (-1, 9),
    "nrhs": (-1, 9),
    "nrows": (-1, 65),
    "ncols": (0, "d+1"),
    "folds": (0, "n+1"),
    "max_group": (0, "n+1"),
    "sbatch": (0, 1025),
}
# query -> its parameters after the plan (PLAN_QUERIES) or all of them (STATELESS_QUERIES)
PLAN_QUERIES = {
    "dgp_plan_workspace_bytes": (),
    "dgp_plan_site_stride_bytes": (),
    "dgp_laplace_workspace_bytes": (),
    "dgp_laplace_batched_workspace_bytes": (),
    "dgp_ep_workspace_bytes": (),
    "dgp_loo_workspace_bytes": (),
    "dgp_loo_value_workspace_bytes": (),
    "dgp_predict_workspace_bytes": ("m",),
    "dgp_predict_terms_workspace_bytes": ("m",),
    "dgp_mean_vjp_workspace_bytes": ("m",),
    "dgp_predict_slopes_workspace_bytes": ("m", "ncols"),
    "dgp_posterior_period_moments_workspace_bytes": ("m", "ngroups"),
    "dgp_posterior_exceedance_moments_workspace_bytes": ("m", "ngroups", "nlevels", "panel_rows"),
    "dgp_cross_validate_workspace_bytes": ("folds", "max_group"),
    "dgp_laplace_cross_validate_workspace_bytes": ("folds", "max_group"),
    "dgp_fisher_workspace_bytes": ("ndiag",),
    "dgp_predict_sensitivity_workspace_bytes": ("m", "ndiag", "nrhs"),
    "dgp_deletion_influence_workspace_bytes": ("m", "folds", "max_group", "ngroups"),
}
STATELESS_QUERIES = {
    "dgp_period_moments_workspace_bytes": ("m", "ngroups", "sbatch"),
    "dgp_period_third_moments_workspace_bytes": ("m", "ngroups", "sbatch"),
    "dgp_window_moments_workspace_bytes": ("m", "q", "sbatch"),
    "dgp_exceedance_moments_workspace_bytes": ("m", "ngroups", "nlevels", "sbatch"),
    "dgp_sample_value_workspace_bytes": ("m", "ngroups", "nrows", "nterms", "sbatch"),
}
DIST_GRID = {"world": (1, 2), "group_panels": (1, 2)}

# int-returning entries that are no refusal channel: pure queries, and the two constructors (recorded by hand below)
NOT_ENTRIES = {"dgp_version", "dgp_model_ntheta", "dgp_model_nterms", "dgp_model_input_differentiable", "dgp_plan_batch",
               "dgp_plan_destroy", "dgp_dist_destroy", "dgp_dist_groups", "dgp_plan_create", "dgp_dist_create", "dgp_composite_define"}
# host-side bookkeeping that a plan without workspace ACCEPTS: recorded with a null plan only
HOST_ONLY = {"dgp_plan_set_lookahead", "dgp_plan_set_option", "dgp_plan_get_option", "dgp_plan_set_batch", "dgp_plan_set_dr_weights",
             "dgp_plan_set_timing"}
# entries whose first argument is not a plan or a dtype: every pointer null, once
POINTER_FIRST = {"dgp_debug_interval_terms", "dgp_debug_censored_terms", "dgp_debug_bvn_excess", "dgp_debug_clock_probe"}
INT_TYPES = (C.c_int, C.c_int64, C.c_size_t)


def values(name, n, d):
    if name in GRID:
        return GRID[name]
    return {"q": GRID["m"], "nterms": GRID["nlevels"], "sbatch": GRID["batch"], "ncols": tuple(range(1, d + 1)), "folds": (1, 5, n),
            "max_group": (1, 64, 65, n)}[name]  # max_group: across CV_SMALL_GROUP


def bad_values(name, n, d):
    return tuple({"d+1": d + 1, "n+1": n + 1}.get(v, v) for v in BAD[name])


def argument_sets(params, n, d):
    """The grid's product, then every out-of-range value against the first valid value of the other parameters."""
    sets = list(itertools.product(*(values(q, n, d) for q in params)))
    base = [values(q, n, d)[0] for q in params]
    for k, q in enumerate(params):
        for v in bad_values(q, n, d):
            sets.append(tuple(base[:k] + [v] + base[k + 1:]))
    return sets


def make_plan(lib, model, d, dtype, n, batch):
    h = C.c_void_p()
    assert lib.dgp_plan_create(model, dtype, n, d, C.byref(h)) == 0
    assert lib.dgp_plan_set_batch(h, batch) == 0
    return h


def record_sizes(lib):
    sizes = {}
    listed = set(PLAN_QUERIES) | set(STATELESS_QUERIES) | {"dgp_dist_workspace_bytes"}
    wanted = {k for k in _lib.SIGNATURES if k.endswith("_workspace_bytes")} | {"dgp_plan_site_stride_bytes"}
    assert wanted == listed, sorted(wanted ^ listed)
    for (model, d), dtype, n, batch in itertools.product(MODELS, GRID["dtype"], GRID["n"], GRID["batch"]):
        h = make_plan(lib, model, d, dtype, n, batch)
        row = sizes[f"model={model} d={d} dtype={dtype} n={n} batch={batch}"] = {}
        for name, params in PLAN_QUERIES.items():
            row[name] = [int(getattr(lib, name)(h, *a)) for a in argument_sets(params, n, d)]
        lib.dgp_plan_destroy(h)
    row = sizes["null plan"] = {}
    for name, params in PLAN_QUERIES.items():
        row[name] = [int(getattr(lib, name)(None, *(values(q, 300, 3)[0] for q in params)))]
    row = sizes["stateless"] = {}
    for name, params in STATELESS_QUERIES.items():
        row[name] = [int(getattr(lib, name)(*a)) for a in argument_sets(params, 300, 3)]
    row = sizes["dist"] = {}
    for (model, d), dtype, n, world, gp in itertools.product(MODELS, GRID["dtype"], GRID["n"], DIST_GRID["world"],
                                                             DIST_GRID["group_panels"]):
        h = C.c_void_p()
        assert lib.dgp_dist_create(model, dtype, n, d, 0, world, gp, C.byref(h)) == 0
        row[f"model={model} d={d} dtype={dtype} n={n} world={world} group_panels={gp}"] = int(lib.dgp_dist_workspace_bytes(h))
        lib.dgp_dist_destroy(h)
    row["null"] = int(lib.dgp_dist_workspace_bytes(None))
    return sizes


def record_refusals(lib):
    """Only on a machine without a GPU.  Every pointer argument is None; stops at a call that is not refused."""
    out = {}

    def call(key, name, args):
        err = lib.dgp_dist_last_error if name.startswith("dgp_dist_") else lib.dgp_last_error
        rc = int(getattr(lib, name)(*args))
        if rc == 0:
            raise RuntimeError(f"abi_contract: {key} was ACCEPTED (rc 0): not a refusal, nothing more is called")
        out[key] = [rc, err().decode("utf-8", "replace")]

    def null_args(types, first):
        return [first] + [0 if t in INT_TYPES else (0.0 if t is C.c_double else None) for t in types[1:]]

    plans = {"f64": make_plan(lib, _lib.MODEL_LOADEST, 3, _lib.F64, 300, 1), "f32": make_plan(lib, _lib.MODEL_LOADEST, 3, _lib.F32, 300, 1),
             "f64x3": make_plan(lib, _lib.MODEL_LOADEST, 3, _lib.F64, 300, 3)}
    dist = C.c_void_p()
    assert lib.dgp_dist_create(_lib.MODEL_LOADEST, _lib.F64, 300, 3, 0, 1, 1, C.byref(dist)) == 0
    for name, (res, types) in _lib.SIGNATURES.items():
        if res is not C.c_int or name in NOT_ENTRIES:
            continue
        if name in POINTER_FIRST:
            call(f"{name}|null", name, null_args(types, None))
            continue
        if name.startswith("dgp_debug_") and types[0] is C.c_int:  # (dtype, ...) diagnostics: the bad dtype only
            call(f"{name}|dtype=7", name, null_args(types, 7))
            continue
        stateless = types[0] is C.c_int
        call(f"{name}|{'dtype=7' if stateless else 'null plan'}", name, null_args(types, 7 if stateless else None))
        if name in HOST_ONLY:
            continue
        firsts = {"f64": 0, "f32": 1} if stateless else ({"dist": dist} if name.startswith("dgp_dist_") else plans)
        for tag, first in firsts.items():
            call(f"{name}|{tag}|null arguments", name, null_args(types, first))
            for k in range(1, len(types)):
                if types[k] not in INT_TYPES:
                    continue
                for bad in (-1, 1 << 30):
                    if types[k] is C.c_size_t and bad < 0:
                        continue
                    args = [1 if (t in INT_TYPES and j > 0) else a for j, (t, a) in enumerate(zip(types, null_args(types, first)))]
                    args[k] = bad
                    call(f"{name}|{tag}|arg{k}={bad}", name, args)
    # the constructors
    h = C.c_void_p()
    for key, args in (("null out", (0, 0, 300, 3, None)), ("n=0", (0, 0, 0, 3, C.byref(h))), ("n=2^20+1", (0, 0, (1 << 20) + 1, 3, C.byref(h))),
                      ("dtype=7", (0, 7, 300, 3, C.byref(h))), ("model=7", (7, 0, 300, 3, C.byref(h))), ("d=9", (0, 0, 300, 9, C.byref(h)))):
        call(f"dgp_plan_create|{key}", "dgp_plan_create", args)
    for key, args in (("null out", (0, 0, 300, 3, 0, 1, 1, None)), ("n=0", (0, 0, 0, 3, 0, 1, 1, C.byref(h))),
                      ("dtype=7", (0, 7, 300, 3, 0, 1, 1, C.byref(h))), ("rank=1 world=1", (0, 0, 300, 3, 1, 1, 1, C.byref(h))),
                      ("group_panels=9", (0, 0, 300, 3, 0, 1, 9, C.byref(h))), ("model=7", (7, 0, 300, 3, 0, 1, 1, C.byref(h)))):
        call(f"dgp_dist_create|{key}", "dgp_dist_create", args)
    call("dgp_composite_define|null", "dgp_composite_define", (None, 0, None))
    for p in plans.values():
        lib.dgp_plan_destroy(p)
    lib.dgp_dist_destroy(dist)
    return out


def differences(want, got, path=""):
    if isinstance(want, dict) and isinstance(got, dict):
        for k in sorted(set(want) | set(got)):
            if k not in want or k not in got:
                yield f"{path}/{k}: only in the {'fixture' if k in want else 'library'}"
            else:
                yield from differences(want[k], got[k], f"{path}/{k}")
    elif want != got:
        yield f"{path}: fixture {want!r} != library {got!r}"


def save(table, path):
    """The file holds the tables without their repetition, one line per query / entry: the plans' size tables as
    query -> one list per plan (in the order of "plans"), the refusals as entry -> "code|text" -> the calls that got it."""
    plans = [k for k in table["sizes"] if k.startswith("model=")]
    packed = {"plans": plans,
              "plan_sizes": {q: [table["sizes"][p][q] for p in plans] for q in PLAN_QUERIES},
              "sizes": {k: v for k, v in table["sizes"].items() if k not in plans},
              "refusals": {}}
    for key, (rc, text) in table["refusals"].items():
        name, _, tag = key.partition("|")
        packed["refusals"].setdefault(name, {}).setdefault(f"{rc}|{text}", []).append(tag)
    dump = lambda v: json.dumps(v, sort_keys=True, separators=(",", ":"))  # noqa: E731
    with open(path, "w") as f:
        f.write("{\n")
        for top in ("plan_sizes", "plans", "refusals", "sizes"):
            rows = packed[top]
            body = ",\n".join(dump(k) + ":" + dump(rows[k]) for k in sorted(rows)) if isinstance(rows, dict) else ",\n".join(map(dump, rows))
            f.write(f"{dump(top)}:{'{' if isinstance(rows, dict) else '['}\n{body}\n{'}' if isinstance(rows, dict) else ']'}"
                    f"{'' if top == 'sizes' else ','}\n")
        f.write("}\n")


def load(path):
    """-> the tables as record_sizes / record_refusals return them."""
    with open(path) as f:
        packed = json.load(f)
    sizes = dict(packed["sizes"])
    for i, plan in enumerate(packed["plans"]):
        sizes[plan] = {q: rows[i] for q, rows in packed["plan_sizes"].items()}
    refusals = {}
    for name, answers in packed["refusals"].items():
        for answer, tags in answers.items():
            rc, _, text = answer.partition("|")
            for tag in tags:
                refusals[f"{name}|{tag}"] = [int(rc), text]
    return {"sizes": sizes, "refusals": refusals}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", metavar="FILE")
    ap.add_argument("--compare", metavar="FILE")
    a = ap.parse_args()
    if bool(a.write) == bool(a.compare):
        ap.error("exactly one of --write / --compare")
    if os.path.exists("/dev/kfd"):
        raise SystemExit("abi_contract: a GPU is visible; the refusal table is recorded on a machine without one")
    lib = _lib.load()
    table = {"sizes": record_sizes(lib), "refusals": record_refusals(lib)}
    if a.write:
        save(table, a.write)
        print(f"{a.write}: {len(table['sizes'])} size tables, {len(table['refusals'])} refusals")
        return 0
    diffs = list(differences(load(a.compare), table))
    for line in diffs[:40]:
        print(line)
    print("identical" if not diffs else f"{len(diffs)} difference(s)")
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
