"""The batched factorisation's schedule is data (discontinuum_amd/csrc/dgp_schedule.h: a list of UPDATE / PANELS / SOLVE /
SYNC launches) with a host-side checker: every tile receives its k-blocks in ascending gap-free order exactly once before
its column is factored, nothing reads a block column before it is final, accesses across the two streams are ordered.  That
invariant is what makes the left-looking schedule's fp64 factor bitwise the group-ahead one's (a trailing tile starts at -C
and continues ONE k-ordered fma chain, csrc/dgp_gemm.h::trailing_begin), so it is checked without a GPU: the header has no
HIP in it, and examples/potrf_schedule_check.cpp -- compiled here with g++ -- runs the checker over today's schedule, the
pure left-looking one, the default cut and the hybrid cuts for every nbk in 4..80 and G in {2, 4, 8} (ragged last group
included), and over hand-made violations that it must reject (a skipped k-block, a descending order, a column factored
early, a k-block applied twice, a read of a column that is not final, a missing group, missing cross-stream waits).
What the schedule restates: the Cholesky inside the reference's `mll(output, y)`, engines/gpytorch.py:350-353."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "discontinuum_amd", "csrc")


def build_checker(out_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "examples", "potrf_schedule_check.cpp"), "-o", str(out_path)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr


def test_schedule_header_has_no_hip_in_it():
    text = open(os.path.join(CSRC, "dgp_schedule.h")).read()
    assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text


def test_checker_accepts_the_schedules_and_rejects_violations(tmp_path):
    exe = tmp_path / "potrf_schedule_check"
    build_checker(exe)
    run = subprocess.run([str(exe), "4", "80"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    last = run.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and "FAIL" not in run.stdout
    # 77 sizes x 3 group sizes x (today + left-looking + default + 4 x 3 x 2 x 3 hybrid cuts); violations wherever there are >= 3 groups
    assert int(last[1]) == 77 * 3 * (3 + 72)
    assert int(last[2]) >= 77 * 3 * 5


def test_option_keys_are_the_next_free_ones():
    from discontinuum_amd import _lib

    assert (_lib.OPT_POTRF_SCHEDULE, _lib.OPT_POTRF_SWEEP, _lib.OPT_POTRF_SOLVE, _lib.OPT_POTRF_OVERLAP, _lib.OPT_POTRF_SLOTS, _lib.OPT_POTRF_TAIL,
            _lib.OPT_POTRF_TAIL_SWEEP) == (9, 10, 11, 12, 13, 14, 15)
    header = open(os.path.join(ROOT, "include", "dgp_hip.h")).read()
    for name, key in (("SCHEDULE", 9), ("SWEEP", 10), ("SOLVE", 11), ("OVERLAP", 12), ("SLOTS", 13), ("TAIL", 14), ("TAIL_SWEEP", 15)):
        assert f"#define DGP_OPT_POTRF_{name} {key}" in header
