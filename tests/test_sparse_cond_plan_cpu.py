"""The plan of the sparse conditional without q_sqrt (csrc/sparse_cond_plan.hpp: sparse_cond_plan) is pure host code: this test builds
tests/host/sparse_cond_plan_check.cpp with the system C++ compiler under the address and undefined-behaviour sanitizers and runs it as a
process of its own.  The program holds the tiles, chunks and splits of seven shapes to literal numbers, then walks every (n, M, D, DO) of
the case table of tests/sparse_cond_cases.py and a sweep as the two kernels walk them, and exits non-zero on the first violated invariant
(the splits cover every row exactly once, every output and every partial slot is written exactly once, the regions of the scratch are
aligned, disjoint and inside the total, the plan is a function of its four arguments alone)."""
import os
import shutil
import subprocess

import pytest

from tests import sparse_cond_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sparse_cond_plan_covers_every_row_exactly_once(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "sparse_cond_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "doubly-stochastic-dgp_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "sparse_cond_plan_check.cpp"), "-o", exe], check=True)
    shapes = []
    for kind, ard, wv, white, n, M, D, DO, flags in list(SC.CASES.values()) + list(SC.CASES_FWD.values()):
        shapes += [str(n), str(M), str(D), str(DO)]
    run = subprocess.run([exe] + shapes, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "every invariant holds" in run.stdout
