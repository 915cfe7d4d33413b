"""The plan of the reverse pass of the Gram matrix (csrc/gram_grad_plan.hpp: gram_grad_plan) is pure host code: this test builds
tests/host/gram_grad_plan_check.cpp with the system C++ compiler under the address and undefined-behaviour sanitizers and runs it as a
process of its own.  The program holds the row blocks and column splits of nine shapes to literal numbers, then walks every (n, n2, D)
of the case table of tests/gram_grad_cases.py and a sweep of n, n2 <= 300 as the kernel walks them and exits non-zero on the first
violated invariant (every row and column pair met exactly once, every partial row written exactly once, no index outside its matrix,
regions aligned, disjoint and inside the total, the plan a function of (n, n2, D, form) alone)."""
import os
import shutil
import subprocess

import pytest

from tests import gram_grad_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gram_grad_plan_covers_every_pair_exactly_once(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "gram_grad_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "doubly-stochastic-dgp_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "gram_grad_plan_check.cpp"), "-o", exe], check=True)
    shapes = []
    for kind, sym, n, n2, D, *_ in GC.CASES.values():
        shapes += [str(n), "0" if sym else str(n2), str(D)]
    run = subprocess.run([exe] + shapes, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "every invariant holds" in run.stdout
