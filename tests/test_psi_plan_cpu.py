"""The plan of the RBF kernel expectations and of their reverse pass (csrc/psi_plan.hpp: psi_plan_forward, psi_plan_reverse) is pure
host code: this test builds tests/host/psi_plan_check.cpp with the system C++ compiler under the address and undefined-behaviour
sanitizers and runs it as a process of its own.  The program holds the row splits and chunks of twelve shapes to literal numbers, then
walks a grid of (n, M, D) and of what the caller asks for and exits non-zero on the first violated invariant (no empty split or chunk,
regions aligned, disjoint, inside the total and large enough for their kernels, nothing taken for what is not asked for, no wrap)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_psi_plan_invariants_hold_on_the_grid(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "psi_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "doubly-stochastic-dgp_amd", "csrc"), os.path.join(ROOT, "tests", "host", "psi_plan_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "every invariant holds" in run.stdout
