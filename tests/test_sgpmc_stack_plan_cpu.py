"""The plan of the stack of sparse sampled layers (csrc/sgpmc_stack_plan.hpp: sgpmc_stack_plan) is pure host code: this test builds
tests/host/sgpmc_stack_plan_check.cpp with the system C++ compiler under the address and undefined-behaviour sanitizers and runs it as a
process of its own.  The program walks every stack of the case table of tests/sgpmc_stack_cases.py, the benchmark shape held to literal
numbers and a sweep, forward-only and with the reverse's regions, and exits non-zero on the first violated invariant (the regions of the
scratch are aligned, disjoint, large enough and inside the total; every entry of every F, every row and every partial slot is met
exactly once; shapes that do not chain are refused; the plan is a function of its arguments alone)."""
import os
import shutil
import subprocess

import pytest

from tests import sgpmc_stack_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sgpmc_stack_plan_regions_and_launches(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "sgpmc_stack_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "doubly-stochastic-dgp_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "sgpmc_stack_plan_check.cpp"), "-o", exe], check=True)
    args = []
    for name in KC.NAMES + [KC.FORWARD_ONLY]:
        args += [str(a) for a in KC.shape_args(name)]
    run = subprocess.run([exe] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "%d stacks from the command line" % (len(KC.NAMES) + 1) in run.stdout and "every invariant holds" in run.stdout
