"""The launch sequence of the blocked Cholesky + triangular inverse (csrc/chol_plan.hpp: chol_route, potrf_lds, chol_plan) is pure host
code: this test builds tests/host/chol_plan_check.cpp with the system C++ compiler under the address and undefined-behaviour sanitizers and
runs it as a process of its own.  The program holds the step lists of six inputs to literal text written from the code the planner
replaced, holds the route to the four expressions it replaced at every n up to 2304, and replays the plan of every legal call at n = 128 ..
2304 against the algorithm: every 64 x 64 tile receives every panel's update exactly once before it is read as final, every block of the
inverse sums every term exactly once from final operands, every operand lies inside its buffer, no launch writes one region twice, the
items accumulate log det and status in order, the grids stay inside their caps.  It exits non-zero on the first violated invariant."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (input, invariant) checks of the first run: 62866 over 9800 replayed plans and 1755 refused calls
CHECKS_FLOOR = 60000
PLANS_FLOOR = 9800


def test_chol_plan_replays_against_the_algorithm(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "chol_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "doubly-stochastic-dgp_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "chol_plan_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"(\d+) plans replayed, (\d+) calls refused, (\d+) checks, every invariant holds", run.stdout)
    assert m, run.stdout
    assert int(m.group(1)) >= PLANS_FLOOR and int(m.group(2)) > 0 and int(m.group(3)) >= CHECKS_FLOOR, run.stdout
