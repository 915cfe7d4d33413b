"""The split-K planner of the reverse pass (csrc/model_plan.hpp: plan_caps, plan_layer, plan_reductions) is pure host code: this
test builds tests/host/plan_check.cpp with the system C++ compiler under the address and undefined-behaviour sanitizers and runs it as
a process of its own.  The program walks a grid of layer shapes, minibatch sizes and DSDGP_FORCE switches over fake base addresses and
exits non-zero on the first violated invariant (task ranges, partial regions inside their buffers and disjoint, capacities, every
result produced exactly once, groups, reduction block ranges)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_invariants_hold_on_the_grid(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "doubly-stochastic-dgp_amd", "csrc"), os.path.join(ROOT, "tests", "host", "plan_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "every invariant holds" in run.stdout
