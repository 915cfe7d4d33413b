"""The plan of the pathwise draws (csrc/pathwise_plan.hpp: pathwise_plan, pathwise_scratch) is pure host code: this test builds
tests/host/pathwise_plan_check.cpp with the system C++ compiler under the address and undefined-behaviour sanitizers and runs it as a
process of its own.  The program holds the chunk counts of six shapes to literal numbers, then walks every (L, M, D, DO, S) of the case
table of tests/pathwise_cases.py and a sweep as k_pw_eval walks them, and exits non-zero on the first violated invariant (the chunks cover
every frequency, input dimension, inducing row and output exactly once, no staged index leaves its LDS array, the LDS bytes are within the
limit, the regions of the scratch are aligned, disjoint and inside the total, the plans are functions of their arguments alone — neither
takes the row count, and the kernel's takes no draw count)."""
import os
import shutil
import subprocess

import pytest

from tests import pathwise_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pathwise_plan_covers_every_index_exactly_once(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "pathwise_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "doubly-stochastic-dgp_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "pathwise_plan_check.cpp"), "-o", exe], check=True)
    shapes = []
    for kind, ard, wv, white, n, L, D, M, DO, S, per_draw, add, flags in PC.CASES.values():
        shapes += [str(L), str(M), str(D), str(DO), str(S)]
    run = subprocess.run([exe] + shapes, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "every invariant holds" in run.stdout
