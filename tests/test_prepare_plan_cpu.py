"""What a prepare recomputes (csrc/prepare_plan.hpp: the validity record ParamState with its transitions, prep_plan) is pure host code:
this test builds tests/host/prepare_check.cpp with the system C++ compiler under the address and undefined-behaviour sanitizers and runs
it as a process of its own.  The program keeps a ledger of parameter versions per layer and of the versions the factor, the forward-side
and the gradient-side products were computed from, walks every sequence of events (theta moved, a layer's q moved, track_theta on / off,
evaluations with and without a gradient, pruned from every layer, on one or two streams, a saved forward pass and its reverse pass,
ensure_prepared) up to a fixed length for L = 1..3, white or not, on every factorisation route, and exits non-zero on the first
violated invariant: nothing stale is ever kept, and a table of sequences pins what is redone."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prepare_plan_invariants_hold_on_every_sequence(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "prepare_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "doubly-stochastic-dgp_amd", "csrc"), os.path.join(ROOT, "tests", "host", "prepare_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "every invariant holds" in run.stdout
    print(run.stdout.strip())
    walked = re.search(r"(\d+) \(sequence, configuration\) pairs", run.stdout)
    assert walked and int(walked.group(1)) > 1000000, run.stdout
