"""What a forward pass launches and keeps (csrc/forward_plan.hpp: fwd_plan and the record for the reverse pass; csrc/chain_policy.hpp: the
size rules) is pure host code: this test builds tests/host/forward_check.cpp with the system C++ compiler under the address and
undefined-behaviour sanitizers and runs it as a process of its own.  The program holds fwd_plan, field by field, to a transcription of
the conditions the forward pass took inline before the plan existed, over a grid that straddles every threshold of the rules (padded
inducing counts 32..1024, input widths 1..65, outputs 1..30, row blocks around 160 / 256 / 512 / 768 for the first and for the inner
layers, L = 1..5, every kind of call, likelihood, gradient set, subset of caller draws and forward-side DSDGP_FORCE setting); checks
invariants that do not depend on the transcription and the record's transitions; and pins the plans of the benchmark configurations.
It exits non-zero on the first violation."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_forward_plan_equals_the_inline_decisions_on_every_input(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "forward_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "doubly-stochastic-dgp_amd", "csrc"), os.path.join(ROOT, "tests", "host", "forward_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "every invariant holds" in run.stdout
    print(run.stdout.strip())
    walked = re.search(r"(\d+) inputs walked", run.stdout)
    assert walked and int(walked.group(1)) > 700000, run.stdout      # about half of what the grid comes to
