"""The small two-layer models that tests/test_gpu_evaluate.py and tests/test_gpu_calibration.py score, built once per process, and the
child-process runner both files use for the switches that are read when the device model is created."""
import json
import os
import subprocess
import sys

import numpy as np

from tests.helpers import kern_spec, make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS, S_MAX = 37, 37
_cases = {}


def _build_case(name):
    """two layers, D_in = 2, M = 16, inner width 2; (model, Xs, Ys, zs for S_MAX samples)"""
    rng = np.random.RandomState(5)
    N, D, M = 40, 2, 16
    X = rng.randn(N, D)
    Z = X[:M] + 0.01 * rng.randn(M, D)
    kw, DY = {}, 2
    if name == "rbf":
        specs, Y, Ys = [kern_spec("rbf", D, 1.2, 0.9)] * 2, rng.randn(N, DY), rng.randn(NS, DY)
    elif name == "matern_white":
        DY = 1
        specs, Y, Ys, kw = [kern_spec("matern52", D, 0.9, 1.1)] * 2, rng.randn(N, DY), rng.randn(NS, DY), dict(white=True)
    elif name == "bernoulli":
        specs, kw = [kern_spec("rbf", D, 1.2, 0.9)] * 2, dict(bernoulli=True)
        Y, Ys = rng.choice([-1.0, 1.0], N * DY).reshape(N, DY), rng.choice([-1.0, 1.0], NS * DY).reshape(NS, DY)
    else:
        DY = 3
        specs, kw = [kern_spec("rbf", D, 1.2, 0.9)] * 2, dict(num_classes=3)
        Y, Ys = rng.randint(0, 3, size=(N, 1)).astype(np.float64), rng.randint(0, 3, size=(NS, 1)).astype(np.float64)
    _, _, model = make_case(X, Y, Z, specs, lik_var=0.1, S=3, **kw)
    Xs = rng.randn(NS, D)
    zs = [rng.randn(S_MAX, NS, 2), rng.randn(S_MAX, NS, DY)]
    return model, Xs, Ys, zs


def _case(name):
    if name not in _cases:
        _cases[name] = _build_case(name)
    return _cases[name]


def run_child(snippet, env_extra):
    """`snippet` (argv: the repository root, the package directory) in a fresh process without DSDGP_FORCE / DSDGP_NO_OVERLAP but with
    env_extra -> the JSON of its last stdout line"""
    env = dict(os.environ)
    env.pop("DSDGP_FORCE", None)
    env.pop("DSDGP_NO_OVERLAP", None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", snippet, ROOT, os.path.join(ROOT, "doubly-stochastic-dgp_amd")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])
