"""The case table of the greedy inducing-point tests (tests/test_greedy_reference_cpu.py, tests/test_gpu_greedy.py).  Each case sits
on an edge the kernels of csrc/greedy.hip can get wrong; the shapes are the smallest that reach it (a one-wave workgroup sweeps chunks
of 128 rows, two per lane; the stream rows — D of the transposed data, j of the column store — are consumed 16 at a time; from 2048
chunks on, n > 262 144, a workgroup takes more than one chunk).

Recipe per case: rng = np.random.default_rng(sum(ord(c) for c in name)); X = rng.standard_normal((n, D)) + offset; ARD lengthscales
l (1 + 0.5 u_d) with u = rng.random(D) drawn after X.  The lengthscales are long enough that no kernel value between two rows
underflows: with short ones every far row keeps d = v - tiny and the arg-max is a coin toss.  `dup`: 500 rows drawn (rng.integers)
from 20 distinct ones; with threshold 1e-6 the selection stops at m = 20.

MARGIN: the k-means tests' figure.  A residual drifts by about 2 j^2 2^-53 v under a different summation order — 6e-11 at j = 520,
2e-13 at j <= 33 — so every case keeps its margin (tests/greedy_reference.py) above 1e-9; one that does not gets another seed."""
import functools

import numpy as np

from tests import greedy_reference as R

MARGIN = 1e-9

#         n      D    M    kind        ard    v    l     extras
CASES = {
    "a": (600, 3, 40, "rbf", False, 1.3, 2.5, {}),
    "b": (1000, 8, 130, "matern52", True, 0.7, 1.5, {}),
    "c": (2049, 1, 33, "matern52", False, 2.0, 0.7, {}),            # one row past 16 chunks, one column past two buffers
    "d": (4100, 17, 257, "matern52", True, 1.0, 3.0, {}),           # D one past a buffer, M one past 16 buffers
    "e": (3000, 64, 520, "rbf", False, 1.0, 6.0, {}),
    "off": (900, 5, 64, "rbf", False, 1.0, 3.0, {"offset": 1e6}),   # differences of rows, not |x|^2 + |z|^2 - 2 x.z
    "wide": (700, 784, 48, "rbf", False, 1.0, 25.0, {}),            # the MNIST width
    "tiny": (17, 2, 16, "rbf", False, 1.0, 1.5, {}),                # nearly every row, last residual about 1e-6 v
    "big": (20000, 8, 128, "rbf", False, 1.0, 2.0, {}),
    "dup": (500, 4, 32, "rbf", False, 1.0, 1.5, {"distinct": 20, "threshold": 1e-6}),
    "white": (400, 3, 24, "rbf", False, 0.9, 2.0, {"white": 0.05}),
    "first": (500, 4, 30, "matern52", False, 1.1, 2.0, {"first": 123}),
    "edge": (257, 2, 17, "rbf", True, 1.0, 1.2, {}),                # one row past two chunks, one column past a buffer
    "long": (262273, 1, 3, "rbf", False, 1.0, 1.5, {}),             # 2050 chunks: two per workgroup, 1025 partials to fold
}
NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict(X, M, kind, ard, v, ls (array of 1 or D), white, first, threshold)"""
    n, D, M, kind, ard, v, l, extra = CASES[name]
    rng = np.random.default_rng(sum(ord(c) for c in name))
    if "distinct" in extra:
        base = rng.standard_normal((extra["distinct"], D))
        X = base[rng.integers(0, extra["distinct"], n)]
    else:
        X = rng.standard_normal((n, D)) + extra.get("offset", 0.0)
    ls = l * (1.0 + 0.5 * rng.random(D)) if ard else np.array([l])
    X.setflags(write=False)
    return dict(X=X, M=M, kind=kind, ard=ard, v=v, ls=ls, white=extra.get("white", 0.0), first=extra.get("first"),
                threshold=extra.get("threshold", 0.0))


def _run(name, dtype):
    c = inputs(name)
    return R.greedy(c["X"], c["M"], c["kind"], c["v"], c["ls"], white=c["white"], first=c["first"], threshold=c["threshold"], dtype=dtype)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the long-double run, computed once per case and shared (read-only)"""
    return _run(name, R.LD)


@functools.lru_cache(maxsize=None)
def float64(name):
    """the plain float64 run"""
    return _run(name, np.float64)


def kernel_of(name):
    """the gpflow_compat kernel of a case"""
    from doubly_stochastic_dgp.gpflow_compat import RBF, Matern52, White
    c = inputs(name)
    D = c["X"].shape[1]
    cls = RBF if c["kind"] == "rbf" else Matern52
    k = cls(D, variance=c["v"], lengthscales=c["ls"] if c["ard"] else float(c["ls"][0]), ARD=c["ard"])
    return k + White(D, variance=c["white"]) if c["white"] else k
