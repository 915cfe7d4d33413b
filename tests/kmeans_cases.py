"""The case table of the k-means tests (tests/test_kmeans_reference_cpu.py, tests/test_gpu_kmeans.py).  Each case sits on one edge the
kernels of csrc/kmeans.hip can get wrong; the shapes are the smallest that reach it (the assign launch tiles 128 rows x 64 centres x
32 columns, MFMA k-groups of 4; the sort works in chunks of at least 256 rows).

Recipe per case: rng = np.random.default_rng(ord(letter)); X = rng.standard_normal((n, D)) + offset; start rows rng.permutation(n)[:M]."""
import functools

import numpy as np

from tests import kmeans_reference as R

MARGIN = 1e-9
ITERS = (1, 2, 10)

#        n     D    M     offset   edge
CASES = {
    "a": (1000, 8, 37, 0.0),       # ragged centroid tile, two k-steps
    "b": (777, 17, 16, 0.0),       # ragged k-group, ragged last row block
    "c": (600, 100, 50, 0.0),      # D > 64
    "d": (300, 784, 33, 0.0),      # the MNIST width
    "e": (4099, 3, 130, 0.0),      # D < 4, one centroid past 128, many row blocks
    "f": (3000, 6, 513, 0.0),      # one centroid past 512
    "g": (500, 5, 12, 1e6),        # centring
    "h": (257, 1, 5, 0.0),         # D = 1
    "i": (2500, 4, 2048, 0.0),     # the largest M, clusters of one or two rows
}
NAMES = tuple(CASES) + ("dup",)
DUP = 7          # `dup`: centre 7 is an exact copy of centre 3 and must end empty


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(X, start rows, most iterations the case is run for, centres left out of the margin)"""
    if name == "dup":
        rng = np.random.default_rng(5)
        X = rng.standard_normal((400, 6))
        idx = rng.permutation(400)[:20]
        idx[DUP] = idx[3]
        return X, idx, 1, (DUP,)
    n, D, M, offset = CASES[name]
    rng = np.random.default_rng(ord(name))
    X = rng.standard_normal((n, D)) + offset
    idx = rng.permutation(n)[:M]
    return X, idx, max(ITERS), ()


def iters_of(name):
    return (1,) if name == "dup" else ITERS


@functools.lru_cache(maxsize=None)
def reference(name):
    """tests/kmeans_reference.lloyd's per-iteration records, computed once per case and shared (read-only)"""
    X, idx, iters, skip = inputs(name)
    return R.lloyd(X, X[idx], iters, skip=skip)
