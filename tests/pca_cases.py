"""The case table of the PCA tests (tests/test_pca_reference_cpu.py, tests/test_gpu_pca.py).  Each case sits on one edge the kernels of
csrc/pca.hip can get wrong; the shapes are the smallest that reach it (the Gram launch tiles C in 64 x 64, MFMA fragments of 16, row
chunks of 32 and row splits of at least 256 rows; the Jacobi step works on 16 x 16 blocks of pairs).

Recipe unless stated: rng = np.random.default_rng(seed); X = rng.standard_normal((n, D)) * np.linspace(1, 3, D).  `boost`: the last k
columns are scaled by a further 2.5, which opens a gap behind the k-th eigenvalue where n >> D (the subspace checks need one)."""
import functools

import numpy as np

from tests import pca_reference as R

GAP = 0.05          # (lam_k - lam_{k+1}) / lam_1 from which the k-dimensional subspace is pinned
JACOBI_MAX_D = 128  # the numpy Jacobi is too slow above

#            n     D     k   center seed  recipe      edge
CASES = {
    "tiny": (5, 3, 2, 0, 1, "plain"),              # odd D, padded pair
    "one_row": (1, 4, 1, 0, 2, "plain"),           # rank 1
    "d1": (7, 1, 1, 0, 3, "plain"),                # no pair at all
    "pair_equal": (2, 2, 1, 0, 0, "pair_equal"),   # X = [[2, 1], [1, 2]]: a_pp = a_qq, 45 degree rotation
    "diag": (64, 16, 4, 0, 0, "diag"),             # X[i, i] = i + 1, else 0: C diagonal, every a_pq = 0 exactly
    "odd17": (257, 17, 5, 0, 4, "plain"),          # ragged row chunk, fragment edge 16 | 17
    "t33": (100, 33, 8, 0, 5, "boost"),            # fragment edge 32 | 33, three blocks of pairs
    "t65": (130, 65, 16, 0, 6, "boost"),           # tile edge 64 | 65: three tiles, one off the diagonal
    "rank": (10, 33, 12, 0, 7, "plain"),           # k above the rank: null-space columns, and the solver must stop
    "dupcol": (50, 6, 3, 0, 8, "dupcol"),          # column 3 a copy of column 1
    "offset": (500, 5, 2, 1, 9, "offset"),         # data + 1e6, center = 1; two row splits
    "c100": (1000, 100, 30, 0, 10, "boost"),       # several row splits
    "split": (4099, 40, 10, 0, 11, "boost"),       # ragged last split
    "wide": (64, 128, 20, 0, 12, "plain"),         # rank-deficient, many steps per sweep
    "mnist_w": (96, 784, 30, 0, 13, "plain"),      # the cfg-4 width
    "max_d": (64, 1024, 32, 0, 14, "plain"),       # the limit
}
NAMES = tuple(CASES)
JACOBI_NAMES = tuple(n for n in NAMES if CASES[n][1] <= JACOBI_MAX_D)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(X, k, center); X is shared: do not write to it"""
    n, D, k, center, seed, recipe = CASES[name]
    if recipe == "pair_equal":
        X = np.array([[2.0, 1.0], [1.0, 2.0]])
    elif recipe == "diag":
        X = np.zeros((n, D))
        X[np.arange(D), np.arange(D)] = np.arange(1.0, D + 1.0)
    else:
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((n, D)) * np.linspace(1.0, 3.0, D)
        if recipe == "boost":
            X[:, D - k:] *= 2.5
        elif recipe == "dupcol":
            X[:, 3] = X[:, 1]
        elif recipe == "offset":
            X = X + 1e6
    X.setflags(write=False)
    return X, k, bool(center)


@functools.lru_cache(maxsize=None)
def truth(name):
    X, _, center = inputs(name)
    return R.truth(X, center)


@functools.lru_cache(maxsize=None)
def jacobi(name):
    assert name in JACOBI_NAMES
    return R.jacobi(truth(name)["C"])


def gap(name):
    """(lam_k - lam_{k+1}) / lam_1, or 0 where k = D"""
    lam, k = truth(name)["lam"], CASES[name][2]
    return float((lam[k - 1] - lam[k]) / lam[0]) if k < lam.shape[0] else 0.0


def gapped(name):
    return gap(name) >= GAP


def projector_bar(name):
    """D 2^-52 |C|_F / (lam_k - lam_{k+1}) of a gapped case"""
    tr, (_, D, k) = truth(name), CASES[name][:3]
    return D * R.EPS * tr["normF"] / (tr["lam"][k - 1] - tr["lam"][k])
