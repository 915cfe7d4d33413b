"""The case table of the sparse conditional without q_sqrt (tests/test_gpu_sparse_cond.py, tests/test_sparse_cond_plan_cpu.py): one case
on each side of every threshold of csrc/sparse_cond.hip and csrc/sparse_cond_plan.hpp —
    the column tile of 64 rows of X:       n = 1, 63, 64, 65, 129
    the row split: one tile per split up to 256 tiles, two from 257 on:  n = 16384 (256 tiles), 16391 (257 tiles: 129 splits, the last of one)
    the chunk of 64 rows of A:             M = 1, 15, 16, 17, 33, 50, 64, 65
    the chunk of 16 outputs:               DO = 1, 15, 16, 17, 33;  the 64 outputs a wave holds: DO = 64, 65 (a second sweep over A)
    the input width:                       D = 1, 8, 32 in both calls; D = 33 forward only (the reverse refuses it)
— and across the table both kernels, scalar and ARD lengthscales, a White part, both `white`, rows of X equal to rows of Z, data at an
offset of 1e6, a row of X so far away that every exponential underflows, gv = 0 and gm = 0.

The jitter is variance M / 50: cond(Ku) <= (variance M + jitter) / jitter = 51, so that what the factorisation loses — cond(Ku) u on any
route, the device's or numpy's — stays below what the bar resolves (the same choice as tests/test_gpu_dense_layers.py; the
factorisation on ill-conditioned matrices has its own tests).  The long-double truth and its float64 twin are computed once per case."""
import functools

import numpy as np

from tests import sparse_cond_reference as SR

RBF, MATERN52 = 0, 1
VARIANCE = 1.3

#            kind      ard white_var white  n      M   D   DO  flags
CASES = {
    "n1":       (RBF,      0, None, True,  1,     5,  2,  1,  ()),
    "n63":      (MATERN52, 1, None, False, 63,    15, 3,  2,  ()),
    "n64":      (RBF,      1, 0.2,  True,  64,    16, 8,  15, ()),
    "n65":      (RBF,      0, None, False, 65,    17, 1,  16, ()),
    "n129":     (MATERN52, 0, 0.3,  False, 129,   33, 8,  17, ()),
    "m1":       (RBF,      0, None, False, 20,    1,  2,  3,  ()),
    "m50":      (MATERN52, 1, None, True,  70,    50, 3,  33, ()),
    "m64":      (RBF,      1, None, True,  40,    64, 2,  2,  ()),
    "m65":      (RBF,      0, 0.1,  False, 66,    65, 2,  1,  ()),
    "do64":     (RBF,      1, None, False, 33,    17, 2,  64, ()),
    "do65":     (MATERN52, 0, None, True,  70,    20, 2,  65, ()),
    "d32":      (RBF,      1, None, True,  30,    9,  32, 2,  ()),
    "d32m":     (MATERN52, 0, 0.2,  False, 67,    12, 32, 1,  ()),
    "zrows":    (RBF,      1, None, False, 40,    12, 3,  2,  ("zrows",)),
    "zrows_m":  (MATERN52, 0, None, True,  40,    12, 3,  2,  ("zrows",)),
    "offset":   (RBF,      1, None, False, 70,    10, 2,  2,  ("offset",)),
    "far":      (RBF,      0, None, True,  20,    6,  2,  2,  ("far",)),
    "gv0":      (MATERN52, 1, 0.2,  False, 65,    17, 3,  2,  ("gv0",)),
    "gm0":      (RBF,      1, None, False, 65,    17, 3,  2,  ("gm0",)),
    "t256":     (RBF,      0, None, True,  16384, 3,  1,  1,  ()),
    "t257":     (MATERN52, 0, None, False, 16391, 3,  1,  2,  ()),
}
NAMES = list(CASES)
FORWARD_ONLY = "d33"          # the forward takes it, the reverse refuses it
CASES_FWD = {FORWARD_ONLY: (RBF, 1, None, False, 20, 7, 33, 2, ())}
FAR_ROW = 7


def inputs(name):
    kind, ard, wv, white, n, M, D, DO, flags = (CASES.get(name) or CASES_FWD[name])
    rng = np.random.default_rng(sum(map(ord, name)) + 7 * n + M)
    Z, X = rng.standard_normal((M, D)), rng.standard_normal((n, D))
    if "zrows" in flags:
        X[::3][:M // 2] = Z[:len(X[::3][:M // 2])]
    if "far" in flags:
        X[FAR_ROW] += 1e3                  # every exponential of this row underflows
    if "offset" in flags:
        Z, X = Z + 1e6, X + 1e6
    ls = np.sqrt(D) * rng.uniform(0.7, 1.4, D if ard else 1)
    q_mu, gm, gv = rng.standard_normal((M, DO)), rng.standard_normal((n, DO)), rng.standard_normal(n)
    if "gv0" in flags:
        gv = np.zeros(n)
    if "gm0" in flags:
        gm = np.zeros((n, DO))
    return dict(kind=kind, ard=bool(ard), white_var=wv, white=white, n=n, M=M, D=D, DO=DO, Z=Z, X=X, ls=ls, variance=VARIANCE,
                jitter=VARIANCE * M / 50.0, q_mu=q_mu, gm=gm, gv=gv, flags=flags)


def _args(c):
    return c["kind"], c["Z"], c["X"], c["q_mu"], c["variance"], c["ls"]


@functools.lru_cache(maxsize=None)
def forward(name, dtype=SR.LD):
    c = inputs(name)
    return SR.forward(*_args(c), c["white_var"], c["jitter"], c["white"], dtype=dtype)


@functools.lru_cache(maxsize=None)
def reverse(name, dtype=SR.LD):
    c = inputs(name)
    return SR.reverse(*_args(c), c["ard"], c["white_var"], c["jitter"], c["white"], c["gm"], c["gv"], dtype=dtype)
