"""The case table of the kernel-expectation tests (tests/test_psi_reference_cpu.py, tests/test_gpu_psi.py).  Each case sits on one edge
the kernels of csrc/psi.hip can get wrong; the shapes are the smallest that reach it (k_psi2 tiles psi2 in 16 x 16, works on blocks of
16 rows, k-groups of 4 input dimensions in chunks of 32, and splits the rows from 64 rows per split on).

Recipe unless stated: rng = np.random.default_rng(seed); mu, Z standard normal, s uniform on [0, 0.8), variance 1.7, lengthscales
sqrt(D) x (uniform on [0.5, 1.5) per dimension with ARD, else 0.9)."""
import functools

import numpy as np

from tests import psi_reference as R

#            n    M   D  ARD seed recipe        edge
CASES = {
    "n1": (1, 2, 3, 1, 1, "plain"),             # a single row
    "n15": (15, 16, 4, 0, 2, "plain"),          # one short row block, a full tile, a full k-group
    "n16": (16, 17, 1, 0, 3, "plain"),          # a full row block; tile edge 16 | 17: an off-diagonal tile and its mirror; D = 1
    "n17": (17, 1, 5, 1, 4, "plain"),           # one past the row block; M = 1; D = 5: a ragged second k-group
    "n33": (33, 2, 3, 0, 5, "plain"),           # three row blocks; M = 2
    "m33": (20, 33, 2, 0, 7, "plain"),          # three tile rows: tile (2, 0) and its mirror
    "m50": (40, 50, 3, 1, 6, "plain"),          # ten tiles, a ragged last one
    "split": (130, 18, 3, 1, 8, "plain"),       # three row splits per tile, the last one ragged
    "split2": (200, 17, 5, 0, 9, "some_zero"),  # four row splits; s = 0 on every third row
    "d30": (24, 17, 30, 1, 10, "plain"),        # a ragged last k-group (30 = 7 x 4 + 2)
    "d65": (19, 18, 65, 1, 11, "plain"),        # three chunks of the delta^2 operand, the last one ragged
    "zero": (33, 17, 3, 1, 12, "zero"),         # s exactly 0 everywhere
    "null": (33, 17, 3, 1, 12, "null"),         # the same through s == NULL
    "tiny_s": (20, 5, 3, 0, 13, "tiny_s"),      # s = 1e-30
    "huge_s": (20, 5, 3, 1, 14, "huge_s"),      # s = 1e6
    "offset": (40, 17, 4, 1, 15, "offset"),     # mu and Z at an offset of 1e6
    "far": (18, 6, 2, 0, 16, "far"),            # z_0 sixty lengthscales away: its entries underflow to +0
    "negvar": (20, 5, 3, 1, 17, "negvar"),      # s[3, 1] = -0.75 l_1^2: l^2 + 2 s < 0 in row 3
    # the same in the LAST row, the one every masked row past the end is read from, with a ragged last row block and three splits
    "negvar_last": (130, 18, 3, 1, 18, "negvar_last"),
}
NAMES = tuple(CASES)
NEGVAR = ("negvar", "negvar_last")
FINITE = tuple(n for n in NAMES if n not in NEGVAR)
QUADRATURE = ("n16", "m33")                    # D <= 2; their s and l are rescaled into the rule's range by quadrature_inputs


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(mu, s (None for the NULL route), Z, variance, ls (scalar array or (D,)), ard); shared: do not write to the arrays"""
    n, M, D, ard, seed, recipe = CASES[name]
    rng = np.random.default_rng(seed)
    mu, Z = rng.standard_normal((n, D)), rng.standard_normal((M, D))
    s = rng.uniform(0.0, 0.8, (n, D))
    ls = np.sqrt(D) * (rng.uniform(0.5, 1.5, D) if ard else np.array([0.9]))
    if recipe == "some_zero":
        s[::3] = 0.0
    elif recipe in ("zero", "null"):
        s[:] = 0.0
    elif recipe == "tiny_s":
        s[:] = 1e-30
    elif recipe == "huge_s":
        s[:] = 1e6
    elif recipe == "offset":
        mu, Z = mu + 1e6, Z + 1e6
    elif recipe == "far":
        Z[0] = 60.0 * ls[0]
    elif recipe == "negvar":
        s[3, 1] = -0.75 * ls[1] ** 2
    elif recipe == "negvar_last":
        s[n - 1, 1] = -0.75 * ls[1] ** 2
    for a in (mu, Z, s, ls):
        a.setflags(write=False)
    return dict(mu=mu, s=None if recipe == "null" else s, Z=Z, variance=1.7, ls=ls, ard=bool(ard))


def _args(c):
    return c["mu"], c["s"], c["Z"], c["variance"], c["ls"]


@functools.lru_cache(maxsize=None)
def truth(name):
    """dict(psi0, psi1, psi2: long double; absE (M, M): max_n of the sum of the magnitudes of the terms of the psi2 exponent)"""
    p0, p1, p2, absE = R.psi(*_args(inputs(name)), dtype=R.LD, want_abs=True)
    return dict(psi0=p0, psi1=p1, psi2=p2, absE=absE)


@functools.lru_cache(maxsize=None)
def float64(name):
    p0, p1, p2 = R.psi(*_args(inputs(name)), dtype=np.float64)
    return dict(psi0=p0, psi1=p1, psi2=p2)


@functools.lru_cache(maxsize=None)
def quadrature_inputs(name):
    """the case with s scaled into [0, 0.3) and the lengthscales raised to >= 0.5: the range in which the H = 100 rule is exact"""
    c = dict(inputs(name))
    c["s"] = c["s"] * (0.3 / 0.8)
    c["ls"] = np.maximum(c["ls"], 0.5)
    return c
