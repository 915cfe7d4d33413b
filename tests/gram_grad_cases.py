"""The case table of the tests of the reverse pass of the Gram matrix (tests/test_gram_grad_reference_cpu.py,
tests/test_gram_grad_plan_cpu.py, tests/test_gpu_gram_grad.py).

The thresholds k_gg_pass of csrc/gram_grad.hip and its plan (csrc/gram_grad_plan.hpp) actually have, and the cases either side of each:
  * a workgroup owns GG_T = 128 rows:                              rb127, rb128, rb129 (symmetric), x129 (cross, both passes)
  * the column side is staged in tiles of GG_CT = 16 columns:       c15, c16, c17 / s15, s16, s17; several tiles in one split: c33, c50, s33, s50
  * a second column split from 65 columns on (GG_MIN_COLS = 64):   cs64 (one split), cs65 (two), cs129 (three, the last one ragged);
                                                                   x129 has two splits in pass a and three in pass b; rb127 .. rb129 two / three
  * the instance is chosen by D <= 4, 8, 16, 32:                    D = 1, 3, 4 | 5, 8 | 9, 16 | 17, 30, 32; `d33` is the first width refused
and what the kernel has to get right at any size: a White part (white_s, white_c), scalar and ARD lengthscales, a G that is not symmetric
(every symmetric case), rows of X2 equal to rows of X (dup_c), a duplicated row in the symmetric form (dup_s), a pair far enough apart for
the exponential to underflow (far_c, far_s), data at an offset of 1e6 (offset_*; n = 33, n2 = 17, D = 5).

Data: standard normal rows, lengthscales sqrt(D) uniform(0.5, 1.5) (so that the scaled squared distances stay of order one at every D),
variance 1.7, a White variance 0.3 where there is one, G standard normal; everything from default_rng(seed)."""
import functools

import numpy as np

from tests import gram_grad_reference as R

RBF, M52 = R.RBF, R.MATERN52
#             kind  sym   n   n2   D  ard white seed
CASES = {
    "c1":       (RBF, 0,   1,   1,  1, 0, 0, 1),
    "c15":      (M52, 0,  15,  17,  3, 1, 0, 2),
    "c16":      (RBF, 0,  16,  16,  3, 0, 0, 3),
    "c17":      (M52, 0,  17,  15,  8, 1, 0, 4),
    "c33":      (RBF, 0,  33,  50,  5, 1, 0, 5),
    "c50":      (M52, 0,  50,  33,  1, 0, 0, 6),
    "s1":       (M52, 1,   1,   0,  3, 1, 0, 7),
    "s15":      (RBF, 1,  15,   0,  3, 1, 0, 8),
    "s16":      (M52, 1,  16,   0,  8, 0, 0, 9),
    "s17":      (RBF, 1,  17,   0,  1, 0, 0, 10),
    "s33":      (M52, 1,  33,   0,  4, 1, 0, 11),
    "s50":      (RBF, 1,  50,   0,  9, 1, 0, 12),
    "rb127":    (M52, 1, 127,   0,  3, 1, 0, 13),
    "rb128":    (RBF, 1, 128,   0,  3, 0, 0, 14),
    "rb129":    (M52, 1, 129,   0,  3, 1, 0, 15),
    "cs64":     (RBF, 0,   5,  64,  3, 1, 0, 16),
    "cs65":     (M52, 0,   5,  65,  3, 1, 0, 17),
    "cs129":    (RBF, 0,  17, 129,  5, 0, 0, 18),
    "x129":     (M52, 0, 129,  65,  3, 1, 0, 19),
    "d16":      (RBF, 0,  17,  33, 16, 1, 0, 20),
    "d17":      (M52, 1,  33,   0, 17, 1, 0, 21),
    "d30":      (RBF, 0,  17,  33, 30, 1, 0, 22),
    "d30s":     (M52, 1,  33,   0, 30, 0, 0, 23),
    "d32":      (M52, 0,  33,  17, 32, 1, 0, 24),
    "d32s":     (RBF, 1,  33,   0, 32, 0, 0, 25),
    "white_s":  (M52, 1,  33,   0,  3, 1, 1, 26),
    "white_c":  (RBF, 0,  17,  33,  3, 0, 1, 27),
    "dup_c":    (M52, 0,  33,  17,  3, 1, 0, 28),
    "dup_s":    (RBF, 1,  33,   0,  3, 1, 0, 29),
    "far_c":    (M52, 0,  17,  33,  3, 1, 0, 30),
    "far_s":    (RBF, 1,  33,   0,  3, 1, 0, 31),
    "offset_c_rbf": (RBF, 0, 33, 17, 5, 1, 0, 32),
    "offset_c_m52": (M52, 0, 33, 17, 5, 1, 0, 32),
    "offset_s_rbf": (RBF, 1, 33,  0, 5, 0, 0, 33),
    "offset_s_m52": (M52, 1, 33,  0, 5, 0, 0, 33),
    "d33":      (RBF, 0,   5,   3, 33, 1, 0, 34),
}
UNSUPPORTED = "d33"
NAMES = tuple(n for n in CASES if n != UNSUPPORTED)
OFFSET = tuple(n for n in NAMES if n.startswith("offset"))
FAR = ("far_c", "far_s")
OFFSET_VALUE = 1e6
VARIANCE, WHITE_VARIANCE = 1.7, 0.3
KEYS = ("X", "X2", "variance", "lengthscales", "diag")


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(kind, sym, X, X2 (None in the symmetric form), G, variance, ls, ard, white (a variance or None)); shared: do not write to
    the arrays"""
    kind, sym, n, n2, D, ard, white, seed = CASES[name]
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D))
    X2 = None if sym else rng.standard_normal((n2, D))
    ls = np.sqrt(D) * rng.uniform(0.5, 1.5, D if ard else 1)
    G = rng.standard_normal((n, n if sym else n2))
    if name == "dup_c":
        X2[[0, 5, 16]] = X[[3, 3, 32]]
    if name == "dup_s":
        X[7] = X[20]
    if name == "far_c":
        X2[4, 1] += 1e4
    if name == "far_s":
        X[9, 2] -= 1e4
    if name in OFFSET:
        X = X + OFFSET_VALUE
        X2 = None if sym else X2 + OFFSET_VALUE
    for a in (X, X2, ls, G):
        if a is not None:
            a.setflags(write=False)
    return dict(kind=kind, sym=bool(sym), X=X, X2=X2, G=G, variance=VARIANCE, ls=ls, ard=bool(ard),
                white=WHITE_VARIANCE if white else None)


def args(c):
    return c["kind"], c["X"], c["X2"], c["G"], c["variance"], c["ls"], c["ard"]


@functools.lru_cache(maxsize=None)
def truth(name):
    """(grad, mag) in long double"""
    return R.gram_grad(*args(inputs(name)), dtype=R.LD)


@functools.lru_cache(maxsize=None)
def float64(name):
    return R.gram_grad(*args(inputs(name)), dtype=np.float64)[0]
