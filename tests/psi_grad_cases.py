"""The case table of the tests of the reverse pass of the kernel expectations (tests/test_psi_grad_reference_cpu.py,
tests/test_gpu_psi_grad.py).  The inputs are those of tests/psi_cases.py wherever a case of it sits on the edge (k_psi2_grad of
csrc/psi_grad.hip tiles the inducing inputs in 16, works on blocks of 16 rows, takes the input dimensions in k-groups of 4 and in one or
two blocks of 16, and splits the rows from 64 rows per split on); `d32` and `d33` are the widest input the kernel takes and the first it
refuses.  The adjoints: g_psi0 = -0.7, g_psi1 (n, M) and g_psi2 (M, M, not symmetric) standard normal from default_rng(1000 + seed)."""
import functools

import numpy as np

from tests import psi_cases as PC
from tests import psi_grad_reference as R

G_PSI0 = -0.7
#  from tests/psi_cases.py:
#   n1, n15, n16, n17          the row-block edges; M = 1 (n17); D = 1 (n16); n15, n16 without ARD: one lengthscale entry
#   m33, m50                   three and four tile rows, a ragged last tile
#   split, split2              three and four row splits, the last one ragged (split2 without ARD)
#   d30                        a ragged k-group, two blocks of 16 dimensions
#   zero / null, tiny_s, huge_s, offset, far, negvar, negvar_last
SHARED = ("n1", "n15", "n16", "n17", "m33", "m50", "split", "split2", "d30", "zero", "null", "tiny_s", "huge_s", "offset", "far", "negvar",
          "negvar_last")
#            n   M   D  ARD seed
OWN = {
    "d32": (24, 17, 32, 1, 21),                 # the widest input: two full blocks of 16 dimensions
    "d33": (5, 3, 33, 1, 22),                   # one past it: refused
}
NAMES = SHARED + ("d32",)
UNSUPPORTED = "d33"
NEGVAR = ("negvar", "negvar_last")
FINITE = tuple(n for n in NAMES if n not in NEGVAR)
NEGVAR_ROW = {"negvar": 3, "negvar_last": 129}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(mu, s (None for the NULL route), Z, variance, ls, ard, g0, g1, g2); shared: do not write to the arrays"""
    if name in OWN:
        n, M, D, ard, seed = OWN[name]
        rng = np.random.default_rng(seed)
        mu, Z = rng.standard_normal((n, D)), rng.standard_normal((M, D))
        s = rng.uniform(0.0, 0.8, (n, D))
        ls = np.sqrt(D) * rng.uniform(0.5, 1.5, D)
        for a in (mu, Z, s, ls):
            a.setflags(write=False)
        c = dict(mu=mu, s=s, Z=Z, variance=1.7, ls=ls, ard=bool(ard))
    else:
        c = dict(PC.inputs(name))
        seed = PC.CASES[name][4]
    rng = np.random.default_rng(1000 + seed)
    n, M = c["mu"].shape[0], c["Z"].shape[0]
    g1, g2 = rng.standard_normal((n, M)), rng.standard_normal((M, M))
    g1.setflags(write=False)
    g2.setflags(write=False)
    c.update(g0=G_PSI0, g1=g1, g2=g2)
    return c


def args(c):
    return c["mu"], c["s"], c["Z"], c["variance"], c["ls"], c["ard"], c["g0"], c["g1"], c["g2"]


@functools.lru_cache(maxsize=None)
def truth(name):
    """(grad, mag) in long double"""
    return R.psi_grad(*args(inputs(name)), dtype=R.LD)


@functools.lru_cache(maxsize=None)
def float64(name):
    return R.psi_grad(*args(inputs(name)), dtype=np.float64)[0]
