"""CPU side of tests/test_gpu_trsm_direct.py: triangular solves on the factors real inducing sets produce.  No GPU, no product code:
tests/test_trsm_reference_cpu.py holds the CPU reference and a float64 restatement of the kernel's algorithm to every device bar.

Matrices.  L = numpy.linalg.cholesky(Ku), Ku = factor_reference.reference_ku(Z, spec, jitter), Z from factor_reference.family_case
(`spread`, `pairs`, `grid1d`) or from the two families added here: `dups` (the second half of Z is an exact copy of the first) and
`subset1d` (sorted uniform draws on [-2.5, 2.5], lengthscale 0.7).  Jitter 1e-6; `pairs` also at 1e-9.  cond(Ku) reaches 1e8 .. 1e9
and the 16 x 16 diagonal blocks of L reach |D^-1||D| of several thousand.  The float64 L is the input of every solver; the truth is
the substitution on that same L in numpy.longdouble (64-bit mantissa: 2000 x finer than any error compared with it).

Measures (op(L) = L or L^T, products through factor_reference.xprod in longdouble):
  rho   max_ij |op(L) X - B|_ij / (|op(L)||X|)_ij   in units of 2^-53: the componentwise backward error (an entry whose scale is zero
        must have a zero residual)
  norm  |op(L) X - B|_F / (n |L|_F |X|_F)           the normwise residual of test_gpu_round2.py::test_trsm_large (its bar: 1e-13)
  fe    max|X - X_true| / max|X_true|
Bars of a device result (DEVICE_FACTOR = 8, the project's margin for another summation order):
  rho_dev <= 8 max(rho_cpu(case), rho_table)        rho_table = the largest rho_cpu over the whole case table, computed, not typed in
  fe_dev  <= 8 max(fe_cpu(case), 2^-52)             both solvers' forward errors scale with the same cond(L)
`cpu` is scipy.linalg.solve_triangular (LAPACK dtrtrs: plain substitution).

What the bars found: 16 x 16 diagonal blocks applied as their explicit inverses and nothing else (blocked_emulation(refine=0), the
kernel as it stood) leave rho at |D^-1||D| roundings — 182 on the factor of a 15-point 1-D grid, 3e3 on B = L[:, :20] — and a forward
error 50 x substitution's on that B.  One refinement step per block (refine=1, the kernel now) brings rho to 1 - 2 x scipy's on every
case.  Before / after on an MI355X: profiles/trsm_refinement_ab.md."""
import numpy as np

from tests import factor_reference as R

LD = np.longdouble
U = 2.0 ** -53
DEVICE_FACTOR = R.DEVICE_FACTOR
FAMILIES = R.FAMILIES + ("dups", "subset1d")
PANEL, BLOCK = 128, 16


def family_case(family, n, seed=0):
    """-> (Z, kernel spec); factor_reference.family_case for its three families"""
    if family in R.FAMILIES:
        return R.family_case(family, n, "rbf", seed)
    rng = np.random.RandomState(1000 * seed + n + 7)
    if family == "dups":
        h = n // 2
        base = rng.randn(n - h, 2)
        Z, ls = np.concatenate([base, base[:h]]), 1.0
    elif family == "subset1d":
        Z, ls = np.sort(rng.uniform(-2.5, 2.5, n))[:, None].copy(), 0.7
    else:
        raise ValueError(family)
    return Z, dict(kind="rbf", input_dim=Z.shape[1], variance=1.0, lengthscales=ls, ARD=False, white_variance=None)


_FACTORS = {}


def factor(family, n, jitter=1e-6):
    """(L, cond(L)) — cached, read-only"""
    key = (family, n, jitter)
    if key not in _FACTORS:
        Z, spec = family_case(family, n)
        L = np.linalg.cholesky(R.reference_ku(Z, spec, jitter))
        L.setflags(write=False)
        _FACTORS[key] = (L, float(np.linalg.cond(L)))
    return _FACTORS[key]


# ------------------------------------------------------------------------------------------------ solvers
def solve_truth(L, B, trans):
    """op(L)^-1 B by substitution in longdouble"""
    Lx = np.asarray(L, dtype=LD)
    X = np.array(B, dtype=LD)
    n = L.shape[0]
    if not trans:
        for i in range(n):
            X[i] = (X[i] - Lx[i, :i] @ X[:i]) / Lx[i, i]
    else:
        for i in range(n - 1, -1, -1):
            X[i] = (X[i] - Lx[i + 1:, i] @ X[i + 1:]) / Lx[i, i]
    return X


def solve_cpu(L, B, trans):
    import scipy.linalg as sla
    return sla.solve_triangular(L, B, lower=True, trans=trans)


def blocked_emulation(L, B, trans, refine=1):
    """the algorithm of csrc/trsm.hip in float64 numpy: every 16 x 16 diagonal block inverted explicitly (forward substitution on the
    identity, a column at a time), then X_i = D_i^-1 acc, acc = B_i - sum_k op(L)_ik X_k, as block products, followed by `refine` steps
    X_i += D_i^-1 (acc - op(D_i) X_i) against the block itself; trans walks the blocks upwards with the transposed blocks and D_i^-T.
    refine = 0 is the kernel as it stood before it was held to these bars."""
    n = L.shape[0]
    nb = -(-n // BLOCK)
    Dinv = []
    for b in range(nb):
        r0, r1 = b * BLOCK, min(n, (b + 1) * BLOCK)
        D = L[r0:r1, r0:r1]
        m = r1 - r0
        Xd = np.zeros((m, m))
        acc = np.eye(m)
        for k in range(m):
            Xd[k] = acc[k] / D[k, k]
            acc[k + 1:] -= np.outer(D[k + 1:, k], Xd[k])
        Dinv.append(Xd)
    X = np.array(B, dtype=np.float64)
    order = range(nb - 1, -1, -1) if trans else range(nb)
    for b in order:
        r0, r1 = b * BLOCK, min(n, (b + 1) * BLOCK)
        D = np.tril(L[r0:r1, r0:r1])
        if not trans:
            acc, Di, Do = X[r0:r1] - L[r0:r1, :r0] @ X[:r0], Dinv[b], D
        else:
            acc, Di, Do = X[r0:r1] - L[r1:, r0:r1].T @ X[r1:], Dinv[b].T, D.T
        x = Di @ acc
        for _ in range(refine):
            x = x + Di @ (acc - Do @ x)
        X[r0:r1] = x
    return X


# ------------------------------------------------------------------------------------------------ measures
def measures(L, X, B, trans, X_true):
    """dict(rho, norm, fe) of a float64 solution X of op(L) X = B; L lower-triangular (only that triangle is used)"""
    Ll = np.tril(np.asarray(L, dtype=np.float64))
    X = np.asarray(X, dtype=np.float64)
    n = Ll.shape[0]
    P = R.xprod(Ll.T, X) if trans else R.xprod(Ll, X, a_lower=True)
    Res = np.abs(P - np.asarray(B, dtype=LD)).astype(np.float64)
    aL = np.abs(Ll)
    scale = (aL.T if trans else aL) @ np.abs(X)
    if np.any(Res[scale == 0.0] != 0.0):
        rho = float("inf")
    else:
        rho = float(np.max(Res / np.where(scale == 0.0, 1.0, scale))) / U
    nx = np.linalg.norm(X)
    norm = float(np.linalg.norm(Res)) / (n * np.linalg.norm(Ll) * nx) if nx > 0 else 0.0
    fe = float(np.max(np.abs(X.astype(LD) - X_true)) / np.max(np.abs(X_true)))
    return dict(rho=rho, norm=norm, fe=fe)


def float64_rho(L, X, B, trans):
    """rho with the product in float64 — for the thousands of columns of the left-looking cases.  The rounding of the product itself is
    at most n 2^-53 |op(L)||X| entrywise (Higham, Accuracy and Stability, 3.5): float64_slack(n) units are added to the bar."""
    Ll = np.tril(np.asarray(L, dtype=np.float64))
    Lo = Ll.T if trans else Ll
    Res = np.abs(Lo @ X - B)
    scale = np.abs(Lo) @ np.abs(X)
    assert not np.any(Res[scale == 0.0] != 0.0)
    return float(np.max(Res / np.where(scale == 0.0, 1.0, scale))) / U


def float64_slack(n):
    return float(n)


# ------------------------------------------------------------------------------------------------ the case table
class Case:
    """one single solve: a factor (family, n, jitter), a right-hand side (kind, nrhs, seed) and, for the left-looking shapes, the
    columns the longdouble measures are taken on"""

    def __init__(self, group, family, n, nrhs, jitter=1e-6, rhs="randn", sample=None, seed=0):
        self.group, self.family, self.n, self.nrhs, self.jitter, self.rhs, self.sample, self.seed = group, family, n, nrhs, jitter, rhs, sample, seed
        self.name = f"{group}-{family}" + ("" if jitter == 1e-6 else f"-j{jitter:g}") + f"-n{n}-r{nrhs}" + ("" if rhs == "randn" else f"-{rhs}") + \
            (f"-s{seed}" if group in ("batched", "shared") else "")

        # lrows: B = L^T[:, :k], the transposed twin of the issue's B = L[:, :k], also has X = [I; 0] — and substitution reproduces it
        # EXACTLY (every L_ij - L_ij 1 cancels, the next row starts from a true 0 or 1), so fe_cpu is 1.6e-16 where a backward-stable
        # solve owes cond(L) 2^-53 = 1e-12.  The blocks of the device kernel return 1 +- 2^-53 and 1e-17 for those 1 and 0, the next
        # block amplifies that by |D^-1|: 1.0e-14 on subset1d (the float64 emulation: 9.1e-15).  Held to rho like every case; fe recorded.
        self.fe_held = rhs != "lrows"

    def L(self):
        return factor(self.family, self.n, self.jitter)[0]

    def cond(self):
        return factor(self.family, self.n, self.jitter)[1]

    def B(self, trans):
        """randn: the same for both values of trans.  lcols: the first nrhs columns of L; at trans = 0 the solution is [I; 0].  lrows: the
        first nrhs columns of L^T; at trans = 1 the solution is [I; 0].  pow2: randn
        columns scaled by 2^-30 .. 2^30 (one exponent per column).  zerocol: randn with column 1 all zero"""
        rng = np.random.RandomState(977 * self.seed + 31 * self.n + self.nrhs)
        if self.rhs in ("lcols", "lrows"):
            L = self.L()
            return np.ascontiguousarray((L.T if self.rhs == "lrows" else L)[:, :self.nrhs])
        B = rng.randn(self.n, self.nrhs)
        if self.rhs == "pow2":
            B = B * pow2_scales(self.nrhs)[None, :]
        elif self.rhs == "zerocol":
            B[:, min(1, self.nrhs - 1)] = 0.0
        return B

    def columns(self):
        """the columns of the longdouble measures: all, or a seeded sample of `sample` of the first `sample_from` columns"""
        if self.sample is None:
            return np.arange(self.nrhs)
        count, among = self.sample
        return np.sort(np.random.RandomState(self.n + among).choice(among, count, replace=False))


def pow2_scales(nrhs):
    return 2.0 ** np.round(np.linspace(-30, 30, nrhs))


N_EDGES = (1, 15, 16, 17, 127, 128, 129, 257, 330)       # the 16-row block, the 128-row panel, two panels and a ragged third
NRHS_EDGES = (1, 15, 17, 64, 65, 130)                    # one wave's 16 columns, one workgroup's 64, the clamped column
LEFT_SAMPLE = (64, 2052)                                 # 64 columns among those the (386, 2052) twin shares


def _table():
    cases = []
    for family in ("pairs", "grid1d"):                   # every n with two nrhs, every nrhs with three n
        for i, n in enumerate(N_EDGES):
            for nrhs in (NRHS_EDGES[i % 6], NRHS_EDGES[(i + 3) % 6]):
                cases.append(Case("edge", family, n, nrhs))
    for family, jitter in [(f, 1e-6) for f in FAMILIES] + [("pairs", 1e-9)]:
        cases.append(Case("family", family, 200, 40, jitter))
    for family in ("pairs", "subset1d"):
        cases.append(Case("left", family, 256, 2048, sample=LEFT_SAMPLE))
        cases.append(Case("left", family, 386, 2056, sample=LEFT_SAMPLE))
        cases.append(Case("twin", family, 386, 2052, sample=LEFT_SAMPLE))
    for family, n, nrhs in [("pairs", 129, 65), ("grid1d", 330, 17), ("dups", 17, 1)]:
        cases.append(Case("layout", family, n, nrhs, seed=1))
    for b, (family, jitter) in enumerate([("spread", 1e-6), ("dups", 1e-6), ("pairs", 1e-9)]):
        cases.append(Case("batched", family, 130, 17, jitter, seed=10 + b))
    for b in range(3):
        cases.append(Case("shared", "subset1d", 130, 17, seed=20 + b))
    for family in ("pairs", "subset1d"):
        cases.append(Case("exact", family, 129, 61, rhs="pow2", seed=2))
        cases.append(Case("exact", family, 129, 61, rhs="randn", seed=2))
        cases.append(Case("exact", family, 129, 20, rhs="zerocol", seed=3))
        cases.append(Case("exact", family, 150, 20, rhs="lcols"))
        cases.append(Case("exact", family, 150, 20, rhs="lrows"))
    return cases


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
_CPU = {}


def twin_rhs(case, trans):
    """the (386, 2052) twin solves the first 2052 columns of the (386, 2056) case's right-hand side"""
    return np.ascontiguousarray(BY_NAME[case.name.replace("twin", "left").replace("r2052", "r2056")].B(trans)[:, :case.nrhs])


def rhs(case, trans):
    return twin_rhs(case, trans) if case.group == "twin" else case.B(trans)


def cpu_reference(case, trans):
    """dict: B, cols, X_true (on cols), X_cpu, and the CPU solve's measures rho / norm / fe (on cols) — cached"""
    key = (case.name, trans)
    if key not in _CPU:
        L, B, cols = case.L(), rhs(case, trans), case.columns()
        B.setflags(write=False)
        X_true = solve_truth(L, B[:, cols], trans)
        X_cpu = solve_cpu(L, B, trans)
        out = dict(B=B, cols=cols, X_true=X_true, X_cpu=X_cpu)
        out.update(measures(L, X_cpu[:, cols], B[:, cols], trans, X_true))
        _CPU[key] = out
    return _CPU[key]


_RHO_TABLE = []


def rho_table():
    """the largest rho of the CPU solve over the whole table, both values of trans"""
    if not _RHO_TABLE:
        _RHO_TABLE.append(max(cpu_reference(c, t)["rho"] for c in CASES for t in (0, 1)))
    return _RHO_TABLE[0]


def bars(case, trans):
    ref = cpu_reference(case, trans)
    return DEVICE_FACTOR * max(ref["rho"], rho_table()), DEVICE_FACTOR * max(ref["fe"], 2.0 ** -52)


def check(case, trans, X, what="device", record=None):
    """measures of the float64 solution X (all columns of the case) + the two bars; asserts both (after handing the figures to `record`).
    -> dict for the profile"""
    ref = cpu_reference(case, trans)
    cols = ref["cols"]
    m = measures(case.L(), X[:, cols], ref["B"][:, cols], trans, ref["X_true"])
    rho_bar, fe_bar = bars(case, trans)
    row = dict(case=case.name, trans=trans, cond=case.cond(), rho=m["rho"], rho_cpu=ref["rho"], fe=m["fe"], fe_cpu=ref["fe"],
               norm=m["norm"], norm_cpu=ref["norm"], rho_bar=rho_bar, fe_bar=fe_bar)
    print("%s trans=%d %s: cond(L) %.3g  rho %.3g (cpu %.3g, bar %.3g)  fe %.3g (cpu %.3g, bar %.3g)  normwise %.3g (cpu %.3g)" %
          (case.name, trans, what, row["cond"], m["rho"], ref["rho"], rho_bar, m["fe"], ref["fe"], fe_bar, m["norm"], ref["norm"]))
    if record is not None:
        record(row)
    assert np.all(np.isfinite(X)), case.name
    assert m["rho"] <= rho_bar, (case.name, trans, what, "rho", m["rho"], rho_bar)
    assert m["fe"] <= fe_bar or not case.fe_held, (case.name, trans, what, "fe", m["fe"], fe_bar)
    assert m["norm"] <= 1e-13, (case.name, trans, what, "normwise", m["norm"])
    return row
