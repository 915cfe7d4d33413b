"""The yardstick of the collapsed-layer tests (tests/test_psi_reference_cpu.py, tests/test_gpu_collapsed.py): the bound and the
prediction of the reference's gplvm_build_likelihood / gplvm_build_predict, psi branch (layers.py:405-450, 483-525), operation by
operation, from the kernel expectations of tests/psi_reference.py.  dtype=np.longdouble is the truth, dtype=np.float64 the same
operation sequence in float64 (numpy has no long-double LAPACK, so the factorisation and the triangular solves are written out and
serve both).  Also the dense textbook forms the reference's own tests compare with (tests/test_collapsed.py:30-54): the exact GP
marginal likelihood and predictive, and Titsias' bound with Qff formed densely."""
import math

import numpy as np

from tests import psi_reference as P

LD = np.longdouble


def chol(A):
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_lower(L, B):
    X = np.array(B, dtype=L.dtype)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def rbf(X, X2, variance, ls, dtype):
    T = dtype
    X, X2 = np.asarray(X, dtype=T), np.asarray(X2, dtype=T)
    l = np.asarray(P.lengthscales(ls, X.shape[1]), dtype=T)
    d = (X[:, None, :] - X2[None, :, :]) / l
    return T(variance) * np.exp(T(-0.5) * np.sum(d * d, axis=2))


def collapsed_from(Kuu, psi0, psi1, psi2, Y, noise_var, dtype=LD, lapack=False):
    """the chain of collapsed() from given statistics (Kuu includes the jitter): dict with bound, terms (6, in the order of
    dsdgp_collapsed_bound), L, G = L^-1 psi2 L^-T, LB, c.  lapack (float64 only): numpy.linalg.cholesky and
    scipy.linalg.solve_triangular in place of the written-out loops — another order of the same operations."""
    T = dtype
    Kuu, psi1, psi2, Y = (np.asarray(a, dtype=T) for a in (Kuu, psi1, psi2, Y))
    psi0 = T(psi0)
    if lapack:
        import scipy.linalg as sla
        assert T is np.float64
        fac, sol = np.linalg.cholesky, lambda L, B: sla.solve_triangular(L, B, lower=True)
    else:
        fac, sol = chol, solve_lower
    N, DY = Y.shape
    M = Kuu.shape[0]
    s2 = T(noise_var)
    sigma = np.sqrt(s2)
    L = fac(Kuu)
    A = sol(L, psi1.T) / sigma
    tmp = sol(L, psi2)
    G = sol(L, tmp.T)
    AAT = G / s2
    LB = fac(AAT + np.eye(M, dtype=T))
    c = sol(LB, A @ Y) / sigma
    two_pi = T(2) * (np.pi if T is np.float64 else LD("3.14159265358979323846264338327950288"))
    terms = np.array([T(-0.5) * T(N * DY) * np.log(two_pi * s2), -T(DY) * np.sum(np.log(np.diag(LB))), T(-0.5) * np.sum(Y * Y) / s2,
                      T(0.5) * np.sum(c * c), T(-0.5) * T(DY) * psi0 / s2, T(0.5) * T(DY) * np.trace(AAT)], dtype=T)
    return dict(bound=np.sum(terms), terms=terms, L=L, G=G, LB=LB, c=c, DY=DY, dtype=T, lapack=lapack)


def collapsed(mu, s, Z, variance, ls, Y, noise_var, jitter, dtype=LD):
    """dict: bound, terms (6, in the order of dsdgp_collapsed_bound), L, LB, c and the inputs the prediction needs"""
    T = dtype
    psi0, psi1, psi2 = P.psi(mu, s, Z, variance, ls, dtype=T)
    M = np.asarray(Z).shape[0]
    Kuu = rbf(Z, Z, variance, ls, T) + T(jitter) * np.eye(M, dtype=T)
    out = collapsed_from(Kuu, psi0, psi1, psi2, Y, noise_var, dtype=T)
    out.update(Z=np.asarray(Z, dtype=T), variance=variance, ls=ls)
    return out


def predict(state, Xs, full_cov=False, Kus=None):
    """(mean (N*, DY), var (N*, DY) or (N*, N*, DY)) of layers.py:512-525.  Kus: K(Z, X*) given (a state of collapsed_from holds no Z)"""
    T = state["dtype"]
    Kus = rbf(state["Z"], Xs, state["variance"], state["ls"], T) if Kus is None else np.asarray(Kus, dtype=T)
    if state.get("lapack"):
        import scipy.linalg as sla
        sol = lambda L, B: sla.solve_triangular(L, B, lower=True)
    else:
        sol = solve_lower
    tmp1 = sol(state["L"], Kus)
    tmp2 = sol(state["LB"], tmp1)
    mean = tmp2.T @ state["c"]
    if full_cov:
        var = rbf(Xs, Xs, state["variance"], state["ls"], T) + tmp2.T @ tmp2 - tmp1.T @ tmp1
        return mean, np.tile(var[:, :, None], [1, 1, state["DY"]])
    var = T(state["variance"]) + np.sum(tmp2 * tmp2, axis=0) - np.sum(tmp1 * tmp1, axis=0)
    return mean, np.tile(var[:, None], [1, state["DY"]])


# ---------------------------------------------------------------------------------------------------------------- dense textbook forms
def exact_gp(X, Y, variance, ls, noise_var, Xs):
    """(log marginal likelihood, predictive mean (N*, DY), predictive covariance (N*, N*)) of exact GP regression, float64 LAPACK"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    N, DY = Y.shape
    K = rbf(X, X, variance, ls, np.float64) + noise_var * np.eye(N)
    Lk = np.linalg.cholesky(K)
    V = np.linalg.solve(Lk, Y)
    lml = -0.5 * np.sum(V * V) - DY * np.sum(np.log(np.diag(Lk))) - 0.5 * N * DY * math.log(2.0 * math.pi)
    Ks = rbf(X, Xs, variance, ls, np.float64)
    A = np.linalg.solve(Lk, Ks)
    return lml, A.T @ V, rbf(Xs, Xs, variance, ls, np.float64) - A.T @ A


def titsias_dense(X, Y, Z, variance, ls, noise_var, jitter):
    """the bound of tests/test_gpu_parity.py::test_natgrad_gamma1_gives_collapsed_bound for any D_Y: deterministic inputs, Qff dense"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    N, DY = Y.shape
    M = np.asarray(Z).shape[0]
    Kuu = rbf(Z, Z, variance, ls, np.float64) + jitter * np.eye(M)
    Kuf = rbf(Z, X, variance, ls, np.float64)
    Qff = Kuf.T @ np.linalg.solve(Kuu, Kuf)
    Cm = Qff + noise_var * np.eye(N)
    _, ld = np.linalg.slogdet(Cm)
    return (-0.5 * np.sum(Y * np.linalg.solve(Cm, Y)) - 0.5 * DY * ld - 0.5 * N * DY * math.log(2.0 * math.pi)
            - 0.5 * DY / noise_var * (N * variance - np.trace(Qff)))


# ---------------------------------------------------------------------------------------------------------------- the cases
#            N    M   D  DY  s>0  ls    noise seed
CASES = {
    "tiny": (7, 1, 1, 1, True, 0.8, 0.1, 1),
    "n40": (40, 9, 1, 1, False, 0.7, 0.2, 2),
    "dy3": (33, 17, 3, 3, True, 1.1, 0.3, 3),
    "m50": (100, 50, 2, 1, False, 0.6, 0.05, 4),
    "m130": (300, 130, 4, 3, True, 0.9, 0.1, 5),
}
NAMES = tuple(CASES)
JITTER = 1e-6
_CACHE = {}


def spaced_points(rng, M, D, gap, half_width=2.5):
    """M points uniform on [-half_width, half_width]^D, drawn one after another, a draw closer than `gap` to an accepted point refused"""
    pts = np.zeros((0, D))
    for _ in range(200000):
        x = rng.uniform(-half_width, half_width, (1, D))
        if pts.shape[0] == 0 or np.min(np.sum((pts - x) ** 2, axis=1)) >= gap * gap:
            pts = np.concatenate([pts, x])
            if pts.shape[0] == M:
                return pts
    raise RuntimeError("spaced_points: the box is full")


def inputs(name):
    """dict(mu, s or None, Z, variance, ls, Y, noise, Xs); shared: do not write to the arrays.  The inducing inputs keep a distance of
    at least l / 2 from one another — the spacing of the grids in the identity tests of tests/test_gpu_collapsed.py: two inducing
    inputs a small fraction of a lengthscale apart make Kuu + jitter I so ill-conditioned that the bound of ANY float64 evaluation
    depends on the order of its operations (LAPACK's factor in place of the written-out one moves it by 35 x e64 at a pair l / 10
    apart), and e64 would then measure the luck of one order rather than the rounding level.  The inducing sets that do sit that close
    — twins 1e-4 apart, data points as inducing inputs, a fine grid; cond(Kuu + jitter I) of 1e7 .. 1e8 — are ILL_CASES / ill_inputs
    below: there the yardstick is a FAMILY of float64 orders fed the device's own statistics, and every stage of the chain is held by
    its own order-independent residual (tests/test_gpu_collapsed_illcond.py, tests/test_collapsed_illcond_cpu.py)."""
    if name not in _CACHE:
        N, M, D, DY, noisy, ls, noise, seed = CASES[name]
        rng = np.random.default_rng(seed)
        mu = rng.standard_normal((N, D))
        s = rng.uniform(0.0, 0.3, (N, D)) if noisy else None
        Z = spaced_points(rng, M, D, 0.5 * ls)
        Y = np.sin(mu @ rng.standard_normal((D, DY))) + 0.2 * rng.standard_normal((N, DY))
        Xs = rng.standard_normal((11, D))
        for a in (mu, Z, Y, Xs) + (() if s is None else (s,)):
            a.setflags(write=False)
        _CACHE[name] = dict(mu=mu, s=s, Z=Z, variance=1.3, ls=np.array([ls]), Y=Y, noise=noise, Xs=Xs)
    return _CACHE[name]


def state(name, dtype):
    key = (name, dtype)
    if key not in _CACHE:
        c = inputs(name)
        _CACHE[key] = collapsed(c["mu"], c["s"], c["Z"], c["variance"], c["ls"], c["Y"], c["noise"], JITTER, dtype=dtype)
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------- ill-conditioned Kuu
#               N    M   D  DY  s>0  ls   noise seed
ILL_CASES = {
    "pairs": (120, 48, 2, 2, True, 1.0, 0.1, 11),       # twins 1e-4 apart, M / 2 rows from one another
    "subset": (200, 130, 2, 1, True, 1.0, 0.1, 12),     # Z = mu[:M]: the inducing inputs are data points; M crosses the 128-row panel
    "grid1d": (150, 64, 1, 1, False, 0.7, 0.1, 13),     # a grid on [-2.5, 2.5]: spacing 0.08 = l / 9
}
ILL_NAMES = tuple(ILL_CASES)
FAMILY, FAMILY_MAX = 6, 16           # written-out order, LAPACK, four seeded permutations of the inducing inputs; extended to at most 16
U = 2.0 ** -53


def ill_inputs(name):
    """as inputs(), for the cases whose Kuu + jitter I has a condition number of 1e7 .. 1e8"""
    key = ("ill", name)
    if key not in _CACHE:
        N, M, D, DY, noisy, ls, noise, seed = ILL_CASES[name]
        rng = np.random.default_rng(seed)
        mu = rng.standard_normal((N, D))
        s = rng.uniform(0.0, 0.3, (N, D)) if noisy else None
        if name == "pairs":
            base = rng.standard_normal((M // 2, D))
            Z = np.concatenate([base, base + 1e-4 * rng.standard_normal((M // 2, D))])
        elif name == "subset":
            Z = mu[:M].copy()
        else:
            Z = np.linspace(-2.5, 2.5, M)[:, None].copy()
        Y = np.sin(mu @ rng.standard_normal((D, DY))) + 0.2 * rng.standard_normal((N, DY))
        Xs = rng.standard_normal((11, D))
        for a in (mu, Z, Y, Xs) + (() if s is None else (s,)):
            a.setflags(write=False)
        _CACHE[key] = dict(mu=mu, s=s, Z=Z, variance=1.3, ls=np.array([ls]), Y=Y, noise=noise, Xs=Xs)
    return _CACHE[key]


def float64_statistics(c):
    """dict(Kuu, psi0, psi1, psi2, Kus) of a case from the float64 reference formulas — what the CPU tests feed the chain in place of the
    device's own statistics"""
    psi0, psi1, psi2 = P.psi(c["mu"], c["s"], c["Z"], c["variance"], c["ls"], dtype=np.float64)
    M = c["Z"].shape[0]
    Kuu = rbf(c["Z"], c["Z"], c["variance"], c["ls"], np.float64) + JITTER * np.eye(M)
    return dict(Kuu=Kuu, psi0=float(psi0), psi1=psi1, psi2=psi2, Kus=rbf(c["Z"], c["Xs"], c["variance"], c["ls"], np.float64))


def evaluate(c, st, dtype=LD, lapack=False, perm=None):
    """bound and prediction of the chain fed the statistics st (dict of float64_statistics' keys), the inducing inputs taken in the order
    `perm`: dict(bound, terms, mean, var (N*, DY), cov (N*, N*, DY), state)"""
    M = st["Kuu"].shape[0]
    p = np.arange(M) if perm is None else perm
    state = collapsed_from(st["Kuu"][np.ix_(p, p)], st["psi0"], st["psi1"][:, p], st["psi2"][np.ix_(p, p)], c["Y"], c["noise"], dtype, lapack)
    state.update(variance=c["variance"], ls=c["ls"])
    mean, var = predict(state, c["Xs"], False, Kus=st["Kus"][p])
    mean2, cov = predict(state, c["Xs"], True, Kus=st["Kus"][p])
    assert np.array_equal(mean, mean2)
    return dict(bound=state["bound"], terms=state["terms"], mean=mean, var=var, cov=cov, state=state)


def family_member(c, st, k):
    """member k of the family of float64 evaluations: 0 the written-out order, 1 LAPACK, k >= 2 the written-out order on a seeded
    permutation of the inducing inputs"""
    if k < 2:
        return evaluate(c, st, np.float64, lapack=(k == 1))
    M = st["Kuu"].shape[0]
    return evaluate(c, st, np.float64, perm=np.random.default_rng(1000 + k).permutation(M))


def errors(got, truth, c):
    """(bound in units of sum |terms|, mean in max |Y|, var in the kernel variance, cov likewise) of an evaluation against the truth"""
    unit = float(np.sum(np.abs(truth["terms"])))
    ymax, v = float(np.max(np.abs(c["Y"]))), c["variance"]
    return (abs(float(got["bound"] - truth["bound"])) / unit, float(np.max(np.abs(got["mean"] - truth["mean"]))) / ymax,
            float(np.max(np.abs(got["var"] - truth["var"]))) / v, float(np.max(np.abs(got["cov"] - truth["cov"]))) / v)


def family_errors(c, st, truth, members=FAMILY):
    """array (members, 4) of errors() over the family"""
    return np.array([errors(family_member(c, st, k), truth, c) for k in range(members)])


def _ratio(Res, scale):
    Res, scale = np.abs(Res).astype(np.float64), np.asarray(scale, dtype=np.float64)
    if np.any(Res[scale == 0.0] != 0.0):
        return float("inf")
    return float(np.max(Res / np.where(scale == 0.0, 1.0, scale))) / U


STAGES = ("L L^T - Kuu", "L G L^T - psi2", "LB LB^T - (G / s2 + I)", "L LB c - psi1^T Y / s2")
PREDICT_STAGES = ("L tmp1 - K(Z, X*)", "LB tmp2 - tmp1")


def stage_residuals(st, Y, noise_var, L, G, LB, c):
    """the four residuals of set_data's chain, each componentwise and scaled by the product of the magnitudes of its factors, in units
    of 2^-53, products in longdouble: they do not depend on the order of anybody's operations.  L, LB: lower triangles are read."""
    x = lambda A: np.asarray(A, dtype=LD)
    L, LB = np.tril(np.asarray(L, dtype=np.float64)), np.tril(np.asarray(LB, dtype=np.float64))
    G, c = np.asarray(G, dtype=np.float64), np.asarray(c, dtype=np.float64)
    aL, aLB = np.abs(L), np.abs(LB)
    s2 = LD(noise_var)
    M = L.shape[0]
    r1 = _ratio(x(L) @ x(L).T - x(st["Kuu"]), aL @ aL.T)
    r2 = _ratio(x(L) @ x(G) @ x(L).T - x(st["psi2"]), aL @ np.abs(G) @ aL.T)
    # G comes out of two one-sided solves and is symmetric only to cond(L) roundings (1e10 .. 1e13 units of |LB||LB^T| in every chain,
    # LAPACK's included); the factorisation reads its lower triangle and the trace its diagonal, so that triangle is what LB answers for
    r3 = _ratio(np.tril(x(LB) @ x(LB).T - (x(G) / s2 + np.eye(M, dtype=LD))), aLB @ aLB.T)
    r4 = _ratio(x(L) @ (x(LB) @ x(c)) - x(st["psi1"]).T @ x(Y) / s2, aL @ (aLB @ np.abs(c)))
    return np.array([r1, r2, r3, r4])


def predict_residuals(Kus, L, LB, tmp1, tmp2):
    x = lambda A: np.asarray(A, dtype=LD)
    L, LB = np.tril(np.asarray(L, dtype=np.float64)), np.tril(np.asarray(LB, dtype=np.float64))
    return np.array([_ratio(x(L) @ x(tmp1) - x(Kus), np.abs(L) @ np.abs(tmp1)), _ratio(x(LB) @ x(tmp2) - x(tmp1), np.abs(LB) @ np.abs(tmp2))])


def lapack_chain_residuals(c, st):
    """the six residuals (STAGES + PREDICT_STAGES) of the LAPACK / scipy chain on the statistics st"""
    import scipy.linalg as sla
    state = collapsed_from(st["Kuu"], st["psi0"], st["psi1"], st["psi2"], c["Y"], c["noise"], np.float64, lapack=True)
    tmp1 = sla.solve_triangular(state["L"], st["Kus"], lower=True)
    tmp2 = sla.solve_triangular(state["LB"], tmp1, lower=True)
    return np.concatenate([stage_residuals(st, c["Y"], c["noise"], state["L"], state["G"], state["LB"], state["c"]),
                           predict_residuals(st["Kus"], state["L"], state["LB"], tmp1, tmp2)])


def assembly_terms(LB, G, c, Y, psi0, noise_var):
    """the six terms of the bound in longdouble from given LB, G = L^-1 psi2 L^-T and c (the formulas of collapsed_from)"""
    x = lambda A: np.asarray(A, dtype=LD)
    LB, G, c, Y = x(LB), x(G), x(c), x(Y)
    N, DY = Y.shape
    s2 = LD(noise_var)
    two_pi = LD(2) * LD("3.14159265358979323846264338327950288")
    return np.array([LD(-0.5) * LD(N * DY) * np.log(two_pi * s2), -LD(DY) * np.sum(np.log(np.diag(LB))), LD(-0.5) * np.sum(Y * Y) / s2,
                     LD(0.5) * np.sum(c * c), LD(-0.5) * LD(DY) * LD(psi0) / s2, LD(0.5) * LD(DY) * np.trace(G) / s2], dtype=LD)


# ---------------------------------------------------------------------------------------------------------------- the truth at cond 1e8
# At cond(Kuu) of 1e7 .. 1e8 the plain longdouble chain is itself only good to cond x 2^-64: a permutation of the inducing inputs moves
# its mean by 1e-12 of max |Y|.  The truth of the ill-conditioned cases therefore carries every number of the ill-conditioned part of the
# chain as an unevaluated sum hi + lo of two longdoubles (Dekker 1971 / Knuth's error-free sum and product, splitter 2^32 + 1 for the
# 64-bit mantissa; about 37 digits), still numpy.longdouble and written-out loops.  Logarithms, the constant terms and K(X*, X*) stay in
# plain longdouble: nothing amplifies their 1e-19.
_SPLITTER = LD(2 ** 32 + 1)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _renorm(s, e):
    h = s + e
    return h, e - (h - s)


def _two_prod(a, b):
    p = a * b
    t = _SPLITTER * a
    ah = t - (t - a)
    al = a - ah
    t = _SPLITTER * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dd(a):
    a = np.asarray(a, dtype=LD)
    return a, np.zeros_like(a)


def dd_add(x, y):
    s, e = _two_sum(x[0], y[0])
    return _renorm(s, e + (x[1] + y[1]))


def dd_sub(x, y):
    return dd_add(x, (-y[0], -y[1]))


def dd_mul(x, y):
    p, e = _two_prod(x[0], y[0])
    return _renorm(p, e + (x[0] * y[1] + x[1] * y[0]))


def dd_div(x, y):
    q1 = x[0] / y[0]
    r = dd_sub(x, dd_mul(y, (q1, np.zeros_like(q1))))
    q2 = r[0] / y[0]
    r = dd_sub(r, dd_mul(y, (q2, np.zeros_like(q2))))
    q3 = r[0] / y[0]
    h, l = _renorm(q1, q2)
    return _renorm(h, l + q3)


def dd_sqrt(x):
    s = np.sqrt(x[0])
    r = dd_sub(x, dd_mul((s, np.zeros_like(s)), (s, np.zeros_like(s))))
    return _renorm(s, r[0] / (LD(2) * s))


def dd_sum(x, axis=0):
    """pairwise sum along one axis"""
    h, l = np.moveaxis(x[0], axis, 0), np.moveaxis(x[1], axis, 0)
    if h.shape[0] == 0:
        return np.zeros(h.shape[1:], dtype=LD), np.zeros(h.shape[1:], dtype=LD)
    while h.shape[0] > 1:
        m = h.shape[0] // 2
        sh, sl = dd_add((h[:m], l[:m]), (h[m:2 * m], l[m:2 * m]))
        h, l = np.concatenate([sh, h[2 * m:]]), np.concatenate([sl, l[2 * m:]])
    return h[0], l[0]


def dd_matmul(A, B):
    """(m, k) @ (k, n)"""
    P = dd_mul((A[0][:, :, None], A[1][:, :, None]), (B[0][None, :, :], B[1][None, :, :]))
    return dd_sum(P, axis=1)


def dd_T(x):
    return x[0].T, x[1].T


def dd_value(x):
    return x[0] + x[1]


def dd_chol(A):
    n = A[0].shape[0]
    Lh, Ll = np.zeros((n, n), dtype=LD), np.zeros((n, n), dtype=LD)
    for j in range(n):
        col = (A[0][j:, j], A[1][j:, j])
        if j:
            prod = dd_matmul((Lh[j:, :j], Ll[j:, :j]), (Lh[j, :j][:, None], Ll[j, :j][:, None]))
            col = dd_sub(col, (prod[0][:, 0], prod[1][:, 0]))
        if not col[0][0] > 0:
            raise np.linalg.LinAlgError("not positive definite")
        piv = dd_sqrt((col[0][:1], col[1][:1]))
        Lh[j, j], Ll[j, j] = piv[0][0], piv[1][0]
        if j + 1 < n:
            q = dd_div((col[0][1:], col[1][1:]), piv)
            Lh[j + 1:, j], Ll[j + 1:, j] = q
    return Lh, Ll


def dd_solve_lower(L, B):
    n = L[0].shape[0]
    Xh, Xl = np.array(B[0], dtype=LD), np.array(B[1], dtype=LD)
    for i in range(n):
        acc = (Xh[i:i + 1], Xl[i:i + 1])
        if i:
            acc = dd_sub(acc, dd_matmul((L[0][i:i + 1, :i], L[1][i:i + 1, :i]), (Xh[:i], Xl[:i])))
        q = dd_div(acc, (L[0][i, i], L[1][i, i]))
        Xh[i], Xl[i] = q[0][0], q[1][0]
    return Xh, Xl


def truth(c, st, perm=None):
    """the chain of evaluate() on the statistics st with the ill-conditioned part in double-longdouble: dict(bound, terms, mean, var, cov)
    as longdouble.  c = LB^-1 L^-1 (psi1^T Y) / s2 is formed without the N columns of A — the same number."""
    M = st["Kuu"].shape[0]
    p = np.arange(M) if perm is None else perm
    Y = np.asarray(c["Y"], dtype=LD)
    N, DY = Y.shape
    s2 = LD(c["noise"])
    ds2 = (s2, LD(0))
    L = dd_chol(dd(st["Kuu"][np.ix_(p, p)]))
    tmp = dd_solve_lower(L, dd(st["psi2"][np.ix_(p, p)]))
    G = dd_solve_lower(L, dd_T(tmp))
    AAT = dd_div(G, ds2)
    LB = dd_chol(dd_add(AAT, dd(np.eye(M))))
    rhs = dd_div(dd_matmul(dd(st["psi1"][:, p].T), dd(Y)), ds2)
    cc = dd_solve_lower(LB, dd_solve_lower(L, rhs))
    dLB = (np.diag(LB[0]), np.diag(LB[1]))
    two_pi = LD(2) * LD("3.14159265358979323846264338327950288")
    half = LD(0.5)
    terms = np.array([-half * LD(N * DY) * np.log(two_pi * s2), -LD(DY) * np.sum(np.log(dLB[0]) + dLB[1] / dLB[0]), -half * np.sum(Y * Y) / s2,
                      half * dd_value(dd_sum(dd_sum(dd_mul(cc, cc), 0), 0)), -half * LD(DY) * LD(st["psi0"]) / s2,
                      half * LD(DY) * dd_value(dd_sum((np.diag(AAT[0]), np.diag(AAT[1])), 0))], dtype=LD)
    tmp1 = dd_solve_lower(L, dd(st["Kus"][p]))
    tmp2 = dd_solve_lower(LB, tmp1)
    mean = dd_value(dd_matmul(dd_T(tmp2), cc))
    q = dd_sub(dd_sum(dd_mul(tmp2, tmp2), 0), dd_sum(dd_mul(tmp1, tmp1), 0))
    var = LD(c["variance"]) + dd_value(q)
    Q = dd_sub(dd_matmul(dd_T(tmp2), tmp2), dd_matmul(dd_T(tmp1), tmp1))
    cov = rbf(c["Xs"], c["Xs"], c["variance"], c["ls"], LD) + dd_value(Q)
    return dict(bound=np.sum(terms), terms=terms, mean=mean, var=np.tile(var[:, None], [1, DY]), cov=np.tile(cov[:, :, None], [1, 1, DY]))
