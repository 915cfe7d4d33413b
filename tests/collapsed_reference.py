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


def collapsed(mu, s, Z, variance, ls, Y, noise_var, jitter, dtype=LD):
    """dict: bound, terms (6, in the order of dsdgp_collapsed_bound), L, LB, c and the inputs the prediction needs"""
    T = dtype
    psi0, psi1, psi2 = P.psi(mu, s, Z, variance, ls, dtype=T)
    Y = np.asarray(Y, dtype=T)
    N, DY = Y.shape
    M = np.asarray(Z).shape[0]
    s2 = T(noise_var)
    sigma = np.sqrt(s2)
    Kuu = rbf(Z, Z, variance, ls, T) + T(jitter) * np.eye(M, dtype=T)
    L = chol(Kuu)
    A = solve_lower(L, psi1.T) / sigma
    tmp = solve_lower(L, psi2)
    AAT = solve_lower(L, tmp.T) / s2
    LB = chol(AAT + np.eye(M, dtype=T))
    c = solve_lower(LB, A @ Y) / sigma
    two_pi = T(2) * (np.pi if T is np.float64 else LD("3.14159265358979323846264338327950288"))
    terms = np.array([T(-0.5) * T(N * DY) * np.log(two_pi * s2), -T(DY) * np.sum(np.log(np.diag(LB))), T(-0.5) * np.sum(Y * Y) / s2,
                      T(0.5) * np.sum(c * c), T(-0.5) * T(DY) * psi0 / s2, T(0.5) * T(DY) * np.trace(AAT)], dtype=T)
    return dict(bound=np.sum(terms), terms=terms, L=L, LB=LB, c=c, Z=np.asarray(Z, dtype=T), variance=variance, ls=ls, DY=DY, dtype=T)


def predict(state, Xs, full_cov=False):
    """(mean (N*, DY), var (N*, DY) or (N*, N*, DY)) of layers.py:512-525"""
    T = state["dtype"]
    Kus = rbf(state["Z"], Xs, state["variance"], state["ls"], T)
    tmp1 = solve_lower(state["L"], Kus)
    tmp2 = solve_lower(state["LB"], tmp1)
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
    apart), and e64 would then measure the luck of one order rather than the rounding level."""
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
