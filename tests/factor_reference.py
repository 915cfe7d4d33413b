"""CPU side of tests/test_gpu_factor_direct.py: the inducing-point families, the reference Ku (the oracle's kernel + jitter), the
LAPACK factor and its two inverses, the residual measures in extended precision, and the 40-digit truth.  No GPU, no product code:
tests/test_factor_reference_cpu.py runs all of it through LAPACK and holds the reference itself to every bar.

Measures (eps = 2^-52, n = M, the real part of the padded matrix; products in numpy.longdouble — 64-bit mantissa on x86-64 — below
n = 1024, in float64 from there on, where the bars get the product's own n eps):
  factor_backward    max|L L^T - Ku| / max|Ku|                               bar 1e-14 n  (the project's potrf bar)
  inverse_residuals  max|X L - I| / (n eps max(|X||L|)), max|L X - I| / (n eps max(|L||X|))
  congruence_residual max|X Ku X^T - I| / (n eps max(|X||L||L^T||X^T|))      (the inverse against Ku where no Lu is kept)
  kinv_residual      max|Kinv Ku - I| / (n eps max(|Kinv||Ku|))
  kinv_asymmetry     max|Kinv - Kinv^T| / max|Kinv|                          bar n eps
  forward_error      max|A - A_true| / max|A_true|  against the factor / inverse computed with 40 digits
The bars of the scaled measures are relative to the same measure of a CPU result: device_bar()."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

EPS = 2.0 ** -52
LD = np.longdouble
FLOAT64_PRODUCTS_FROM = 1024          # n >= this: float64 products, bars + n eps (scaled measures: + 1.0)
DEVICE_FACTOR = 8.0                   # margin over the CPU reference for another summation order (MFMA 16x16x4 blocks, two accumulators)

FAMILIES = ("spread", "pairs", "grid1d")


def family_case(family, M, kind="rbf", seed=0):
    """-> (Z (M x D), kernel spec dict for tests.helpers.kern_spec / oracle.Kern).
    spread: Z = 2 randn, D = 3.   pairs: near-duplicate twins M/2 apart (second half = first half + 1e-4 randn), D = 2: they straddle
    the 16-row and 128-row block borders of the blocked factorisations.   grid1d: a 1-D grid in [0, 1], lengthscale 0.5: the smooth,
    numerically low-rank Gram matrix."""
    rng = np.random.RandomState(1000 * seed + M)
    if family == "spread":
        Z, ls = 2.0 * rng.randn(M, 3), 1.0
    elif family == "pairs":
        h = M // 2
        base = rng.randn(M - h, 2)
        Z, ls = np.concatenate([base, base[:h] + 1e-4 * rng.randn(h, 2)]), 1.0
    elif family == "grid1d":
        Z, ls = np.linspace(0.0, 1.0, M)[:, None].copy(), 0.5
    else:
        raise ValueError(family)
    D = Z.shape[1]
    return Z, dict(kind=kind, input_dim=D, variance=1.0, lengthscales=ls, ARD=False, white_variance=None)


def reference_ku(Z, spec, jitter):
    """Ku = K(Z, Z) + jitter I as layers.py:171 forms it (the oracle's kernel: float64, expand-the-square distances).  A factorisation
    reads one triangle: the lower one, mirrored (BLAS leaves Z Z^T unsymmetric in the last bit)."""
    from oracle import dgp_oracle as O
    K = O.Kern(**spec).K(O.NP, np.asarray(Z, dtype=np.float64)) + jitter * np.eye(Z.shape[0])
    return np.tril(K) + np.tril(K, -1).T


# ------------------------------------------------------------------------------------------------ extended-precision products
_POOL = None


def _pool():
    global _POOL
    if _POOL is None:
        _POOL = ThreadPoolExecutor(max_workers=max(1, min(8, len(os.sched_getaffinity(0)))))
    return _POOL


def xprod(A, B, a_lower=False):
    """A @ B in longdouble (float64 for n >= FLOAT64_PRODUCTS_FROM), row blocks in parallel (numpy's longdouble matmul is a plain
    loop that releases the GIL).  a_lower: A is lower-triangular — row block [r0, r1) stops at column r1."""
    n = A.shape[0]
    if n >= FLOAT64_PRODUCTS_FROM:
        return np.asarray(A, dtype=np.float64) @ np.asarray(B, dtype=np.float64)
    A, B = np.ascontiguousarray(A, dtype=LD), np.ascontiguousarray(B, dtype=LD)
    step = 32
    blocks = [(r0, min(n, r0 + step)) for r0 in range(0, n, step)]

    def one(b):
        r0, r1 = b
        k = min(r1, A.shape[1]) if a_lower else A.shape[1]
        return A[r0:r1, :k] @ B[:k]

    return np.concatenate(list(_pool().map(one, blocks)), axis=0)


def product_slack(n):
    """what a float64 product adds to a scaled residual (n >= FLOAT64_PRODUCTS_FROM): |fl(A B) - A B| <= n eps |A||B|, i.e. 1.0"""
    return 1.0 if n >= FLOAT64_PRODUCTS_FROM else 0.0


def _maxabs(A):
    return float(np.max(np.abs(A)))


def factor_backward(L, Ku):
    """max|L L^T - Ku| / max|Ku| reading the lower triangle of L only"""
    Ll = np.tril(np.asarray(L, dtype=np.float64))
    R = xprod(Ll, Ll.T, a_lower=True) - Ku
    return _maxabs(R) / _maxabs(Ku)


def factor_bar(n):
    return 1e-14 * n + (n * EPS if n >= FLOAT64_PRODUCTS_FROM else 0.0)


def inverse_residuals(X, L):
    """(left, right): max|X L - I| / (n eps max(|X||L|)), max|L X - I| / (n eps max(|L||X|)); X, L lower-triangular n x n"""
    n = L.shape[0]
    X, L = np.tril(np.asarray(X, dtype=np.float64)), np.tril(np.asarray(L, dtype=np.float64))
    I = np.eye(n)
    aX, aL = np.abs(X), np.abs(L)
    left = _maxabs(xprod(X, L, a_lower=True) - I) / (n * EPS * _maxabs(aX @ aL))
    right = _maxabs(xprod(L, X, a_lower=True) - I) / (n * EPS * _maxabs(aL @ aX))
    return left, right


def congruence_residual(X, Ku, L):
    """max|X Ku X^T - I| / (n eps max(|X| |L||L^T| |X^T|)): the inverse factor against Ku itself, for models that keep no Lu.  L (any
    factor of Ku to working accuracy) only enters the scale: X (L L^T + E) X^T with |E| <= n eps |L||L^T| is what a backward-stable
    factorisation followed by a stable inversion leaves."""
    n = Ku.shape[0]
    X = np.tril(np.asarray(X, dtype=np.float64))
    aX, aL = np.abs(X), np.abs(np.tril(L))
    R = xprod(xprod(X, Ku, a_lower=True), X.T) - np.eye(n)
    return _maxabs(R) / (n * EPS * _maxabs(aX @ (aL @ aL.T) @ aX.T))


def kinv_residual(Kinv, Ku):
    n = Ku.shape[0]
    return _maxabs(xprod(Kinv, Ku) - np.eye(n)) / (n * EPS * _maxabs(np.abs(Kinv) @ np.abs(Ku)))


def kinv_asymmetry(Kinv):
    return _maxabs(Kinv - Kinv.T) / _maxabs(Kinv)


def device_bar(cpu_value, n, factor=DEVICE_FACTOR):
    """bar of a scaled measure: `factor` x the CPU reference's own value, never below 1.0 (+ the float64 product's share at large n)"""
    return max(1.0, factor * cpu_value) + product_slack(n)


# ------------------------------------------------------------------------------------------------ the CPU reference
def lapack_reference(Ku):
    """LAPACK dpotrf, then Lu^-1 twice: forward substitution on the identity (dtrtrs) and dtrtri"""
    import scipy.linalg as sla
    L = np.linalg.cholesky(Ku)
    X_sub = np.tril(sla.solve_triangular(L, np.eye(L.shape[0]), lower=True))
    X_tri, info = sla.lapack.dtrtri(L, lower=1)
    assert info == 0
    return L, X_sub, np.tril(X_tri)


def reference_measures(Ku, with_kinv=True):
    """every measure of the CPU reference on Ku: dict with L, X_sub, X_tri, cond, factor, left / right (the larger of the two inverses),
    kinv (of X^T X from the inverse with the larger residual) and the individual values"""
    L, X_sub, X_tri = lapack_reference(Ku)
    n = Ku.shape[0]
    out = dict(L=L, X_sub=X_sub, X_tri=X_tri, n=n, cond=float(np.linalg.cond(Ku)), factor=factor_backward(L, Ku))
    ls, rs = inverse_residuals(X_sub, L)
    lt, rt = inverse_residuals(X_tri, L)
    cs, ct = congruence_residual(X_sub, Ku, L), congruence_residual(X_tri, Ku, L)
    out.update(left_sub=ls, right_sub=rs, left_tri=lt, right_tri=rt, left=max(ls, lt), right=max(rs, rt), congr_sub=cs, congr_tri=ct,
               congr=max(cs, ct))
    if with_kinv:
        ks, kt = kinv_residual(X_sub.T @ X_sub, Ku), kinv_residual(X_tri.T @ X_tri, Ku)
        out.update(kinv_sub=ks, kinv_tri=kt, kinv=max(ks, kt))
    return out


# ------------------------------------------------------------------------------------------------ 40-digit truth
_TRUTHS = {}


def _truth_key(Ku):
    Ku = np.ascontiguousarray(Ku, dtype=np.float64)
    return (Ku.shape[0], Ku.tobytes())


def _truth_compute(key):
    import mpmath
    n = key[0]
    Ku = np.frombuffer(key[1], dtype=np.float64).reshape(n, n)
    with mpmath.workdps(40):
        mpf = mpmath.mpf
        A = np.array([[mpf(float(Ku[i, j])) for j in range(n)] for i in range(n)], dtype=object)
        L = np.full((n, n), mpf(0), dtype=object)
        for j in range(n):
            d = A[j, j] - (np.dot(L[j, :j], L[j, :j]) if j else mpf(0))
            assert d > 0
            ljj = mpmath.sqrt(d)
            L[j, j] = ljj
            if j + 1 < n:
                s = A[j + 1:, j] - (L[j + 1:, :j].dot(L[j, :j]) if j else mpf(0))
                L[j + 1:, j] = s / ljj
        X = np.full((n, n), mpf(0), dtype=object)          # row i of X:  X_i,: = (e_i - L_i,:i X_:i,:) / L_ii
        for i in range(n):
            row = -(L[i, :i].dot(X[:i, :i + 1])) if i else np.full(1, mpf(0), dtype=object)
            row[i] = row[i] + mpf(1)
            X[i, :i + 1] = row / L[i, i]
        to_ld = np.vectorize(lambda v: LD(mpmath.nstr(v, 25)), otypes=[LD])
        return to_ld(L), to_ld(X)


def truth(Ku):
    """(L, X = L^-1) of the float64 matrix Ku computed with mpmath at 40 decimal digits, returned as longdouble (19 digits: far below
    every error that is compared with them).  Cached per matrix."""
    key = _truth_key(Ku)
    if key not in _TRUTHS:
        _TRUTHS[key] = _truth_compute(key)
    return _TRUTHS[key]


def truth_many(matrices, workers=8):
    """fill the cache for several matrices at once in fresh worker processes (pure Python arithmetic: one interpreter per core)"""
    import multiprocessing
    keys = [k for k in dict.fromkeys(_truth_key(K) for K in matrices) if k not in _TRUTHS]
    if not keys:
        return
    keys.sort(key=lambda k: -k[0])
    if len(keys) == 1:
        _TRUTHS[keys[0]] = _truth_compute(keys[0])
        return
    workers = max(1, min(workers, len(keys), len(os.sched_getaffinity(0))))
    with multiprocessing.get_context("spawn").Pool(workers) as pool:
        for k, v in zip(keys, pool.map(_truth_compute, keys, chunksize=1)):
            _TRUTHS[k] = v


def forward_error(A, A_true):
    """entrywise max error relative to max|A_true| over the lower triangle"""
    D = np.tril(np.asarray(A, dtype=LD) - A_true)
    return float(np.max(np.abs(D)) / np.max(np.abs(A_true)))
