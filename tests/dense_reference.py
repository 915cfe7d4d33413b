"""Reference of the dense layers (layers.GPR_Layer, layers.GPMC_Layer; the reference's layers.py:263-293, 310-342) in numpy, at a
chosen precision: long double is the truth of tests/test_gpu_dense_layers.py and tests/test_gpu_heinonen.py, float64 the same operation
sequence at the device's precision (its distance from the truth is e64 of the project's bar).  numpy's linalg has no long double, so
the factorisation and the triangular solves are written out here (row by row, vectorised along the row) and used at both precisions.
mag of an entry is the sum of the magnitudes of the terms added into it (a dot product's |a_k| |b_k|, a sum's |t_k|; where the summands
are themselves sums of products, as dF/dK inside the reverse pass of the Gram matrix, the leaf products); what the factorisation and the
triangular solves lose is in e64.

    GPR:  K = k(F, F) + (white + s2) I,  L = chol(K),  V = L^-1 (Y - m(F)),  alpha = L^-T V
          bound = -1/2 N DY log 2 pi - DY sum log L_ii - 1/2 sum V^2
          dF/dK = 1/2 (alpha alpha^T - DY K^-1), pushed back through the Gram matrix (tests/gram_grad_reference.py); dF/dm = alpha
          at X*: A = L^-1 k(F, X*), mean = A^T V + m(X*), var = kdiag - colsum(A^2) or k(X*, X*) - A^T A
    GPMC: Lu = chol(k(X, X) + (white + jitter) I), f = Lu q_mu + m(X), vjp(dF) = Lu^T dF
          at X*: A = Lu^-1 k(X, X*), mean = A^T q_mu + m(X*), var as above"""
import numpy as np

from tests import gram_grad_reference as GR

LD = np.longdouble


def two_pi(dtype):
    return dtype(8.0) * np.arctan(dtype(1.0))


def chol(A, dtype):
    A = np.array(A, dtype=dtype)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - np.sum(L[j, :j] * L[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_lower(L, B, trans=False):
    """L^-1 B, with trans L^-T B"""
    B = np.array(B, dtype=L.dtype)
    n = L.shape[0]
    if not trans:
        for i in range(n):
            B[i] = (B[i] - L[i, :i] @ B[:i]) / L[i, i]
    else:
        for i in range(n - 1, -1, -1):
            B[i] = (B[i] - L[i + 1:, i] @ B[i + 1:]) / L[i, i]
    return B


def mean_fn(mean, X, dtype):
    """mean: None (Zero), "identity", or (A, b) of a Linear"""
    X = np.asarray(X, dtype=dtype)
    if mean is None:
        return None
    if isinstance(mean, str):
        return X
    A, b = mean
    return X @ np.asarray(A, dtype=dtype) + np.asarray(b, dtype=dtype)


def _kdiag(variance, white, dtype):
    return dtype(variance) + dtype(white or 0.0)


def gpr(kind, F, Y, variance, ls, ard, white, s2, mean=None, Xnew=None, dtype=LD):
    """-> (res, mag): dicts with `bound`, `terms` (3), the gradients `variance`, `lengthscales`, `lik_variance`, `white_variance` (the
    same entry as lik_variance; present with a White part), `X_mean`, and with Xnew `mean`, `var` (N*, DY), `cov` (N*, N*)"""
    F, Y = np.asarray(F, dtype=dtype), np.asarray(Y, dtype=dtype)
    N, DY = Y.shape
    K = GR.gram(kind, F, None, variance, ls, dtype(white or 0.0) + dtype(s2), dtype=dtype)
    L = chol(K, dtype)
    m = mean_fn(mean, F, dtype)
    V = solve_lower(L, Y if m is None else Y - m)
    res, mag = {}, {}
    logs = np.log(np.diagonal(L))
    t = np.array([dtype(-0.5) * N * DY * np.log(two_pi(dtype)), -dtype(DY) * np.sum(logs), dtype(-0.5) * np.sum(V * V)], dtype=dtype)
    res["terms"], mag["terms"] = t, np.array([abs(t[0]), DY * np.sum(np.abs(logs)), abs(t[2])], dtype=dtype)
    res["bound"], mag["bound"] = np.atleast_1d((t[0] + t[1]) + t[2]), np.atleast_1d(np.sum(mag["terms"]))
    alpha = solve_lower(L, V, trans=True)
    Li = solve_lower(L, np.eye(N, dtype=dtype))
    Ki = Li.T @ Li
    dK = dtype(0.5) * (alpha @ alpha.T) - dtype(0.5) * DY * Ki
    g, _ = GR.gram_grad(kind, F, None, dK, variance, ls, ard, dtype=dtype)
    # dF/dK is itself a sum of products (alpha alpha^T, L^-T L^-1), and the reverse pass of the Gram matrix sums over it: the terms added
    # into an entry of the result are the leaf products, so mag is taken through both sums
    dK_mag = dtype(0.5) * (np.abs(alpha) @ np.abs(alpha).T) + dtype(0.5) * DY * (np.abs(Li).T @ np.abs(Li))
    _, gm = GR.gram_grad(kind, F, None, dK_mag, variance, ls, ard, dtype=dtype)
    dX, dXm = g["X"], gm["X"]
    if isinstance(mean, str):
        dX, dXm = dX + alpha, dXm + np.abs(alpha)
    elif mean is not None:
        A = np.asarray(mean[0], dtype=dtype)
        dX, dXm = dX + alpha @ A.T, dXm + np.abs(alpha) @ np.abs(A).T
    res.update(variance=g["variance"], lengthscales=g["lengthscales"], lik_variance=g["diag"], X_mean=dX)
    mag.update(variance=gm["variance"], lengthscales=gm["lengthscales"], lik_variance=gm["diag"], X_mean=dXm)
    if white is not None:
        res["white_variance"], mag["white_variance"] = g["diag"], gm["diag"]
    if Xnew is not None:
        _predict(res, mag, kind, F, L, V, Xnew, variance, ls, white, mean, dtype)
    return res, mag


def _predict(res, mag, kind, X, L, W, Xnew, variance, ls, white, mean, dtype):
    """mean = A^T W + m(X*), var, cov from A = L^-1 k(X, X*)"""
    Xs = np.asarray(Xnew, dtype=dtype)
    A = solve_lower(L, GR.gram(kind, X, Xs, variance, ls, dtype=dtype))
    mu, mum = A.T @ W, np.abs(A).T @ np.abs(W)
    ms = mean_fn(mean, Xs, dtype)
    if ms is not None:
        mu, mum = mu + ms, mum + np.abs(ms)
    kd, a2 = _kdiag(variance, white, dtype), np.sum(A * A, 0)
    res["mean"], mag["mean"] = mu, mum
    res["var"], mag["var"] = np.tile((kd - a2)[:, None], [1, W.shape[1]]), np.tile((kd + a2)[:, None], [1, W.shape[1]])
    Kss = GR.gram(kind, Xs, None, variance, ls, dtype(white or 0.0), dtype=dtype)
    res["cov"], mag["cov"] = Kss - A.T @ A, np.abs(Kss) + np.abs(A).T @ np.abs(A)


def gpmc(kind, X, q_mu, variance, ls, white, jitter, mean=None, dF=None, Xnew=None, dtype=LD):
    """-> (res, mag): `Lu`, `latents` (N, D), with dF `vjp`, with Xnew `mean`, `var`, `cov`"""
    X, q = np.asarray(X, dtype=dtype), np.asarray(q_mu, dtype=dtype)
    Lu = chol(GR.gram(kind, X, None, variance, ls, dtype(white or 0.0) + dtype(jitter), dtype=dtype), dtype)
    res, mag = {"Lu": Lu}, {}
    f, fm = Lu @ q, np.abs(Lu) @ np.abs(q)
    m = mean_fn(mean, X, dtype)
    if m is not None:
        f, fm = f + m, fm + np.abs(m)
    res["latents"], mag["latents"] = f, fm
    if dF is not None:
        dF = np.asarray(dF, dtype=dtype)
        res["vjp"], mag["vjp"] = Lu.T @ dF, np.abs(Lu).T @ np.abs(dF)
    if Xnew is not None:
        _predict(res, mag, kind, X, Lu, q, Xnew, variance, ls, white, mean, dtype)
    return res, mag


def log_density(kind, X, Y, q_mu, variance0, ls0, jitter, variance1, ls1, ard1, s2, mean0=None, mean1=None, dtype=LD, Lu=None):
    """log p(Y | f) + log p(q_mu) of the two-layer dense model (DGP_Heinonen) and its gradient in q_mu -> (value, gradient, parts):
    f = Lu q_mu + m0(X), the GPR bound at f, the standard-normal prior of q_mu.  Lu: a factor to use as it is (the device's own)"""
    q = np.asarray(q_mu, dtype=dtype)
    if Lu is None:
        Lu = gpmc(kind[0], X, q, variance0, ls0, None, jitter, dtype=dtype)[0]["Lu"]
    Lu = np.asarray(Lu, dtype=dtype)
    f = Lu @ q
    m = mean_fn(mean0, X, dtype)
    if m is not None:
        f = f + m
    r, _ = gpr(kind[1], f, Y, variance1, ls1, ard1, None, s2, mean1, dtype=dtype)
    prior = dtype(-0.5) * np.sum(q * q) - dtype(0.5) * q.size * np.log(two_pi(dtype))
    return r["bound"][0] + prior, Lu.T @ r["X_mean"] - q, dict(r, prior=prior)
