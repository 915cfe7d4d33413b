"""Reference of the sparse conditional without q_sqrt and of its reverse pass (dsdgp_sparse_conditional[_grad], csrc/sparse_cond.hip; the
reference's layers.py:178-219 with `q_sqrt is None`, layers.py:249-260) in numpy, at a chosen precision: long double is the truth of
tests/test_gpu_sparse_cond.py and tests/test_gpu_sgpmc.py, float64 the same operation sequence at the device's precision (its distance
from the truth is e64 of the project's bar).  The factorisation and the triangular solves are those of tests/dense_reference.py (numpy's
linalg has no long double), the Gram matrix and its reverse pass those of tests/gram_grad_reference.py.

    Ku = K(Z, Z) + (white_variance + jitter) I,  Lu = chol(Ku),  A = Lu^-1 K(Z, X),  W = q_mu (white) or Lu^-1 q_mu,  kd = variance + white_variance
    mean = A^T W,  var_r = kd - sum_i A_ir^2
    A_bar = W gm^T - 2 A diag(gv),  W_bar = A gm,  K1_bar = Lu^-T A_bar,  Lu_bar = -tril(K1_bar A^T) [- tril((Lu^-T W_bar) W^T)],
    q_mu_bar = W_bar or Lu^-T W_bar,  Ku_bar = Lu^-T 1/2 (P + P^T) Lu^-1 with P = Phi(Lu^T Lu_bar),  kd_bar = sum_r gv_r
    d_Z = d_X of the cross form (Z, X, K1_bar) + d_X of the symmetric form (Z, Ku_bar);  d_X = the cross form's d_X2;  d_kern: the two
    forms' entries added, kd_bar into the variance and (with a White part) into the last entry, with the symmetric form's diagonal sum.

mag of an entry is the sum of the magnitudes of the terms added into it, taken through the products down to the leaf products (every
factor replaced by its magnitude, Lu^-1 by the magnitudes of the explicit inverse); what the factorisation and the solves lose is in e64."""
import numpy as np

from tests import dense_reference as DR
from tests import gram_grad_reference as GR

LD = np.longdouble
KEYS_FWD = ("mean", "var")
KEYS_REV = ("q_mu", "Z", "X", "variance", "lengthscales", "diag")


def _phi_sym(Q):
    """1/2 (P + P^T), P = Phi(Q) the lower triangle of Q with a halved diagonal: S_ij = 1/2 Q[max(i, j)][min(i, j)]"""
    L = np.tril(Q)
    return (L + L.T - np.diag(np.diagonal(Q))) * Q.dtype.type(0.5)


def factors(kind, Z, X, q_mu, variance, ls, white_variance, jitter, white, dtype=LD):
    Z, X, q = (np.asarray(a, dtype=dtype) for a in (Z, X, q_mu))
    wv = dtype(white_variance or 0.0)
    Lu = DR.chol(GR.gram(kind, Z, None, variance, ls, wv + dtype(jitter), dtype=dtype), dtype)
    A = DR.solve_lower(Lu, GR.gram(kind, Z, X, variance, ls, dtype=dtype))
    W = q if white else DR.solve_lower(Lu, q)
    return Z, X, Lu, A, W, dtype(variance) + wv


def forward(kind, Z, X, q_mu, variance, ls, white_variance, jitter, white, dtype=LD):
    """-> (res, mag): `mean` (n, DO), `var` (n,)"""
    Z, X, Lu, A, W, kd = factors(kind, Z, X, q_mu, variance, ls, white_variance, jitter, white, dtype)
    a2 = np.sum(A * A, 0)
    return dict(mean=A.T @ W, var=kd - a2), dict(mean=np.abs(A).T @ np.abs(W), var=kd + a2)


def full_cov(kind, Z, X, q_mu, variance, ls, white_variance, jitter, white, dtype=LD):
    """K(X, X) - A^T A (n, n), and its mag"""
    Z, X, Lu, A, W, kd = factors(kind, Z, X, q_mu, variance, ls, white_variance, jitter, white, dtype)
    K = GR.gram(kind, X, None, variance, ls, dtype(white_variance or 0.0), dtype=dtype)
    return K - A.T @ A, np.abs(K) + np.abs(A).T @ np.abs(A)


def reverse(kind, Z, X, q_mu, variance, ls, ard, white_variance, jitter, white, gm, gv, dtype=LD):
    """-> (res, mag): `q_mu` (M, DO), `Z` (M, D), `X` (n, D), `variance`, `lengthscales`, `diag` (shape (1,) or (D,))"""
    Z, X, Lu, A, W, kd = factors(kind, Z, X, q_mu, variance, ls, white_variance, jitter, white, dtype)
    gm, gv = np.asarray(gm, dtype=dtype), np.asarray(gv, dtype=dtype).reshape(-1)
    M = Z.shape[0]
    Li = DR.solve_lower(Lu, np.eye(M, dtype=dtype))
    aLi, aA, aW, aLu = np.abs(Li), np.abs(A), np.abs(W), np.abs(Lu)
    Abar, Abar_m = W @ gm.T - dtype(2.0) * A * gv[None, :], aW @ np.abs(gm).T + dtype(2.0) * aA * np.abs(gv)[None, :]
    Wbar, Wbar_m = A @ gm, aA @ np.abs(gm)
    K1, K1_m = DR.solve_lower(Lu, Abar, trans=True), aLi.T @ Abar_m
    T, T_m = K1 @ A.T, K1_m @ aA.T
    if white:
        qbar, qbar_m = Wbar, Wbar_m
    else:
        qbar, qbar_m = DR.solve_lower(Lu, Wbar, trans=True), aLi.T @ Wbar_m
        T, T_m = T + qbar @ W.T, T_m + qbar_m @ aW.T
    Lbar, Lbar_m = -np.tril(T), np.tril(T_m)
    S, S_m = _phi_sym(Lu.T @ Lbar), _phi_sym(aLu.T @ Lbar_m)
    Kbar = DR.solve_lower(Lu, DR.solve_lower(Lu, S, trans=True).T, trans=True).T
    Kbar_m = aLi.T @ S_m @ aLi
    g1, _ = GR.gram_grad(kind, Z, X, K1, variance, ls, ard, dtype=dtype)
    _, m1 = GR.gram_grad(kind, Z, X, K1_m, variance, ls, ard, dtype=dtype)
    g2, _ = GR.gram_grad(kind, Z, None, Kbar, variance, ls, ard, dtype=dtype)
    _, m2 = GR.gram_grad(kind, Z, None, Kbar_m, variance, ls, ard, dtype=dtype)
    kdbar, kdbar_m = np.sum(gv), np.sum(np.abs(gv))
    has_white = white_variance is not None
    res = dict(q_mu=qbar, Z=g1["X"] + g2["X"], X=g1["X2"], variance=g1["variance"] + g2["variance"] + kdbar,
               lengthscales=g1["lengthscales"] + g2["lengthscales"], diag=g2["diag"] + (kdbar if has_white else dtype(0.0)))
    mag = dict(q_mu=qbar_m, Z=m1["X"] + m2["X"], X=m1["X2"], variance=m1["variance"] + m2["variance"] + kdbar_m,
               lengthscales=m1["lengthscales"] + m2["lengthscales"], diag=m2["diag"] + (kdbar_m if has_white else dtype(0.0)))
    return res, mag


def functional(kind, Z, X, q_mu, variance, ls, white_variance, jitter, white, gm, gv, dtype=LD):
    """J = sum gm * mean + sum gv * var: the scalar whose gradient `reverse` returns"""
    r, _ = forward(kind, Z, X, q_mu, variance, ls, white_variance, jitter, white, dtype)
    return np.sum(np.asarray(gm, dtype=dtype) * r["mean"]) + np.sum(np.asarray(gv, dtype=dtype).reshape(-1) * r["var"])
