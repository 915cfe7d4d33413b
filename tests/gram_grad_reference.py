"""Reference of the reverse pass of the Gram matrix (dsdgp_gram_grad, csrc/gram_grad.hip) in numpy, at a chosen precision: long double
is the truth of tests/test_gpu_gram_grad.py, float64 the same operation sequence at the device's precision (its distance from the truth
is e64 of the project's bar).  Every x_d - y_d is the difference of the inputs, scaled afterwards.  Also the forward Gram matrix
(`gram`), which the tests of the reference differentiate numerically.

    u_d = (x_d - y_d) / l_d,  r2 = sum_d u_d^2,  k = v k1(r2),  dk1 = d k1 / d r2
    RBF: k1 = exp(-r2 / 2);  Matern52: r = sqrt(r2 + 1e-12), k1 = (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r), dk1 = -5/6 (1 + sqrt5 r) exp(-sqrt5 r)
    w = G (cross form), G + G^T (symmetric form);  t = 2 v w dk1;  f = 1 (cross), 1/2 (symmetric)
    d_X[i, d] = sum_j t_ij u_ijd / l_d,  d_X2[j, d] = -sum_i t_ij u_ijd / l_d,  d_l_d = -f sum_ij t_ij u_ijd^2 / l_d,  d_v = f sum_ij w_ij k1_ij
    diag = sum_i G_ii (symmetric form), 0 (cross form)
mag of an entry is the sum of the magnitudes of the terms added into it."""
import numpy as np

LD = np.longdouble
RBF, MATERN52 = 0, 1


def _k1(kind, r2, dtype):
    if kind == RBF:
        k1 = np.exp(dtype(-0.5) * r2)
        return k1, dtype(-0.5) * k1
    s5 = np.sqrt(dtype(5.0))
    r = np.sqrt(r2 + dtype(1e-12))
    e = np.exp(-s5 * r)
    return (dtype(1.0) + s5 * r + dtype(5.0) / dtype(3.0) * (r * r)) * e, -(dtype(5.0) / dtype(6.0)) * (dtype(1.0) + s5 * r) * e


def _scaled_differences(X, X2, ls, dtype):
    X, X2 = np.asarray(X, dtype=dtype), np.asarray(X2, dtype=dtype)
    D = X.shape[1]
    il = dtype(1.0) / np.broadcast_to(np.asarray(ls, dtype=dtype).reshape(-1), (D,))
    return (X[:, None, :] - X2[None, :, :]) * il, il


def gram(kind, X, X2, variance, ls, diag_add=0.0, dtype=LD):
    """K(X, X2), or K(X, X) + diag_add I with X2=None"""
    u, _ = _scaled_differences(X, X if X2 is None else X2, ls, dtype)
    K = dtype(variance) * _k1(kind, np.sum(u * u, -1), dtype)[0]
    if X2 is None:
        K = K + dtype(diag_add) * np.eye(K.shape[0], dtype=dtype)
    return K


def gram_grad(kind, X, X2, G, variance, ls, ard, dtype=LD):
    """-> (grad, mag): dicts with `X` (n, D), `X2` (n2, D; None with X2=None), `variance`, `lengthscales` (D entries with ard, else one),
    `diag` (shape (1,) each)"""
    sym = X2 is None
    G = np.asarray(G, dtype=dtype)
    u, il = _scaled_differences(X, X if sym else X2, ls, dtype)
    k1, dk1 = _k1(kind, np.sum(u * u, -1), dtype)
    w = G + G.T if sym else G
    f = dtype(0.5) if sym else dtype(1.0)
    t = dtype(2.0) * dtype(variance) * (w * dk1)
    tu = t[:, :, None] * u
    grad, mag = {}, {}
    grad["X"], mag["X"] = np.sum(tu, 1) * il, np.sum(np.abs(tu), 1) * il
    if sym:
        grad["X2"] = mag["X2"] = None
    else:
        grad["X2"], mag["X2"] = -np.sum(tu, 0) * il, np.sum(np.abs(tu), 0) * il
    sl, sl_mag = np.sum(tu * u, (0, 1)), np.sum(np.abs(tu * u), (0, 1))
    dl, dl_mag = -f * (sl * il), f * (sl_mag * il)
    if not ard:
        dl, dl_mag = np.sum(dl, keepdims=True), np.sum(dl_mag, keepdims=True)
    grad["lengthscales"], mag["lengthscales"] = dl, dl_mag
    grad["variance"], mag["variance"] = np.atleast_1d(f * np.sum(w * k1)), np.atleast_1d(f * np.sum(np.abs(w * k1)))
    dg = np.diagonal(G) if sym else np.zeros(1, dtype=dtype)
    grad["diag"], mag["diag"] = np.atleast_1d(np.sum(dg)), np.atleast_1d(np.sum(np.abs(dg)))
    return grad, mag
