"""Reference of the pathwise function draws (csrc/pathwise.hip, doubly_stochastic_dgp/pathwise.py), plain numpy.  dtype = np.longdouble is
the truth, dtype = np.float64 the same operation sequence in double (the twin); every function returns (value, mag), mag the sum of the
magnitudes of the terms added into each entry, each sine / cosine term weighted by 1 + sum_d |x_d - c_d| |Omega_dj| (an ulp of theta moves
the term by that much).  Also: the basis sampler restated, the closed-form moments of a draw given the basis, and the replay of a draw's
normals through oracle/philox.py.

  theta_j(x) = sum_d (x_d - c_d) Omega_dj,   f0(x)_o = sqrt(s2 / L) sum_j [a_jo cos theta_j(x) + b_jo sin theta_j(x)]
  Ku = K(Z, Z) + (White variance + jitter) I,  Lu = chol(Ku),  u_o = q_mu_o + q_sqrt_o eps_o  (white: Lu times that)
  v = Ku^-1 (u - f0(Z)),   f(x)_o = f0(x)_o + sum_m k(x, z_m) v_mo + add(x)_o
"""
import numpy as np

from oracle import philox

LD = np.longdouble


def sample_basis(kind, D, L, lengthscales, rng):
    """Omega (D, L): g = standard_normal((D, L)); Matern52: times sqrt(5 / chisquare(5, L)) per frequency; row d over l_d"""
    g = rng.standard_normal((D, L))
    if kind == "matern52":
        g = g * np.sqrt(5.0 / rng.chisquare(5, size=L))[None, :]
    return g / np.broadcast_to(np.asarray(lengthscales, dtype=np.float64).reshape(-1), (D,))[:, None]


def kernel(kind, X, Z, variance, ls, dtype=LD):
    """k(X, Z) from the differences, (n, m)"""
    X, Z = np.asarray(X, dtype=dtype), np.asarray(Z, dtype=dtype)
    ls = np.broadcast_to(np.asarray(ls, dtype=dtype).reshape(-1), (X.shape[1],))
    t = (X[:, None, :] - Z[None, :, :]) * (dtype(1) / ls)
    r2 = np.sum(t * t, axis=-1)
    s2 = dtype(variance)
    if kind == "rbf":
        return s2 * np.exp(-r2 / 2)
    s5 = np.sqrt(dtype(5))
    r = np.sqrt(r2 + dtype(1e-12))
    return s2 * (1 + s5 * r + dtype(5) / 3 * (r * r)) * np.exp(-s5 * r)


def prior(X, Omega, origin, Wc, Ws, variance, dtype=LD):
    """f0 at X (n, D) for the draws Wc, Ws (S, L, DO): ((S, n, DO), mag)"""
    X, Om, c = np.asarray(X, dtype=dtype), np.asarray(Omega, dtype=dtype), np.asarray(origin, dtype=dtype)
    Wc, Ws = np.asarray(Wc, dtype=dtype), np.asarray(Ws, dtype=dtype)
    L = Om.shape[1]
    xc = X - c[None, :]
    th = xc @ Om
    weight = 1 + np.abs(xc) @ np.abs(Om)
    cs, sn = np.cos(th), np.sin(th)
    amp = np.sqrt(dtype(variance) / dtype(L))
    f0 = amp * (np.einsum("nj,sjo->sno", cs, Wc) + np.einsum("nj,sjo->sno", sn, Ws))
    mag = amp * (np.einsum("nj,sjo->sno", np.abs(cs) * weight, np.abs(Wc)) + np.einsum("nj,sjo->sno", np.abs(sn) * weight, np.abs(Ws)))
    return f0, mag


def evaluate(kind, X, Omega, origin, Wc, Ws, Z, V, variance, ls, add=None, dtype=LD):
    """f at X — (n, D) for every draw or (S, n, D) — as ((S, n, DO), mag).  V (S, M, DO) or None: the prior part alone.  add: None, or
    (n, DO) / (S, n, DO)"""
    S = np.shape(Wc)[0]
    X = np.asarray(X, dtype=dtype)
    if X.ndim == 2:                                      # the same rows for every draw: the basis functions once
        f, m = prior(X, Omega, origin, Wc, Ws, variance, dtype)
        if V is not None and np.shape(V)[1] > 0:
            K, v = kernel(kind, X, Z, variance, ls, dtype), np.asarray(V, dtype=dtype)
            f, m = f + np.einsum("nm,smo->sno", K, v), m + np.einsum("nm,smo->sno", np.abs(K), np.abs(v))
        if add is not None:
            a = np.asarray(add, dtype=dtype)
            f, m = f + a, m + np.abs(a)
        return f, m
    Xs = X
    out, mag = [], []
    for s in range(S):
        f, m = prior(Xs[s], Omega, origin, np.asarray(Wc)[s:s + 1], np.asarray(Ws)[s:s + 1], variance, dtype)
        f, m = f[0], m[0]
        if V is not None and np.shape(V)[1] > 0:
            K, v = kernel(kind, Xs[s], Z, variance, ls, dtype), np.asarray(V, dtype=dtype)[s]
            f, m = f + K @ v, m + np.abs(K) @ np.abs(v)
        if add is not None:
            a = np.asarray(add, dtype=dtype)
            a = a[s] if a.ndim == 3 else a
            f, m = f + a, m + np.abs(a)
        out.append(f), mag.append(m)
    return np.stack(out), np.stack(mag)


def cholesky(A):
    """lower Cholesky factor in A's dtype (numpy's own takes no long double); ValueError at a non-positive pivot"""
    A = np.array(A)
    n = A.shape[0]
    Lo = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - Lo[j, :j] @ Lo[j, :j]
        if not d > 0:
            raise ValueError(f"pivot {j + 1} is not positive")
        Lo[j, j] = np.sqrt(d)
        Lo[j + 1:, j] = (A[j + 1:, j] - Lo[j + 1:, :j] @ Lo[j, :j]) / Lo[j, j]
    return Lo


def solve_lower(Lo, B, trans=False):
    """Lo^-1 B, with trans Lo^-T B, by substitution in Lo's dtype"""
    n = Lo.shape[0]
    Xo = np.array(B, dtype=Lo.dtype)
    if not trans:
        for i in range(n):
            Xo[i] = (Xo[i] - Lo[i, :i] @ Xo[:i]) / Lo[i, i]
    else:
        for i in range(n - 1, -1, -1):
            Xo[i] = (Xo[i] - Lo[i + 1:, i] @ Xo[i + 1:]) / Lo[i, i]
    return Xo


def ku(kind, Z, variance, ls, white_var, jitter, dtype=LD):
    M = np.shape(Z)[0]
    return kernel(kind, Z, Z, variance, ls, dtype) + (dtype(white_var or 0.0) + dtype(jitter)) * np.eye(M, dtype=dtype)


def inducing_draws(Lu, q_mu, q_sqrt, eps, white, dtype=LD):
    """u (S, M, DO) and the magnitudes of its terms"""
    q_mu, eps = np.asarray(q_mu, dtype=dtype), np.asarray(eps, dtype=dtype)
    S = eps.shape[0]
    u = np.broadcast_to(q_mu[None], (S,) + q_mu.shape).copy()
    mag = np.abs(u)
    if q_sqrt is not None:
        q = np.tril(np.asarray(q_sqrt, dtype=dtype))
        u = u + np.einsum("omk,sko->smo", q, eps)
        mag = mag + np.einsum("omk,sko->smo", np.abs(q), np.abs(eps))
    if white:
        u, mag = np.einsum("mk,sko->smo", Lu, u), np.einsum("mk,sko->smo", np.abs(Lu), mag)
    return u, mag


def weights(kind, Z, Omega, origin, Wc, Ws, q_mu, q_sqrt, eps, variance, ls, white_var, jitter, white, dtype=LD):
    """v = Ku^-1 (u - f0(Z)): ((S, M, DO), mag), mag = |Ku^-1| times the magnitudes of the terms of u - f0(Z)"""
    Ku = ku(kind, Z, variance, ls, white_var, jitter, dtype)
    Lu = cholesky(Ku)
    if eps is None:
        eps = np.zeros((np.shape(Wc)[0],) + tuple(np.shape(q_mu)))
    u, umag = inducing_draws(Lu, q_mu, q_sqrt, eps, white, dtype)
    f0, fmag = prior(Z, Omega, origin, Wc, Ws, variance, dtype)
    M = Ku.shape[0]
    Kinv = solve_lower(Lu, solve_lower(Lu, np.eye(M, dtype=dtype)), trans=True)
    v = np.stack([solve_lower(Lu, solve_lower(Lu, u[s] - f0[s]), trans=True) for s in range(u.shape[0])])
    mag = np.einsum("mk,sko->smo", np.abs(Kinv), umag + fmag)
    return v, mag


def moments_given_basis(kind, X, Omega, origin, Z, q_mu, q_sqrt, variance, ls, white_var, jitter, white, dtype=LD):
    """exact mean (n, DO) and covariance (DO, n, n) of f(X) over the weights a, b, eps with the basis fixed (add = 0):
    mean = B E[u],  cov = K^(X, X) - B K^(Z, X) - K^(X, Z) B^T + B K^(Z, Z) B^T + B Cov[u_o] B^T,  B = k(X, Z) Ku^-1,
    K^(x, x') = s2 / L sum_j cos(theta_j(x) - theta_j(x'))"""
    X, Z = np.asarray(X, dtype=dtype), np.asarray(Z, dtype=dtype)
    Om, c = np.asarray(Omega, dtype=dtype), np.asarray(origin, dtype=dtype)
    n, L = X.shape[0], Om.shape[1]
    th = (np.concatenate([X, Z]) - c[None, :]) @ Om
    Khat = dtype(variance) / L * (np.cos(th) @ np.cos(th).T + np.sin(th) @ np.sin(th).T)
    Lu = cholesky(ku(kind, Z, variance, ls, white_var, jitter, dtype))
    B = solve_lower(Lu, solve_lower(Lu, kernel(kind, Z, X, variance, ls, dtype)), trans=True).T            # (n, M)
    q_mu = np.asarray(q_mu, dtype=dtype)
    Eu = Lu @ q_mu if white else q_mu
    base = Khat[:n, :n] - B @ Khat[n:, :n] - Khat[:n, n:] @ B.T + B @ Khat[n:, n:] @ B.T
    cov = []
    for o in range(q_mu.shape[1]):
        R = np.tril(np.asarray(q_sqrt, dtype=dtype)[o])
        R = Lu @ R if white else R
        BR = B @ R
        cov.append(base + BR @ BR.T)
    return B @ Eu, np.stack(cov)


def replay_normals(seed, l, S, L, M, DO):
    """layer l's normal draws as the device draws them: Wc, Ws (S, L, DO) from the streams 3l, 3l + 1, eps (S, M, DO) from 3l + 2"""
    Wc = philox.randn_reference(seed, 3 * l, S * L * DO).reshape(S, L, DO)
    Ws = philox.randn_reference(seed, 3 * l + 1, S * L * DO).reshape(S, L, DO)
    eps = philox.randn_reference(seed, 3 * l + 2, S * M * DO).reshape(S, M, DO)
    return Wc, Ws, eps


def ratio(dev, truth, twin, mag):
    """worst |dev - truth| / (8 max(e64, 2^-50 mag)) over the entries, e64 = |twin - truth|"""
    dev, truth, twin, mag = (np.atleast_1d(np.asarray(a)) for a in (dev, truth, twin, mag))
    err = np.abs(dev - truth).astype(np.float64)
    e64 = np.abs(twin - truth).astype(np.float64)
    bar = 8.0 * np.maximum(e64, 2.0 ** -50 * mag.astype(np.float64))
    if np.any(np.isnan(err)) or np.any((bar == 0.0) & (err != 0.0)):
        return float("inf")
    return float(np.max(err / np.where(bar == 0.0, 1.0, bar)))
