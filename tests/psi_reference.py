"""The yardstick of the kernel-expectation tests (tests/test_psi_reference_cpu.py, tests/test_gpu_psi.py): the expectations of an RBF
kernel under a diagonal Gaussian input, GPflow 1.1.1's expectation(DiagonalGaussian, (RBF, InducingPoints)[, (RBF, InducingPoints)]),
in the DIRECT form

    psi0       = N v
    psi1[n, m] = v prod_d (l_d^2 / (l_d^2 + s_nd))^1/2 exp(-1/2 sum_d (mu_nd - z_md)^2 / (l_d^2 + s_nd))
    psi2[m, k] = sum_n v^2 prod_d (l_d^2 / (l_d^2 + 2 s_nd))^1/2
                 exp(-sum_d [(z_md - z_kd)^2 / (4 l_d^2) + (mu_nd - (z_md + z_kd) / 2)^2 / (l_d^2 + 2 s_nd)])

`psi(..., dtype=np.longdouble)` is the truth, `psi(..., dtype=np.float64)` the same operation sequence in float64: its distance from
the truth (e64) is what the device is allowed a multiple of.  `quadrature` is an independent check of the closed forms (a tensor
Gauss-Hermite rule over the input's density), exact only for l >= 0.5, s <= 0.3 at H = 100."""
import numpy as np

LD = np.longdouble
ROW_BLOCK = 8


def lengthscales(ls, D):
    return np.broadcast_to(np.asarray(ls, dtype=np.float64).reshape(-1), (D,)).copy()


def psi(mu, s, Z, variance, ls, dtype=LD, want_abs=False):
    """(psi0, psi1 (N, M), psi2 (M, M)) in `dtype`; s None = zeros.  want_abs: also absE (M, M) = max_n of the sum of the magnitudes
    of the terms of the psi2 exponent (the log-prefactor terms included)."""
    T = dtype
    mu, Z = np.asarray(mu, dtype=T), np.asarray(Z, dtype=T)
    N, D = mu.shape
    M = Z.shape[0]
    s = np.zeros((N, D), dtype=T) if s is None else np.asarray(s, dtype=T)
    v = T(variance)
    l2 = np.asarray(lengthscales(ls, D), dtype=T) ** 2
    psi0 = T(N) * v
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        a1 = l2 + s
        pre1 = np.sqrt(np.prod(l2 / a1, axis=1))
        d1 = mu[:, None, :] - Z[None, :, :]
        psi1 = v * pre1[:, None] * np.exp(T(-0.5) * np.sum(d1 * d1 / a1[:, None, :], axis=2))
        dz = Z[:, None, :] - Z[None, :, :]
        e0 = np.sum(dz * dz / (T(4) * l2), axis=2)
        psi2 = np.zeros((M, M), dtype=T)
        absE = np.zeros((M, M), dtype=np.float64)
        for a in range(0, N, ROW_BLOCK):
            b = min(a + ROW_BLOCK, N)
            a2 = l2 + T(2) * s[a:b]
            pre2 = v * v * np.sqrt(np.prod(l2 / a2, axis=1))
            dm = (d1[a:b, :, None, :] + d1[a:b, None, :, :]) / T(2)      # mu - (z_m + z_k) / 2 from differences: exact at an offset
            e1 = np.sum(dm * dm / a2[:, None, None, :], axis=3)
            psi2 = psi2 + np.sum(pre2[:, None, None] * np.exp(-(e0[None] + e1)), axis=0)
            if want_abs:
                lg = 0.5 * np.sum(np.abs(np.log(np.abs((l2 / a2).astype(np.float64)))), axis=1)
                tot = (np.abs(e0[None]) + np.sum(np.abs(dm * dm / a2[:, None, None, :]), axis=3)).astype(np.float64) + lg[:, None, None]
                absE = np.fmax(absE, np.max(tot, axis=0))
    return (psi0, psi1, psi2, absE) if want_abs else (psi0, psi1, psi2)


def quadrature(mu, s, Z, variance, ls, H=100):
    """psi1 and psi2 by a tensor Gauss-Hermite rule with H nodes per dimension (float64; D <= 2)."""
    mu, Z = np.asarray(mu, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    N, D = mu.shape
    assert D <= 2
    s = np.zeros((N, D)) if s is None else np.asarray(s, dtype=np.float64)
    l = lengthscales(ls, D)
    x, w = np.polynomial.hermite.hermgauss(H)
    w = w / np.sqrt(np.pi)
    if D == 1:
        G, W = x[:, None], w
    else:
        G = np.stack(np.meshgrid(x, x, indexing="ij"), -1).reshape(-1, 2)
        W = (w[:, None] * w[None, :]).reshape(-1)
    psi1, psi2 = np.zeros((N, Z.shape[0])), np.zeros((Z.shape[0], Z.shape[0]))
    for n in range(N):
        xs = mu[n] + np.sqrt(2.0 * s[n]) * G
        K = variance * np.exp(-0.5 * np.sum(((xs[:, None, :] - Z[None, :, :]) / l) ** 2, axis=2))
        psi1[n] = W @ K
        psi2 += np.einsum("q,qi,qj->ij", W, K, K)
    return psi1, psi2
