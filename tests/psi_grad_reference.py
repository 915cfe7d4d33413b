"""The yardstick of the tests of the reverse pass of the kernel expectations (tests/test_psi_grad_reference_cpu.py,
tests/test_gpu_psi_grad.py, tests/test_gpu_collapsed_grad.py): the adjoints of mu, s, Z, the kernel variance and the lengthscales given
the adjoints g_psi0, g_psi1, g_psi2 of the statistics of tests/psi_reference.psi, formula by formula in the direct form, and the adjoints
of the collapsed bound of tests/collapsed_reference.collapsed.  dtype=np.longdouble is the truth, dtype=np.float64 the same operation
sequence in float64: its distance from the truth (e64) is what the device is allowed a multiple of.  Next to every output entry stands
`mag`, the sum of the magnitudes of the terms that are added into it (down to the single pair: |Q_rij| |delta| ..., not |q_ri| |delta|):
the unit in which an error of that entry is measured.

Notation (csrc/psi_grad.hip): l2 = l^2, w1 = 1 / (l2 + s), w2 = 1 / (l2 + 2 s), t = (w2 - 1 / l2) / 4, delta_rid = mu_rd - z_id,
Delta_ijd = z_id - z_jd, A_ri = g_psi1_ri psi1_ri, Gs = (g_psi2 + g_psi2^T) / 2, Q_rij = Gs_ij v^2 exp(E_rij)."""
import numpy as np

from tests import collapsed_reference as CR
from tests import psi_reference as P

LD = np.longdouble
ROW_BLOCK = 8
KEYS = ("X_mean", "X_var", "Z", "variance", "lengthscales")


def psi_grad(mu, s, Z, variance, ls, ard, g_psi0, g_psi1, g_psi2, dtype=LD):
    """(grad, mag): dicts over KEYS; X_mean, X_var (N, D), Z (M, D), variance (), lengthscales (D,) with ard, else (1,).  g_psi1 (N, M)
    or None, g_psi2 (M, M) or None; s None = zeros (X_var is then the derivative at s = 0)."""
    T = dtype
    mu, Z = np.asarray(mu, dtype=T), np.asarray(Z, dtype=T)
    N, D = mu.shape
    M = Z.shape[0]
    s = np.zeros((N, D), dtype=T) if s is None else np.asarray(s, dtype=T)
    v = T(variance)
    l = np.asarray(P.lengthscales(ls, D), dtype=T)
    l2 = l * l
    zero = lambda *shape: np.zeros(shape, dtype=T)
    d_mu, m_mu, d_s, m_s, d_Z, m_Z, d_l2, m_l2 = (zero(N, D), zero(N, D), zero(N, D), zero(N, D), zero(M, D), zero(M, D), zero(D), zero(D))
    d_v, m_v = T(N) * T(g_psi0), T(N) * abs(T(g_psi0))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        d1 = mu[:, None, :] - Z[None, :, :]                                      # delta (N, M, D)
        if g_psi1 is not None:
            w1 = T(1) / (l2 + s)
            pre1 = np.sqrt(np.prod(l2 * w1, axis=1))
            psi1 = v * pre1[:, None] * np.exp(T(-0.5) * np.sum(d1 * d1 * w1[:, None, :], axis=2))
            A = np.asarray(g_psi1, dtype=T) * psi1
            aA = np.abs(A)
            a1, ab1 = np.sum(A, axis=1), np.sum(aA, axis=1)
            d_mu += -w1 * np.sum(A[:, :, None] * d1, axis=1)
            m_mu += np.abs(w1) * np.sum(aA[:, :, None] * np.abs(d1), axis=1)
            d_Z += np.sum(A[:, :, None] * w1[:, None, :] * d1, axis=0)
            m_Z += np.sum(aA[:, :, None] * np.abs(w1[:, None, :] * d1), axis=0)
            dW1 = a1[:, None] / (T(2) * w1) - T(0.5) * np.sum(A[:, :, None] * d1 * d1, axis=1)
            mW1 = ab1[:, None] / np.abs(T(2) * w1) + T(0.5) * np.sum(aA[:, :, None] * d1 * d1, axis=1)
            d_s += -w1 * w1 * dW1
            m_s += w1 * w1 * mW1
            d_l2 += np.sum(-w1 * w1 * dW1 + a1[:, None] / (T(2) * l2), axis=0)
            m_l2 += np.sum(w1 * w1 * mW1 + ab1[:, None] / (T(2) * l2), axis=0)
            d_v += np.sum(A) / v
            m_v += np.sum(aA) / v
        if g_psi2 is not None:
            g2 = np.asarray(g_psi2, dtype=T)
            Gs = (g2 + g2.T) / T(2)
            dz = Z[:, None, :] - Z[None, :, :]                                   # Delta (M, M, D)
            dz2 = dz * dz
            e0 = np.sum(dz2 / (T(4) * l2), axis=2)
            R, aR = zero(M, M, D), zero(M, M, D)
            for a in range(0, N, ROW_BLOCK):
                b = min(a + ROW_BLOCK, N)
                sb, db = s[a:b], d1[a:b]
                a2 = l2 + T(2) * sb
                w2 = T(1) / a2
                t = (w2 - T(1) / l2) / T(4)
                pre2 = v * v * np.sqrt(np.prod(l2 / a2, axis=1))
                dm = (db[:, :, None, :] + db[:, None, :, :]) / T(2)
                e1 = np.sum(dm * dm / a2[:, None, None, :], axis=3)
                Q = Gs[None] * (pre2[:, None, None] * np.exp(-(e0[None] + e1)))  # (B, M, M)
                aQ = np.abs(Q)
                q, aq = np.sum(Q, axis=2), np.sum(aQ, axis=2)
                ar, aar = np.sum(q, axis=1), np.sum(aq, axis=1)
                Pm = np.einsum("rij,ijd->rd", Q, dz2)
                aP = np.einsum("rij,ijd->rd", aQ, dz2)
                R += np.einsum("rij,rd->ijd", Q, t)
                aR += np.einsum("rij,rd->ijd", aQ, np.abs(t))
                d_mu[a:b] += T(-2) * w2 * np.sum(q[:, :, None] * db, axis=1)
                m_mu[a:b] += T(2) * np.abs(w2) * np.sum(aq[:, :, None] * np.abs(db), axis=1)
                d_Z += T(2) * np.sum(q[:, :, None] * w2[:, None, :] * db, axis=0)
                m_Z += T(2) * np.sum(aq[:, :, None] * np.abs(w2[:, None, :] * db), axis=0)
                dW2 = ar[:, None] / (T(2) * w2) - np.sum(q[:, :, None] * db * db, axis=1) + Pm / T(4)
                mW2 = aar[:, None] / np.abs(T(2) * w2) + np.sum(aq[:, :, None] * db * db, axis=1) + aP / T(4)
                d_s[a:b] += T(-2) * w2 * w2 * dW2
                m_s[a:b] += T(2) * w2 * w2 * mW2
                d_l2 += np.sum(-w2 * w2 * dW2 + ar[:, None] / (T(2) * l2) + Pm / (T(4) * l2 * l2), axis=0)
                m_l2 += np.sum(w2 * w2 * mW2 + aar[:, None] / (T(2) * l2) + aP / (T(4) * l2 * l2), axis=0)
                d_v += T(2) * np.sum(ar) / v
                m_v += T(2) * np.sum(aar) / v
            d_Z += T(4) * np.sum(dz * R, axis=1)
            m_Z += T(4) * np.sum(np.abs(dz) * aR, axis=1)
        d_l, m_l = T(2) * l * d_l2, T(2) * l * m_l2
        if not ard:
            d_l, m_l = np.sum(d_l, keepdims=True), np.sum(m_l, keepdims=True)
    grad = dict(X_mean=d_mu, X_var=d_s, Z=d_Z, variance=d_v, lengthscales=d_l)
    mag = dict(X_mean=m_mu, X_var=m_s, Z=m_Z, variance=m_v, lengthscales=m_l)
    return grad, mag


# ---------------------------------------------------------------------------------------------------------------- the collapsed bound
def _inverse(L, dtype):
    """(L L^T)^-1 from the written-out solves of tests/collapsed_reference.py"""
    Li = CR.solve_lower(L, np.eye(L.shape[0], dtype=dtype))
    return Li.T @ Li


def bound_adjoints(Kuu, psi0, psi1, psi2, Y, noise_var, dtype=LD):
    """The adjoints of the collapsed bound F(Kuu, psi0, psi1, psi2, s2) of collapsed_reference.collapsed_from, by the closed forms with
    Sigma = Kuu + psi2 / s2, alpha = Sigma^-1 psi1^T Y / s2:  dict(bound, g_psi0, g_psi1, g_psi2, d_Kuu, d_s2, mag_s2)."""
    T = dtype
    Kuu, psi1, psi2, Y = (np.asarray(a, dtype=T) for a in (Kuu, psi1, psi2, Y))
    psi0, s2 = T(psi0), T(noise_var)
    N, DY = Y.shape
    st = CR.collapsed_from(Kuu, psi0, psi1, psi2, Y, noise_var, dtype=T)
    Sigma = Kuu + psi2 / s2
    Si = _inverse(CR.chol(Sigma), T)
    Ki = _inverse(st["L"], T)
    b = psi1.T @ Y
    alpha = Si @ b / s2
    half, dy = T(0.5), T(DY)
    dSigma = -half * dy * Si - half * alpha @ alpha.T
    g_psi0 = -half * dy / s2
    g_psi1 = Y @ alpha.T / s2
    g_psi2 = dSigma / s2 + half * dy * Ki / s2
    KpK = Ki @ psi2 @ Ki
    d_Kuu = dSigma + half * dy * Ki - half * dy * KpK / s2
    terms = np.array([-half * T(N) * dy / s2, half * np.sum(Y * Y) / (s2 * s2), -np.sum(b * (Si @ b)) / (s2 * s2 * s2),
                      half * dy * psi0 / (s2 * s2), -half * dy * np.sum(Ki * psi2) / (s2 * s2), -np.sum(dSigma * psi2) / (s2 * s2)], dtype=T)
    return dict(bound=st["bound"], g_psi0=g_psi0, g_psi1=g_psi1, g_psi2=g_psi2, d_Kuu=d_Kuu, d_s2=np.sum(terms),
                mag_s2=np.sum(np.abs(terms)))


GRAD_KEYS = ("Z", "variance", "lengthscales", "lik_variance", "X_mean", "X_var")


def collapsed_grad(mu, s, Z, variance, ls, ard, Y, noise_var, jitter, dtype=LD):
    """(bound, grad, mag) of the collapsed bound of collapsed_reference.collapsed with respect to Z, the kernel variance, the
    lengthscales, the noise variance and the inputs' means and variances (dicts over GRAD_KEYS).  Kuu = K(Z, Z) + jitter I reaches Z and
    the kernel as psi1 at mu = Z, s = None with g_psi1 = d_Kuu: both of its input adjoints belong to Z."""
    T = dtype
    psi0, psi1, psi2 = P.psi(mu, s, Z, variance, ls, dtype=T)
    M = np.asarray(Z).shape[0]
    Kuu = CR.rbf(Z, Z, variance, ls, T) + T(jitter) * np.eye(M, dtype=T)
    adj = bound_adjoints(Kuu, psi0, psi1, psi2, Y, noise_var, dtype=T)
    g1, m1 = psi_grad(mu, s, Z, variance, ls, ard, adj["g_psi0"], adj["g_psi1"], adj["g_psi2"], dtype=T)
    g2, m2 = psi_grad(Z, None, Z, variance, ls, ard, 0.0, adj["d_Kuu"], None, dtype=T)
    grad = dict(Z=g1["Z"] + (g2["Z"] + g2["X_mean"]), variance=g1["variance"] + g2["variance"],
                lengthscales=g1["lengthscales"] + g2["lengthscales"], lik_variance=adj["d_s2"], X_mean=g1["X_mean"], X_var=g1["X_var"])
    mag = dict(Z=m1["Z"] + (m2["Z"] + m2["X_mean"]), variance=m1["variance"] + m2["variance"],
               lengthscales=m1["lengthscales"] + m2["lengthscales"], lik_variance=adj["mag_s2"], X_mean=m1["X_mean"], X_var=m1["X_var"])
    return adj["bound"], grad, mag


def exact_gp_grad(X, Y, variance, ls, noise_var, dtype=LD):
    """(log marginal likelihood, its gradient in (variance, one shared lengthscale, noise variance)) of exact GP regression with an RBF
    kernel, written out: dL/dK = 1/2 (a a^T - D_Y K^-1), a = K^-1 Y."""
    T = dtype
    X, Y = np.asarray(X, dtype=T), np.asarray(Y, dtype=T)
    N, DY = Y.shape
    l = T(np.asarray(ls, dtype=np.float64).reshape(-1)[0])
    Kf = CR.rbf(X, X, variance, np.array([float(l)]), T)
    Lk = CR.chol(Kf + T(noise_var) * np.eye(N, dtype=T))
    Ki = _inverse(Lk, T)
    a = Ki @ Y
    two_pi = T(2) * (np.pi if T is np.float64 else LD("3.14159265358979323846264338327950288"))
    lml = T(-0.5) * np.sum(Y * a) - T(DY) * np.sum(np.log(np.diag(Lk))) - T(0.5) * T(N * DY) * np.log(two_pi)
    dK = T(0.5) * (a @ a.T - T(DY) * Ki)
    d = X[:, None, :] - X[None, :, :]
    r2 = np.sum(d * d, axis=2)
    return lml, dict(variance=np.sum(dK * Kf) / T(variance), lengthscales=np.sum(dK * Kf * r2) / (l * l * l), lik_variance=np.trace(dK))
