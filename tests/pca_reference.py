"""CPU reference of the device PCA (csrc/pca.hip; tests/test_pca_reference_cpu.py, tests/test_gpu_pca.py).  Two things:

truth(X, center): the Gram matrix C = Xc^T Xc in numpy longdouble (Xc = X, or X minus its longdouble column means), rounded to float64,
and np.linalg.eigh of it, eigenvalues non-increasing — "the truth" every figure is measured against.

jacobi(C): a float64 numpy version of the device's eigensolver — the same round-robin ordering (D padded to even; step s, pair m:
m = 0: (s, Dp - 1), m >= 1: (s + m, s - m) mod (Dp - 1)), the same skip rule |a_pq| <= 2^-53 sqrt(|a_pp a_qq|), the same rotation
(theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), sgn(0) = 1), the same mirroring of the blocks
(pair a, pair b <= a), the same stopping rule (after a sweep: off <= D 2^-52 |C|_F, off summed from the off-diagonal entries themselves,
or no rotation in the sweep) and the same ranking and sign rule.  Only the rounding of a step differs (numpy evaluates rows, then columns,
without fused multiply-adds).

R_ORTH, R_RES, R_LAM, R_PROJ: the worst ratios the numpy Jacobi reaches over the cases of tests/pca_cases.py it runs on (see
`ratios`); the device is held to 8 x these.  They are computed on first use."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


def truth(X, center):
    """dict: C (D, D) float64, lam (D,) non-increasing, U (D, D) columns to match, mean (D,) longdouble, Xc float64, normF"""
    Xl = np.asarray(X, dtype=np.float64).astype(LD)
    mean = Xl.mean(axis=0) if center else np.zeros(Xl.shape[1], dtype=LD)
    Xl = Xl - mean
    C = (Xl.T @ Xl).astype(np.float64)
    C = np.tril(C) + np.tril(C, -1).T
    lam, U = np.linalg.eigh(C)
    return {"C": C, "lam": lam[::-1].copy(), "U": U[:, ::-1].copy(), "mean": mean, "Xc": Xl.astype(np.float64),
            "normF": float(np.linalg.norm(C))}


def pairs(step, Dp):
    """(p, q), p < q: the Dp / 2 disjoint pairs of a step"""
    m = np.arange(1, Dp // 2)
    a, b = (step + m) % (Dp - 1), (step - m) % (Dp - 1)
    return np.concatenate([[step], np.minimum(a, b)]), np.concatenate([[Dp - 1], np.maximum(a, b)])


def rotations(app, aqq, apq):
    """(rotated?, t, c, s) of the pairs with these diagonal blocks"""
    rot = ~(np.abs(apq) <= 2.0 ** -53 * np.sqrt(np.abs(app * aqq)))
    theta = (aqq - app) / (2.0 * np.where(rot, apq, 1.0))
    t = np.where(rot, np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0)), 0.0)
    c = 1.0 / np.sqrt(t * t + 1.0)
    return rot, t, c, t * c


def jacobi(C, max_sweeps=30):
    """dict: lam (D,) non-increasing, V (D, D) columns to match with the device's sign rule, sweeps, converged, rotations (last sweep)"""
    D = C.shape[0]
    Dp = D + (D & 1)
    A = np.zeros((Dp, Dp))
    A[:D, :D] = C
    V = np.eye(Dp)
    normF = np.sqrt(np.sum(A * A))
    offdiag = ~np.eye(Dp, dtype=bool)
    pid = np.empty(Dp, dtype=np.int64)
    sweeps, converged, nrot = 0, False, 0
    while sweeps < max_sweeps and not converged:
        nrot = 0
        for step in range(Dp - 1):
            p, q = pairs(step, Dp)
            app, aqq, apq = A[p, p], A[q, q], A[p, q]
            rot, t, c, s = rotations(app, aqq, apq)
            nrot += int(rot.sum())
            Ap, Aq = A[p, :].copy(), A[q, :].copy()
            A[p, :], A[q, :] = c[:, None] * Ap - s[:, None] * Aq, s[:, None] * Ap + c[:, None] * Aq
            Ap, Aq = A[:, p].copy(), A[:, q].copy()
            A[:, p], A[:, q] = c * Ap - s * Aq, s * Ap + c * Aq
            # the block (pair a, pair b) is computed for b <= a and mirrored
            pid[p] = pid[q] = np.arange(Dp // 2)
            A = np.where(pid[:, None] >= pid[None, :], A, A.T)
            A[p, p] = np.where(rot, app - t * apq, app)
            A[q, q] = np.where(rot, aqq + t * apq, aqq)
            A[p, q] = A[q, p] = np.where(rot, 0.0, apq)
            Vp, Vq = V[:, p].copy(), V[:, q].copy()
            V[:, p], V[:, q] = c * Vp - s * Vq, s * Vp + c * Vq
        sweeps += 1
        off = np.sqrt(np.sum(A[offdiag] ** 2))
        converged = bool(off <= D * EPS * normF or nrot == 0)
    d = np.diag(A)[:D]
    rank = np.array([np.sum((d > d[i]) | ((d == d[i]) & (np.arange(D) < i))) for i in range(D)])
    order = np.empty(D, dtype=np.int64)
    order[rank] = np.arange(D)
    Vs = V[:D][:, order]
    top = np.argmax(np.abs(Vs), axis=0)          # the first of equal maxima: the lowest row
    Vs = Vs * np.where(Vs[top, np.arange(D)] < 0.0, -1.0, 1.0)
    return {"lam": d[order], "V": Vs, "sweeps": sweeps, "converged": converged, "rotations": nrot}


def figures(tr, lam, V):
    """(r_orth, r_res, r_lam) of the eigenpairs (lam[j], V[:, j]), j < V.shape[1], against the truth `tr`: 1 = D 2^-52 (|C|_F)"""
    D = tr["C"].shape[0]
    k = V.shape[1]
    unit = D * EPS
    scale = unit * tr["normF"] if tr["normF"] > 0 else unit
    r_orth = float(np.max(np.abs(V.T @ V - np.eye(k)))) / unit
    r_res = float(np.max(np.linalg.norm(tr["C"] @ V - V * lam[:k], axis=0))) / scale
    r_lam = float(np.max(np.abs(lam - tr["lam"][:lam.shape[0]]))) / scale
    return r_orth, r_res, r_lam


def projector_figure(tr, V, k):
    """|V_k V_k^T - U_k U_k^T|_2 over D 2^-52 |C|_F / (lam_k - lam_{k+1}), for k < D"""
    D = tr["C"].shape[0]
    gap = tr["lam"][k - 1] - tr["lam"][k]
    P, Pt = V[:, :k] @ V[:, :k].T, tr["U"][:, :k] @ tr["U"][:, :k].T
    return float(np.linalg.norm(P - Pt, 2)) / (D * EPS * tr["normF"] / gap)


_RATIOS = None


def ratios():
    """{"R_ORTH", "R_RES", "R_LAM", "R_PROJ"}: the worst figures of the numpy Jacobi over the cases it runs on (R_PROJ: the gapped ones)"""
    global _RATIOS
    if _RATIOS is None:
        from tests import pca_cases as PC
        figs = [figures(PC.truth(n), PC.jacobi(n)["lam"], PC.jacobi(n)["V"]) for n in PC.JACOBI_NAMES]
        proj = [projector_figure(PC.truth(n), PC.jacobi(n)["V"], PC.CASES[n][2]) for n in PC.JACOBI_NAMES if PC.gapped(n)]
        _RATIOS = {"R_ORTH": max(f[0] for f in figs), "R_RES": max(f[1] for f in figs), "R_LAM": max(f[2] for f in figs),
                   "R_PROJ": max(proj)}
    return _RATIOS


def __getattr__(name):
    if name in ("R_ORTH", "R_RES", "R_LAM", "R_PROJ"):
        return ratios()[name]
    raise AttributeError(name)
