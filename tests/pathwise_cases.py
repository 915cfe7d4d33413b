"""The case table of the pathwise calls (tests/test_gpu_pathwise.py, tests/test_pathwise_plan_cpu.py): the smallest shapes at which
k_pw_eval can go wrong — rows, frequencies, inducing rows and outputs below, at and above a tile of 16, more than one workgroup (65 rows),
more than one frequency chunk of 32, Z tile of 64 and sweep of 32 outputs, ragged k-groups (D = 1, 3, 5, 9), more than one staged chunk of
16 input dimensions (D = 33, 100, 784), both X strides, every mean function — and the numerical edge cases.

(kind, ard, white_var, white, n, L, D, M, DO, S, per_draw, add, flags); flags:
  qnull      q_sqrt = NULL in the weights call
  offset     X and Z moved by 1e6
  theta_lo   lengthscale 1e-3, |theta| up to about 2.8e3: every argument below the switch at 4096 (PW_FAST_MAX)
  theta_hi   lengthscale 1e-3, |theta| up to about 1.6e5, a quarter of them below 4096: arguments on both sides of the switch
  far        row FAR_ROW is 1e3 lengthscales from every inducing row: every exponential of the row underflows
  nan        row NAN_ROW holds a NaN
"""
import functools

import numpy as np

from tests import pathwise_reference as PR

RBF, M52 = "rbf", "matern52"
FAR_ROW, NAN_ROW = 3, 5
JITTER = 1e-6

CASES = {
    "n1":      (RBF, False, None, False, 1, 1, 1, 0, 1, 1, False, None, ()),
    "n15":     (RBF, False, None, False, 15, 15, 3, 1, 3, 3, True, "identity", ()),
    "n16":     (M52, True, 0.3, True, 16, 16, 4, 17, 16, 1, False, "linear", ()),
    "n17":     (RBF, True, None, True, 17, 17, 5, 130, 17, 3, True, None, ()),
    "n65":     (M52, False, None, False, 65, 130, 9, 17, 1, 3, False, None, ()),
    "d33":     (RBF, False, 0.2, False, 65, 33, 33, 17, 35, 1, True, "linear", ()),
    "d100":    (M52, True, None, False, 17, 17, 100, 17, 3, 1, False, None, ()),
    "d784":    (RBF, False, None, False, 5, 16, 784, 17, 1, 1, False, None, ()),
    "qnull":   (RBF, False, None, True, 17, 33, 3, 17, 3, 3, False, None, ("qnull",)),
    "offset":  (RBF, True, None, False, 17, 33, 3, 17, 3, 1, False, "identity", ("offset",)),
    "theta_lo": (RBF, False, None, False, 17, 33, 1, 17, 1, 1, False, None, ("theta_lo",)),
    "theta_hi": (M52, False, None, False, 17, 33, 3, 17, 1, 3, True, None, ("theta_hi",)),
    "far":     (RBF, False, None, False, 17, 17, 3, 17, 3, 1, False, None, ("far",)),
    "nan":     (RBF, False, None, False, 17, 17, 3, 17, 3, 3, True, None, ("nan",)),
}
NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def inputs(name):
    kind, ard, wv, white, n, L, D, M, DO, S, per_draw, add, flags = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    tiny = "theta_lo" in flags or "theta_hi" in flags
    base = 1e-3 if tiny else (1.0 if D <= 2 else 0.6 * np.sqrt(D))
    ls = base * (1.0 + 0.3 * rng.random(D)) if ard else np.array([base])
    Mz = max(M, 1)
    if D <= 2:
        Z = 0.1 * rng.standard_normal((Mz, D))
        Z[:, 0] += 0.9 * np.arange(Mz)
    else:
        Z = 1.5 * rng.standard_normal((Mz, D))
    spread = 0.5 if "theta_lo" in flags else 10.0 if "theta_hi" in flags else 0.3
    if tiny:
        Z = Z * 1e-3                                     # inducing rows a lengthscale apart
    X = Z[rng.integers(0, Mz, size=(S if per_draw else 1, n))] + spread * rng.standard_normal((S if per_draw else 1, n, D))
    if "offset" in flags:
        X, Z = X + 1e6, Z + 1e6
    if "far" in flags:
        X[:, FAR_ROW] = Z[0] + 1e3 * base
    if "nan" in flags:
        X[:, NAN_ROW, D - 1] = np.nan
    X = X if per_draw else X[0]
    variance = 1.3
    Omega = PR.sample_basis(kind, D, L, ls, rng)
    Wc, Ws, eps = rng.standard_normal((S, L, DO)), rng.standard_normal((S, L, DO)), rng.standard_normal((S, Mz, DO))
    q_mu = rng.standard_normal((Mz, DO))
    q_sqrt = None if "qnull" in flags else np.tril(0.3 * rng.standard_normal((DO, Mz, Mz))) + 0.5 * np.eye(Mz)[None]
    A = b = addv = None
    if add == "identity":
        addv = X
    elif add == "linear":
        A, b = rng.standard_normal((D, DO)) / np.sqrt(D), rng.standard_normal(DO)
        addv = X @ A + b
    return dict(kind=kind, ard=ard, white_var=wv, white=white, n=n, L=L, D=D, M=M, DO=DO, S=S, per_draw=per_draw, add=add, flags=flags,
                ls=ls, Z=Z, X=X, origin=Z[0].copy(), variance=variance, Omega=Omega, Wc=Wc, Ws=Ws, eps=eps, q_mu=q_mu, q_sqrt=q_sqrt,
                A=A, b=b, addv=addv, jitter=JITTER)


@functools.lru_cache(maxsize=None)
def weights(name, dtype=PR.LD):
    """(v, mag) of the case's weights call; None for M = 0"""
    c = inputs(name)
    if c["M"] == 0:
        return None
    return PR.weights(c["kind"], c["Z"], c["Omega"], c["origin"], c["Wc"], c["Ws"], c["q_mu"], c["q_sqrt"],
                      None if c["q_sqrt"] is None else c["eps"], c["variance"], c["ls"], c["white_var"], c["jitter"], c["white"], dtype)


def eval_weights(name):
    """the V the evaluation cases are fed: the truth's, rounded to double (None for M = 0)"""
    w = weights(name)
    return None if w is None else np.ascontiguousarray(w[0], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def evaluate(name, dtype=PR.LD):
    """(f, mag) of the case's evaluation call at eval_weights(name); the NaN row's add is NaN with an Identity mean, as on the device"""
    c = inputs(name)
    return PR.evaluate(c["kind"], c["X"], c["Omega"], c["origin"], c["Wc"], c["Ws"], c["Z"], eval_weights(name), c["variance"], c["ls"],
                       c["addv"], dtype)


# ---- the moment-test configuration: one layer, RBF s2 = 1.3, l = 0.8, D = 2; Z a 4 x 4 grid of spacing 1 jittered by 0.1 (cond(Ku) about
# 40: the update does not amplify the basis error); n = 8 rows, L = 256 frequencies, T = S = 4096 draws, a dense lower q_sqrt
MOMENT_SEED = 4
MOMENT_T, MOMENT_L, MOMENT_N = 4096, 256, 8


@functools.lru_cache(maxsize=None)
def moment_config():
    rng = np.random.default_rng(2020)
    gx, gy = np.meshgrid(np.arange(4.0), np.arange(4.0))
    Z = np.stack([gx.ravel(), gy.ravel()], axis=1) + 0.1 * rng.standard_normal((16, 2))
    X = rng.uniform(-0.5, 3.5, size=(MOMENT_N, 2))
    q_mu = rng.standard_normal((16, 1))
    q_sqrt = (np.tril(0.2 * rng.standard_normal((16, 16))) + 0.5 * np.eye(16))[None]
    return dict(kind=RBF, variance=1.3, ls=np.array([0.8]), Z=Z, X=X, q_mu=q_mu, q_sqrt=q_sqrt, white_var=None, jitter=JITTER, white=False,
                origin=Z[0].copy())


def moment_ratios(F, Omega):
    """(worst mean ratio, worst covariance ratio) of the draws F (T, n) at the configuration's X against the exact moments given the
    basis Omega, in standard errors: sd / sqrt(T) for the mean, sqrt((C_ii C_jj + C_ij^2) / T) for the covariance"""
    c = moment_config()
    mean, cov = PR.moments_given_basis(c["kind"], c["X"], Omega, c["origin"], c["Z"], c["q_mu"], c["q_sqrt"], c["variance"], c["ls"],
                                       c["white_var"], c["jitter"], c["white"])
    mean, cov = mean[:, 0].astype(np.float64), cov[0].astype(np.float64)
    T = F.shape[0]
    sd = np.sqrt(np.diag(cov))
    rm = np.max(np.abs(F.mean(axis=0) - mean) / (sd / np.sqrt(T)))
    se = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / T)
    rc = np.max(np.abs(np.cov(F.T, bias=False) - cov) / se)
    return float(rm), float(rc)
