"""References of the joint-shift tests: what float64 itself loses when X and Z move away from the origin, and a long-double
kernel matrix with entrywise bars for dsdgp_gram.  numpy / torch float64 and numpy long double only, no GPU.

THE FAMILY (model level).  oracle.model.elbo_and_grad / propagate with the distance form the device documents (spec["sqdist"] =
"clamped": |x|^2 + |z|^2 - 2 x.z on x / l, clamped at 0, exactly 0 on the diagonal of K(Z, Z)), evaluated at c = 0 and at c times the
four sign patterns of tests/shift_cases.py.  The inputs are on a dyadic grid, so all five are the SAME problem in exact arithmetic and
the differences are rounding alone, each sign pattern an independent realisation of it at the same magnitude.  For a quantity q (the
ELBO, a gradient block, a layer's Fmean - shift, a layer's Fvar), in units of q's largest magnitude at c = 0,

    family(q) = max over the four patterns of max |oracle(c s)(q) - oracle(0)(q)|
    bar(q)    = 8 max(family(q), 2^-40)

8 is this suite's rule for a different but fixed summation order (tests/test_gpu_natgrad_direct.py); 2^-40 ~ 1e-12 is the tolerance the
suite already uses between two summation orders of one gradient (tests/test_gpu_round4.py, tests/test_gpu_round3_tail.py).  The device
is compared with ITS OWN result at c = 0, which the rest of the suite holds to the oracle: a site of the device that loses more than
the expansion itself must shows up as a ratio above 1.  sqdist = "direct" gives the same table for direct differences; it is
recorded beside the other (how much of the movement the form itself costs), never a bar.

THE KERNEL MATRIX (dsdgp_gram).  kernel_ld: direct differences of x / l in long double (u_ld = 2^-64), both kinds, Matern52 with the
1e-12 under its root.  With u = 2^-53, xh = x / l, S = |xh|^2 + |zh|^2, r^2 the exact scaled squared distance and k = f(r^2):

 * expanded form (k_gram_mfma2 / k_gram_mfma3, D <= 32).  A scaled coordinate x (1 / l) carries two roundings, of which the
   reciprocal's is common to x and z (a perturbation of l: 2 u r^2 on r^2); each norm is a D-term FMA chain: (D + 2) u |xh|^2; the dot
   product's D-term accumulation and its operands' roundings: (D + 2) u sum |xh_d zh_d| <= (D + 2) u S / 2, doubled in -2 G; the two
   final additions: u S + u r^2.  First order, every rounding adverse: (2 D + 5) u S + 3 u r^2, which is at most (2 D + 8) u S =
   (D + 4) 2^-52 S whenever r^2 <= S, i.e. x.z >= 0 — every shifted pair and every pair close enough to matter; on the other pairs
   (centred inputs only) the worst case exceeds it by the factor 1 + 3 / (2 D + 8) at most and the typical error is ~ sqrt(D) u S.
   This is the bound of tests/test_gpu_greedy.py.  The kernel value moves by at most sup |dk / dr^2| times that: v / 2 (RBF),
   5 v / 6 (Matern52, at r = 0):        bar_expanded = (D + 4) 2^-52 S sup|dk/dr^2| + 4 ulp(k)
   Far pairs: that product is an absolute 1e-12 v beside a k of 1e-300 v and would hold nothing.  |dk / dr^2| decreases with r^2 for
   both kinds, so with e = (D + 4) 2^-52 S [+ 6 u r^2 for Matern52's exponent, see below] the value moves by at most
   e |dk/dr^2|(max(r^2 - e, 0)); the bar is the SMALLER of the two products, never above the line above.
 * direct form (k_gram, D > 32).  Each scaled coordinate is off by u |xh_d| (beside the common reciprocal), a difference by
   u (|xh_d| + |zh_d|) + u |d_d|, so r^2 = sum d_d^2 by 2 u sum |d_d| (|xh_d| + |zh_d|) <= 2 u r (|xh| + |zh|) (Cauchy-Schwarz) plus
   (D + 5) u r^2 for the squares' sum, the differences' own roundings and the reciprocal: the loss is eps |x / l| r, not eps |x / l|^2.
   Matern52 evaluates exp(-sqrt 5 rho) with rho = sqrt(r^2 + 1e-12) rounded, times a rounded constant: 3 u on the exponent is 6 u r^2
   more.  |dk / dr^2| decreases with r^2 for both kinds, so over the interval it is at most its value at max(r^2 - e, 0):
        e = 2^-52 r (|xh| + |zh|) + (D + 5 [+ 6]) 2^-53 r^2,   bar_direct = e |dk/dr^2|(max(r^2 - e, 0)) + 4 ulp(k)
   The bar is claimed where k_gram runs, D > 32: a first-order worst case with every rounding of a pair aligned is nearly reached
   when the sum has three terms (numpy: 0.55 of it at D = 3), and no honest term of the derivation supplies a factor two there.
 * 4 ulp(k) (np.spacing, so that it stays one denormal step where exp underflows) covers exp, sqrt and the polynomial's few products.

tests/test_shift_reference_cpu.py holds a float64 numpy version of each form to HALF its bar on every entry of every input family at
the widths where dsdgp_gram takes that form (expanded: D <= 32, direct: D > 32), and the expanded bar to at most 1e-6 v, so a pass on
the device says something."""
import functools
import math

import numpy as np

from oracle import model as OM
from tests import shift_cases as SC

LD = np.longdouble
FLOOR = 2.0 ** -40
RULE = 8.0


# ------------------------------------------------------------------------------------------------ the model-level family
def quantities(spec, state, X, Y, zs, S, num_data, shift, L):
    """ELBO, gradient blocks, Fmean - shift (inner layers) and Fvar of one oracle evaluation, as a flat dict of arrays."""
    e, g = OM.elbo_and_grad(spec, state, X, Y, zs, S, num_data=num_data)
    _, Fm, Fv = OM.propagate(spec, state, X, zs, S)
    q = {"elbo": np.array([e])}
    for k in sorted(g):
        q["grad " + k] = g[k]
    for l in range(L):
        q[f"Fmean l{l}"] = Fm[l] - shift if l < L - 1 else Fm[l]
        q[f"Fvar l{l}"] = Fv[l]
    return q


@functools.lru_cache(maxsize=None)
def _evaluate(name, c, pattern, sqdist):
    cs = SC.CASES[name]
    spec, state, _, Xs, arr, sh = SC.build(name, c, pattern)
    spec = dict(spec, sqdist=sqdist)
    return quantities(spec, state, Xs, arr["Y"], arr["zs"], cs["S"], 4 * cs["N"], sh, cs["L"])


def scales(q0):
    return {k: float(np.max(np.abs(v))) + 1e-300 for k, v in q0.items()}


def moved(q, q0, sc):
    """max |q - q0| per quantity in units of the quantity's largest magnitude at c = 0."""
    return {k: float(np.max(np.abs(np.asarray(q[k]) - q0[k]))) / sc[k] for k in q0}


@functools.lru_cache(maxsize=None)
def family(name, c, sqdist="clamped"):
    """-> (members, fam): members[p][q] the movement of quantity q under sign pattern p, fam[q] the largest of the four."""
    q0 = _evaluate(name, 0.0, 0, sqdist)
    sc = scales(q0)
    members = [moved(_evaluate(name, float(c), p, sqdist), q0, sc) for p in range(4)]
    return members, {k: max(m[k] for m in members) for k in q0}


def bars(name, c):
    """bar(q) = 8 max(family(q), 2^-40), relative to the quantity's largest magnitude at c = 0."""
    return {k: RULE * max(v, FLOOR) for k, v in family(name, c)[1].items()}


# ------------------------------------------------------------------------------------------------ the kernel matrix
def kfun(kind, v, r2):
    """k(r^2) in r2's own precision (the double 1e-12 under Matern52's root, as on the device)."""
    T = r2.dtype.type
    if kind == "rbf":
        return T(v) * np.exp(T(-0.5) * r2)
    r = np.sqrt(r2 + T(1e-12))
    s5 = np.sqrt(T(5.0))
    return T(v) * (T(1.0) + s5 * r + T(5.0) / T(3.0) * (r * r)) * np.exp(-s5 * r)


def _dk_dr2(kind, v, r2):
    """|dk / dr^2| in long double."""
    if kind == "rbf":
        return 0.5 * v * np.exp(-0.5 * r2)
    s5 = np.sqrt(LD(5.0))
    r = np.sqrt(r2 + LD(1e-12))
    return LD(5.0) / LD(6.0) * v * (1.0 + s5 * r) * np.exp(-s5 * r)


def _sup_dk(kind, v):
    return 0.5 * v if kind == "rbf" else 5.0 * v / 6.0


def _r2_ld(X, X2, ls):
    xs, zs = X.astype(LD) / ls.astype(LD), X2.astype(LD) / ls.astype(LD)
    r2 = np.zeros((X.shape[0], X2.shape[0]), dtype=LD)
    for d in range(X.shape[1]):
        diff = xs[:, d][:, None] - zs[:, d][None, :]
        r2 += diff * diff
    return r2, xs, zs


def kernel_ld(kind, X, X2, ls, v):
    """K(X, X2) by direct differences in long double (no White, no jitter)."""
    r2, _, _ = _r2_ld(X, X2, ls)
    return kfun(kind, LD(v), r2)


def gram_bars(kind, X, X2, ls, v):
    """-> (K_ld, bar_expanded, bar_direct), entrywise (see the module docstring; bar_direct is claimed for D > 32 only)."""
    D = X.shape[1]
    r2, xs, zs = _r2_ld(X, X2, ls)
    K = kfun(kind, LD(v), r2)
    nx, nz = (xs * xs).sum(1), (zs * zs).sum(1)
    S = nx[:, None] + nz[None, :]
    ulp = 4.0 * np.spacing(np.abs(K.astype(np.float64)))
    m52 = LD((6 if kind == "matern52" else 0) * 2.0 ** -53) * r2
    ee = LD((D + 4) * 2.0 ** -52) * S
    bar_e = np.minimum(ee * LD(_sup_dk(kind, v)), (ee + m52) * _dk_dr2(kind, LD(v), np.maximum(r2 - ee - m52, LD(0.0)))).astype(np.float64) + ulp
    r = np.sqrt(r2)
    e = LD(2.0 ** -52) * r * (np.sqrt(nx)[:, None] + np.sqrt(nz)[None, :]) + LD((D + 5) * 2.0 ** -53) * r2 + m52
    bar_d = (e * _dk_dr2(kind, LD(v), np.maximum(r2 - e, LD(0.0)))).astype(np.float64) + ulp
    return K, bar_e, bar_d


def gram_expanded_f64(kind, X, X2, ls, v):
    """The clamped expansion in plain float64 numpy (what the device's MFMA forms compute, in numpy's order)."""
    xs, zs = X / ls, X2 / ls
    r2 = np.maximum((xs * xs).sum(1)[:, None] + (zs * zs).sum(1)[None, :] - 2.0 * (xs @ zs.T), 0.0)
    return kfun(kind, v, r2)


def gram_direct_f64(kind, X, X2, ls, v):
    """Direct differences of x (1 / l) in plain float64 numpy (k_gram's form)."""
    il = 1.0 / ls
    xs, zs = X * il, X2 * il
    r2 = np.zeros((X.shape[0], X2.shape[0]))
    for d in range(X.shape[1]):
        diff = xs[:, d][:, None] - zs[:, d][None, :]
        r2 += diff * diff
    return kfun(kind, v, r2)


# ------------------------------------------------------------------------------------------------ dsdgp_gram's input families
GRAM_N, GRAM_N2 = 37, 131
GRAM_DIMS = (3, 8, 20, 32, 33, 70)
GRAM_KINDS = ("rbf", "matern52")
GRAM_FAMILIES = ("centred", "shift6", "shift10", "coincide", "ard_spread", "far")
GRAM_V = 1.3


@functools.lru_cache(maxsize=None)
def gram_inputs(fam, D):
    """-> (X (37, D), X2 (131, D), ls (D,)).
    centred / shift6 / shift10: coordinates of standard deviation 1.2 / sqrt(D), lengthscales 0.7 .. 1.3, offset 0 / 2^6 / 2^10 with
      the second sign pattern; coincide: the centred inputs at offset 2^6 with X2[:37] = X bit for bit and X2[37:74] = X + 2^-24;
    ard_spread: lengthscales 2^-5 .. 2^5, coordinates scaled by them, no offset (an offset over l = 2^-5 is a scaled norm of 2^30 and a
      bar near v: the offset families keep moderate lengthscales so that every expanded bar stays below 1e-6 v);
    far: column j of X2 at scaled squared distance 1400 + 120 j / 130 (to within the rows' own spread, 0.01 per coordinate) from every
      row of X: exp's result goes through the denormals (RBF: k = v exp(-700 .. -760)) and to zero."""
    rng = np.random.RandomState(300 + D)
    n, n2 = GRAM_N, GRAM_N2
    sd = 1.2 / math.sqrt(D)
    ls = 0.7 + 0.6 * rng.rand(D)
    X, X2 = sd * rng.randn(n, D), sd * rng.randn(n2, D)
    if fam in ("shift6", "shift10", "coincide"):
        off = (2.0 ** 10 if fam == "shift10" else 2.0 ** 6) * SC.signs(D)[1]
        X, X2 = X + off, X2 + off
        if fam == "coincide":
            X2[:n] = X
            X2[n:2 * n] = X + 2.0 ** -24
    elif fam == "ard_spread":
        ls = 2.0 ** np.linspace(-5.0, 5.0, D)
        X, X2 = X * ls, X2 * ls
    elif fam == "far":
        X = 0.01 * rng.randn(n, D) * ls
        u = rng.randn(n2, D)
        u /= np.linalg.norm(u, axis=1)[:, None]
        X2 = u * np.sqrt(1400.0 + 120.0 * np.arange(n2) / (n2 - 1.0))[:, None] * ls
    elif fam != "centred":
        raise ValueError(fam)
    return np.ascontiguousarray(X), np.ascontiguousarray(X2), ls
