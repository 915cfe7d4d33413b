"""CPU side of tests/test_gpu_calibration.py: quantiles, probability integral transform and CRPS of an equally weighted mixture of S
Gaussians (the predictive distribution of dgp.py:116-126) in float64 numpy / scipy, and the mixture's distribution function and density
in 40-digit mpmath.  No product kernel is involved; tests/test_calibration_reference_cpu.py pins these functions against quadrature and
against direct draws from the mixture.

Components: mu, sg of shape (S, ...) — means and standard deviations, sg = sqrt(max(var + noise, DBL_MIN)).
  Phi(z) = erfc(-z / sqrt 2) / 2 ;  F(x) = mean_s Phi((x - mu_s) / sg_s) ;  f = F'
  quantile q_k: F(q_k) = p_k ;  PIT u = F(y)
  CRPS = mean_s A(y - mu_s, sg_s^2) - (1 / (2 S^2)) sum_s sum_t A(mu_s - mu_t, sg_s^2 + sg_t^2)        (Grimit et al. 2006)
  A(m, s^2) = m (2 Phi(m/s) - 1) + 2 s phi(m/s)
rows = (N, D, 2) of [u, CRPS]; sums = (2 + P, D): [sum_i CRPS, N, #(u <= p_0), ...] per output."""
import mpmath
import numpy as np
from scipy.special import erf, erfc, ndtri

EPS = np.finfo(np.float64).eps
TINY = np.finfo(np.float64).tiny
MAXIT = 128


def sigma(var, noise=0.0):
    return np.sqrt(np.maximum(np.asarray(var, dtype=np.float64) + noise, TINY))


def cdf(x, mu, sg):
    """F(x), x of the components' trailing shape"""
    z = (np.asarray(x)[None] - mu) / sg
    return (0.5 * erfc(-z / np.sqrt(2.0))).mean(0)


def pdf(x, mu, sg):
    z = (np.asarray(x)[None] - mu) / sg
    return (np.exp(-0.5 * z * z) / (np.sqrt(2.0 * np.pi) * sg)).mean(0)


def quantile(mu, sg, p):
    """The root of F(q) = p for every item (trailing shape of mu): Newton steps kept inside a bracket that holds the root,
    [min_s (mu_s + z sg_s), max_s (mu_s + z sg_s)] with z = Phi^-1(p) slightly widened — at its lower end every component's argument
    is <= z, hence F <= p; bisection whenever a step leaves the bracket or fails to halve the previous one; stops when the bracket
    cannot shrink or the step falls below the spacing of q; at most MAXIT steps, then the bracket's midpoint."""
    z = ndtri(p)
    w = 1e-9 * (1.0 + abs(z))
    lo, hi = (mu + (z - w) * sg).min(0), (mu + (z + w) * sg).max(0)
    x = lo + 0.5 * (hi - lo)
    res = x.copy()
    dxold = hi - lo
    glo, ghi = np.full(x.shape, -np.inf), np.full(x.shape, np.inf)
    done = ~(lo < hi)
    with np.errstate(all="ignore"):
        for _ in range(MAXIT):
            if done.all():
                break
            g = cdf(x, mu, sg) - p
            f = pdf(x, mu, sg)
            act = ~done
            hit = act & (g == 0.0)
            res = np.where(hit, x, res)
            done = done | hit
            act = act & ~hit
            neg = act & (g < 0.0)
            pos = act & (g > 0.0)
            lo, glo = np.where(neg, x, lo), np.where(neg, g, glo)
            hi, ghi = np.where(pos, x, hi), np.where(pos, g, ghi)
            mid = lo + 0.5 * (hi - lo)
            dx = g / f
            xn = x - dx
            bis = ~((xn > lo) & (xn < hi)) | (np.abs(2.0 * g) > np.abs(dxold * f))
            xn = np.where(bis, mid, xn)
            dxold = np.where(act, np.where(bis, 0.5 * (hi - lo), np.abs(dx)), dxold)
            stuck = act & bis & ~((mid > lo) & (mid < hi))
            res = np.where(stuck, np.where(-glo <= ghi, lo, hi), res)
            small = act & ~stuck & (xn == x)
            res = np.where(small, x, res)
            go = act & ~stuck & ~small
            res = np.where(go, mid, res)
            x = np.where(go, xn, x)
            done = done | stuck | small
    return res


def quantiles(mu, sg, probs):
    """(..., P)"""
    return np.stack([quantile(mu, sg, float(p)) for p in probs], axis=-1)


def pit(y, mu, sg):
    return cdf(y, mu, sg)


def _A(m, s):
    z = m / s
    return m * erf(z / np.sqrt(2.0)) + s * np.sqrt(2.0 / np.pi) * np.exp(-0.5 * z * z)


def crps(y, mu, sg):
    """closed form; the pair sum over s < t once, doubled, plus the diagonal A(0, 2 sg^2) = 2 sg / sqrt(pi)"""
    S = mu.shape[0]
    first = _A(np.asarray(y)[None] - mu, sg).mean(0)
    pair = np.zeros(mu.shape[1:])
    for s in range(S - 1):
        pair += _A(mu[s][None] - mu[s + 1:], np.sqrt(sg[s][None] ** 2 + sg[s + 1:] ** 2)).sum(0)
    return first - (2.0 * pair + 2.0 * sg.sum(0) / np.sqrt(np.pi)) / (2.0 * S * S)


def crps_single_gaussian(y, mu, sg):
    """S = 1: sg [z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi)]"""
    z = (y - mu) / sg
    return sg * (z * erf(z / np.sqrt(2.0)) + 2.0 * np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi) - 1.0 / np.sqrt(np.pi))


def rows(y, mu, sg):
    return np.stack([pit(y, mu, sg), crps(y, mu, sg)], axis=-1)


def sums(r, probs):
    """(2 + P, D) from rows (N, D, 2)"""
    N, D, _ = r.shape
    return np.stack([r[..., 1].sum(0), np.full(D, float(N))] + [(r[..., 0] <= p).sum(0).astype(np.float64) for p in probs])


def scores(s, probs, Y_std=1.0):
    """the dict DGP_Base.calibration returns (without n and rows), from the (2 + P, D) sums"""
    cnt = s[1]
    tot = s[2:].sum(1) / cnt.sum()
    cov = {}
    for k, p in enumerate(probs):
        for l, r in enumerate(probs):
            if p < 0.5 and abs(r - (1.0 - p)) <= 1e-12:
                cov[float(1.0 - 2.0 * p)] = float(tot[l] - tot[k])
    return {"crps": Y_std * s[0].sum() / cnt.sum(), "crps_per_output": Y_std * s[0] / cnt, "pit_le": s[2:] / cnt, "coverage": cov}


# ---------------------------------------------------------------- 40 digits
mpmath.mp.dps = 40


def cdf_mp(x, mu, sg):
    """F(x) of one item: x a float, mu / sg 1-d float arrays (taken exactly)"""
    x = mpmath.mpf(float(x))
    r2 = mpmath.sqrt(2)
    return sum(mpmath.erfc(-(x - mpmath.mpf(float(m))) / (mpmath.mpf(float(s)) * r2)) / 2 for m, s in zip(mu, sg)) / len(mu)


def pdf_mp(x, mu, sg):
    x = mpmath.mpf(float(x))
    c = mpmath.sqrt(2 * mpmath.pi)
    return sum(mpmath.exp(-((x - mpmath.mpf(float(m))) / mpmath.mpf(float(s))) ** 2 / 2) / (c * mpmath.mpf(float(s)))
               for m, s in zip(mu, sg)) / len(mu)


def bar_F():
    """what a handful of rounded erfc values can move F"""
    return 4.0 * EPS


def residual(q, p, mu, sg):
    """rho = |F_mp(q) - p| / (4 eps + spacing(q) f_mp(q)) of one item"""
    num = abs(cdf_mp(q, mu, sg) - mpmath.mpf(float(p)))
    den = mpmath.mpf(bar_F()) + mpmath.mpf(float(np.spacing(abs(q)))) * pdf_mp(q, mu, sg)
    return float(num / den)
