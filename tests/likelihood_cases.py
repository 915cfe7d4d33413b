"""The case table of tests/test_gpu_likelihood_direct.py and tests/test_likelihood_reference_cpu.py.  No GPU, no product code.

An element-wise case is dict(name, kind, mu, v, y, p0, p1) with flat float64 vectors; a MultiClass case dict(name, mean (S, N, K), var,
labels (N, 1)).  Every kind runs the ordinary regime (mu ~ 1.2 randn, v in [1e-6, 2]); the edges are those where the formulas of
csrc/likelihood.hpp lose digits or change branch: v -> 0 in gv / sqrt(2 v), large means, Poisson counts on both sides of 170! (the
largest factorial in float64), the digamma recurrence / series switch at 8, Beta's alpha = probit scale near 1e-4 and its clipped
targets, StudentT far in the tails, MultiClass at its variance clips, with saturated cdfs and at the workgroup's 16-row edge."""
import numpy as np

SMALL_V = (1e-8, 1e-12, 1e-16, 1e-30, 0.0)
GAMMA_SHAPES = (1e-3, 0.5, 1.0, 7.9, 8.0, 8.1, 50.0, 1e4)
BETA_SCALES = (0.05, 0.1, 1.0, 30.0, 1e3)
BETA_TARGETS = (0.0, 1e-7, 1e-6, 0.5, 1.0 - 1e-6, 1.0)
POISSON_COUNTS = (0.0, 1.0, 170.0, 171.0, 1e3, 1e6)
POISSON_BINSIZES = (0.01, 1.0, 100.0)
STUDENT_NU = (0.5, 2.5, 3.0, 100.0, 1e6)
STUDENT_SCALES = (1e-3, 1.0, 1e3)
GAUSS_P0 = (1e-6, 1.0, 1e6)
DEFAULT_P = {"gaussian": (0.7, 1.0), "bernoulli": (1.0, 1.0), "poisson": (1.0, 0.8), "exponential": (1.0, 1.0), "student_t": (1.3, 3.0),
             "gamma": (2.2, 1.0), "beta": (3.5, 1.0)}


def targets(kind, rng, n):
    if kind == "poisson":
        return rng.poisson(2.0, size=n).astype(np.float64)
    if kind in ("exponential", "gamma"):
        return rng.exponential(1.3, size=n) + 1e-3
    if kind == "beta":
        return rng.uniform(0.02, 0.98, size=n)
    if kind == "bernoulli":
        return (rng.uniform(size=n) < 0.5).astype(np.float64)
    return rng.standard_t(4.0, size=n)


def _case(name, kind, mu, v, y, p0=None, p1=None):
    d0, d1 = DEFAULT_P[kind]
    mu, v, y = (np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), np.shape(mu)).ravel()) for a in (mu, v, y))
    return dict(name=name, kind=kind, mu=mu, v=v, y=y, p0=float(d0 if p0 is None else p0), p1=float(d1 if p1 is None else p1))


def _grid(*axes):
    g = np.meshgrid(*[np.asarray(a, dtype=np.float64) for a in axes], indexing="ij")
    return [a.ravel() for a in g]


def element_cases():
    out = []
    for i, kind in enumerate(DEFAULT_P):
        rng = np.random.RandomState(100 + i)
        n = 72 if kind == "beta" else 144
        out.append(_case(f"{kind}-ordinary", kind, 1.2 * rng.randn(n), rng.uniform(1e-6, 2.0, size=n), targets(kind, rng, n)))
        n = 20
        out.append(_case(f"{kind}-small-v", kind, rng.randn(n), np.resize(SMALL_V, n), targets(kind, rng, n)))
    rng = np.random.RandomState(7)
    # probit kinds: |mu| up to 12
    mu, v = _grid(np.linspace(-12.0, 12.0, 13), (1e-3, 0.5, 2.0))
    out.append(_case("bernoulli-large-mean-01", "bernoulli", mu, v, np.resize([0.0, 1.0], mu.size)))
    out.append(_case("bernoulli-large-mean-pm1", "bernoulli", mu, v, np.resize([1.0, -1.0, -1.0], mu.size)))
    out.append(_case("bernoulli-ordinary-pm1", "bernoulli", 1.2 * rng.randn(48), rng.uniform(1e-6, 2.0, size=48),
                     np.where(rng.uniform(size=48) < 0.5, -1.0, 1.0)))
    out.append(_case("beta-large-mean", "beta", mu, v, np.resize(BETA_TARGETS, mu.size)))
    # exp links: mu in [-30, 30], v up to 20
    mu, v = _grid(np.linspace(-30.0, 30.0, 13), (1e-3, 1.0, 20.0))
    out.append(_case("exponential-large-mean", "exponential", mu, v, np.resize([1e-3, 1.0, 40.0, 3e3], mu.size)))
    out.append(_case("gamma-large-mean", "gamma", mu, v, np.resize([1e-3, 1.0, 40.0, 3e3], mu.size)))
    for b in POISSON_BINSIZES:
        mu, v, y = _grid((-30.0, -3.0, 0.0, 5.0, 13.8, 30.0), (1e-3, 20.0), POISSON_COUNTS)
        out.append(_case(f"poisson-counts-binsize{b:g}", "poisson", mu, v, y, p1=b))
    for sh in GAMMA_SHAPES:
        mu = np.r_[0.0, 0.0, 1.2 * rng.randn(10)]
        v = np.r_[0.5, 1e-12, rng.uniform(1e-6, 2.0, size=10)]
        y = np.r_[1.0, 1.0, rng.exponential(1.3, size=10) + 1e-3]              # mu = 0, y = 1: dp0 = -digamma(shape)
        out.append(_case(f"gamma-shape{sh:g}", "gamma", mu, v, y, p0=sh))
    for sc in BETA_SCALES:
        mu, v, y = _grid((-8.0, -1.0, 0.3, 4.0), (1e-6, 0.7), BETA_TARGETS)      # mu = -8: probit at its 1e-3 floor, alpha = 1e-3 scale
        out.append(_case(f"beta-scale{sc:g}", "beta", mu, v, y, p0=sc))
    for nu in STUDENT_NU:
        for sc in STUDENT_SCALES:
            res, v = _grid((0.0, 0.3, -1.0, 30.0, -1e3), (1e-6, 1.5))             # residual y - mu in units of the scale
            mu = 0.7 * rng.randn(res.size)
            out.append(_case(f"student_t-nu{nu:g}-scale{sc:g}", "student_t", mu, v * sc * sc, mu + res * sc, p0=sc, p1=nu))
    for p0 in GAUSS_P0:
        n = 24
        out.append(_case(f"gaussian-variance{p0:g}", "gaussian", 1.2 * rng.randn(n), rng.uniform(1e-6, 2.0, size=n), rng.randn(n) * 2.0, p0=p0))
    return out


ELEMENT_CASES = element_cases()
assert len({c["name"] for c in ELEMENT_CASES}) == len(ELEMENT_CASES)


def element_case(name):
    return next(c for c in ELEMENT_CASES if c["name"] == name)


# (S, n, DY) of the layout test: S n DY = 1, 255, 256, 257 and more than one block; S n a multiple of 16 and not; (1, 33, 20) and
# (3, 11, 20): ldt = 48, the fourth block of the transposed form holds only padding
LAYOUT_SHAPES = ((1, 1, 1), (1, 255, 1), (3, 85, 1), (5, 17, 3), (1, 256, 1), (2, 64, 2), (16, 16, 1), (1, 257, 1), (1, 13, 20),
                 (1, 33, 20), (3, 11, 20), (2, 48, 3))


def layout_inputs(kind, shape, seed=3):
    """mean, var (S, n, DY), Y (n, DY) and the flat y of the plain 1 x (S n DY) x 1 call"""
    S, n, DY = shape
    rng = np.random.RandomState(seed + S * 1000 + n * 10 + DY)
    mu, v = 1.2 * rng.randn(S, n, DY), rng.uniform(1e-6, 2.0, size=(S, n, DY))
    Y = targets(kind, rng, n * DY).reshape(n, DY)
    return mu, v, Y, np.tile(Y.ravel(), S)


# ------------------------------------------------------------------------------------------------ MultiClass
def _labels(N, K):
    return ((K - 1 - np.arange(N)) % K).astype(np.float64).reshape(N, 1)          # the first row carries K - 1, then every label in turn


def _mc(name, mean, var, labels):
    return dict(name=name, mean=np.ascontiguousarray(mean, dtype=np.float64), var=np.ascontiguousarray(var, dtype=np.float64),
                labels=np.asarray(labels, dtype=np.float64))


def multiclass_cases():
    out = []
    for K, S, N in ((2, 1, 1), (3, 1, 15), (10, 1, 16), (31, 1, 17), (32, 1, 16), (3, 3, 11), (2, 1, 33), (10, 3, 5)):
        rng = np.random.RandomState(10 * K + S * N)
        out.append(_mc(f"mc-ordinary-K{K}-R{S * N}", 1.5 * rng.randn(S, N, K), rng.uniform(0.05, 2.0, size=(S, N, K)), _labels(N, K)))
    # the clips: v_k around 1e-10, v_y around 0.5e-10 (one ulp below, the tie, one ulp above), zero and negative variances; the means
    # a few 1e-5 apart, so that the cdfs stay off their floors where the variances are this small
    K, N = 3, 17
    rng = np.random.RandomState(5)
    lab = _labels(N, K)
    ck, cy = 1e-10, 0.5e-10
    pool_k = [np.nextafter(ck, 0.0), ck, np.nextafter(ck, 1.0), 0.0, -0.3, 3e-10]
    pool_y = [np.nextafter(cy, 0.0), cy, np.nextafter(cy, 1.0), 0.0, -0.3, 3e-10]
    var = np.empty((1, N, K))
    for i in range(N):
        for k in range(K):
            pool = pool_y if k == int(lab[i, 0]) else pool_k
            var[0, i, k] = pool[(i + 2 * k) % len(pool)]
    out.append(_mc("mc-clips-K3-R17", 1e-5 * rng.randn(1, N, K), var, lab))
    var2 = np.where(rng.uniform(size=(1, N, K)) < 0.5, var, rng.uniform(0.05, 1.0, size=(1, N, K)))
    out.append(_mc("mc-clips-mixed-K3-R17", 0.5 * rng.randn(1, N, K), var2, lab))
    # class means 8 sigma apart both ways: the labelled class far below (every cdf at its 1e-4 floor) and far above the others
    for K, N in ((3, 4), (32, 6)):
        rng = np.random.RandomState(K)
        lab = _labels(N, K)
        var = rng.uniform(0.5, 1.5, size=(1, N, K))
        mean = 0.1 * rng.randn(1, N, K)
        sign = np.where(np.arange(N) % 2 == 0, -1.0, 1.0)
        for i in range(N):
            y = int(lab[i, 0])
            mean[0, i, y] += sign[i] * 8.0 * np.sqrt(var[0, i].max() + var[0, i, y])
        out.append(_mc(f"mc-separated-K{K}-R{N}", mean, var, lab))
    return out


MULTICLASS_CASES = multiclass_cases()
