"""CPU side of tests/test_gpu_likelihood_direct.py: what the likelihood kernels of a training step compute, restated once and evaluated
three ways.  No GPU, no product code; tests/test_likelihood_reference_cpu.py holds this module to its own bars.

The rule is upstream's: 20 Gauss-Hermite nodes x_k and weights w_k / sqrt(pi), the float64 numbers numpy's hermgauss(20) gives,
f_k = mu + sqrt(2 v) x_k; closed forms where GPflow has them (Gaussian; Poisson / Exponential / Gamma with the exp link; the Bernoulli's
predictions).  Per element the quantities are
  ve  the variational expectation,  dmu, dv, dp0  its derivatives w.r.t. mean, variance and the likelihood's own parameter
      (Gaussian.variance, StudentT.scale, Gamma.shape, Beta.scale; the analytic derivatives OF THE RULE, not of the integral),
  ld  the log predictive density,  pm, pv  the predictive mean / variance,
and per MultiClass row  p (the probability that the labelled class is largest), ve, dmean[K], dvar[K].

Every quantity is a sum of terms, and each evaluation returns (value, scale) with scale = the sum of the ABSOLUTE values of those terms
(for ld: the terms of the exponents weighted by their share of the sum, plus |ld| itself).  The measure of an error is
    |x - truth| / (eps scale),   eps = 2^-52, scale from the truth,
so that gv / sqrt(2 v) at v -> 0, q - e^2 and the lgamma differences are judged by what their own cancellation allows.

Backends of the one formula set:  MP = 40-digit mpmath on the float64 inputs (the truth);  NPB = numpy + scipy.special, nodes summed
0 .. 19;  THB = torch CPU float64, nodes summed in symmetric pairs from the outside in and the MultiClass product from the last class
down.  bar = factor_reference.device_bar(the larger comparator's worst measure over the case) = 8 x that, never below 1."""
import math

import numpy as np

from tests.factor_reference import device_bar

EPS = 2.0 ** -52
KINDS = ("gaussian", "bernoulli", "poisson", "exponential", "student_t", "gamma", "beta")
HAS_PARAM = ("gaussian", "student_t", "gamma", "beta")
CLOSED_VE = ("gaussian", "poisson", "exponential", "gamma")
ELEMENT_QUANTITIES = ("ve", "dmu", "dv", "dp0", "ld", "pm", "pv")
GH_X, _gw = np.polynomial.hermite.hermgauss(20)
GH_W = _gw / math.sqrt(math.pi)
LD_FLOOR = -600.0          # below it float64's exp leaves the normal range inside the rule: upstream's ld is -inf or denormal-limited


# ------------------------------------------------------------------------------------------------ backends
class NPB:
    name = "numpy"
    exp, log, sqrt, abs = np.exp, np.log, np.sqrt, np.abs

    @staticmethod
    def arr(a):
        return np.asarray(a, dtype=np.float64)

    @staticmethod
    def c(x):
        return float(x)

    @staticmethod
    def erf(x):
        from scipy.special import erf
        return erf(x)

    @staticmethod
    def lgamma(x):
        from scipy.special import gammaln
        return gammaln(x)

    @staticmethod
    def digamma(x):
        from scipy.special import psi
        return psi(x)

    @staticmethod
    def where(mask, a, b):
        return np.where(mask, a, b)

    @staticmethod
    def node_sum(vals):
        out = vals[0]
        for t in vals[1:]:
            out = out + t
        return out

    class_order = staticmethod(lambda K: range(K))

    @staticmethod
    def out(a):
        return np.asarray(a, dtype=np.float64)


class THB:
    name = "torch"

    @staticmethod
    def _t():
        import torch
        return torch

    @classmethod
    def arr(cls, a):
        return cls._t().as_tensor(np.array(a, dtype=np.float64))

    @staticmethod
    def c(x):
        return float(x)

    @classmethod
    def _un(cls, fn, x):
        t = cls._t()
        return getattr(t, fn)(x if t.is_tensor(x) else t.as_tensor(float(x), dtype=t.float64))

    @classmethod
    def where(cls, mask, a, b):
        t = cls._t()
        a, b = (x if t.is_tensor(x) else t.as_tensor(float(x), dtype=t.float64) for x in (a, b))
        return t.where(t.as_tensor(np.asarray(mask)), a, b)

    @staticmethod
    def node_sum(vals):
        n = len(vals)
        out = vals[0] + vals[n - 1]
        for a in range(1, n // 2):
            out = out + (vals[a] + vals[n - 1 - a])
        return out

    class_order = staticmethod(lambda K: range(K - 1, -1, -1))

    @staticmethod
    def out(a):
        return a.numpy().astype(np.float64) if hasattr(a, "numpy") else np.asarray(a, dtype=np.float64)


for _fn, _tn in (("exp", "exp"), ("log", "log"), ("sqrt", "sqrt"), ("abs", "abs"), ("erf", "erf"), ("lgamma", "lgamma"), ("digamma", "digamma")):
    setattr(THB, _fn, classmethod(lambda cls, x, _tn=_tn: cls._un(_tn, x)))


class MP:
    name = "mpmath"
    DPS = 40

    @staticmethod
    def _mp():
        import mpmath
        return mpmath

    @classmethod
    def arr(cls, a):
        mpf = cls._mp().mpf
        a = np.asarray(a, dtype=np.float64)
        return np.array([mpf(float(x)) for x in a.ravel()], dtype=object).reshape(a.shape)

    @classmethod
    def c(cls, x):
        return cls._mp().mpf(float(x))

    @classmethod
    def _un(cls, fn, x):
        f = getattr(cls._mp(), fn)
        return np.frompyfunc(f, 1, 1)(x) if isinstance(x, np.ndarray) else f(x)

    @staticmethod
    def where(mask, a, b):
        return np.where(mask, a, b)

    node_sum = NPB.node_sum
    class_order = NPB.class_order

    @staticmethod
    def out(a):
        """longdouble: 19 digits, far below every error that is compared with them (a term below its range, exp(-1e10), becomes 0)"""
        mp = MP._mp()
        tiny = mp.mpf("1e-4900")
        return np.array([np.longdouble(mp.nstr(x, 25)) if abs(x) > tiny else np.longdouble(0) for x in np.asarray(a, dtype=object).ravel()],
                        dtype=np.longdouble).reshape(np.shape(a))


class MPRAW(MP):
    """the truth left as mpmath numbers (object arrays): for differences that longdouble cannot hold"""
    out = staticmethod(lambda a: np.asarray(a, dtype=object))


for _fn, _mn in (("exp", "exp"), ("log", "log"), ("sqrt", "sqrt"), ("abs", "fabs"), ("erf", "erf"), ("lgamma", "loggamma"), ("digamma", "digamma")):
    setattr(MP, _fn, classmethod(lambda cls, x, _mn=_mn: cls._un(_mn, x)))


class _Sum:
    """a sum of terms with the sum of their magnitudes"""

    def __init__(self, B, terms):
        self.v = terms[0]
        self.s = B.abs(terms[0])
        for t in terms[1:]:
            self.v = self.v + t
            self.s = self.s + B.abs(t)


# ------------------------------------------------------------------------------------------------ the link and the log densities
def _probit(B, f):
    """Phi(f) (1 - 2e-3) + 1e-3: the Bernoulli's and the Beta's inverse link"""
    return B.c(0.5) * (B.c(1.0) + B.erf(f * B.c(math.sqrt(0.5)))) * B.c(1.0 - 2e-3) + B.c(1e-3)


def _dprobit(B, f):
    return B.c(1.0 - 2e-3) * B.c(1.0 / math.sqrt(2.0 * math.pi)) * B.exp(B.c(-0.5) * f * f)


def _logp(B, kind, f, y, p0, p1, want_grad):
    """terms of log p(y | f), and with want_grad the terms of d / df and of d / dp0 (None where the kind has no parameter)"""
    one, half = B.c(1.0), B.c(0.5)
    if kind == "bernoulli":
        p = _probit(B, f)
        is1 = np.asarray(y["f64"] == 1.0)
        q = B.where(is1, p, one - p)
        if not want_grad:
            return [B.log(q)], None, None
        return [B.log(q)], [B.where(is1, one, -one) * _dprobit(B, f) / q], None
    yv = y["b"]
    if kind == "poisson":
        t = [yv * f, yv * B.log(p1), -(B.exp(f) * p1), -B.lgamma(yv + one)]
        return t, None, None
    if kind == "exponential":
        return [-(yv * B.exp(-f)), -f], None, None
    if kind == "gamma":
        return [-(p0 * f), -B.lgamma(p0), (p0 - one) * B.log(yv), -(yv * B.exp(-f))], None, None
    if kind == "student_t":
        nu, r = p1, yv - f
        den = nu * p0 * p0 + r * r
        t = [B.lgamma(half * (nu + one)), -B.lgamma(half * nu), -(half * B.log(nu)), -B.c(0.5 * math.log(math.pi)), -B.log(p0),
             -(half * (nu + one) * B.log(den / (nu * p0 * p0)))]
        if not want_grad:
            return t, None, None
        return t, [(nu + one) * r / den], [-(one / p0) + 0 * f, (nu + one) * r * r / (p0 * den)]
    if kind == "beta":
        m = _probit(B, f)
        al = m * p0
        be = p0 - al
        ly, l1y = y["ly"], y["l1y"]
        t = [(al - one) * ly, (be - one) * l1y, B.lgamma(p0) + 0 * f, -B.lgamma(al), -B.lgamma(be)]
        if not want_grad:
            return t, None, None
        da, db, c = B.digamma(al), B.digamma(be), _dprobit(B, f) * p0
        return (t, [c * ly, -(c * l1y), -(c * da), c * db],
                [m * ly, (one - m) * l1y, B.digamma(p0) + 0 * f, -(m * da), -((one - m) * db)])
    raise ValueError(kind)


def _cond(B, kind, f, p0, p1):
    """conditional mean and variance of y given f"""
    if kind == "poisson":
        e = B.exp(f) * p1
        return e, e
    if kind == "exponential":
        e = B.exp(f)
        return e, e * e
    if kind == "gamma":
        e = B.exp(f)
        return p0 * e, p0 * e * e
    if kind == "beta":
        m = _probit(B, f)
        return m, (m - m * m) / (p0 + B.c(1.0))
    if kind == "student_t":
        return f, p0 * p0 * (p1 / (p1 - B.c(2.0))) + 0 * f
    raise ValueError(kind)


def _targets(B, kind, y):
    y = np.asarray(y, dtype=np.float64)
    out = {"f64": y, "b": B.arr(y)}
    if kind == "beta":
        yc = B.arr(np.clip(y, 1e-6, 1.0 - 1e-6))
        out["ly"], out["l1y"] = B.log(yc), B.log(B.c(1.0) - yc)
    return out


def elementwise(B, kind, mu, v, y, p0=1.0, p1=1.0, which=ELEMENT_QUANTITIES):
    """-> {quantity: (value, scale)} as float64 (MP: longdouble) arrays of mu's shape; mu, v, y float64 arrays of one shape.
    p0: Gaussian.variance / StudentT.scale / Gamma.shape / Beta.scale; p1: Poisson.binsize / StudentT.deg_free."""
    if issubclass(B, MP):
        with MP._mp().workdps(MP.DPS):
            return _elementwise(B, kind, mu, v, y, p0, p1, which)
    with np.errstate(all="ignore"):
        return _elementwise(B, kind, mu, v, y, p0, p1, which)


def _elementwise(B, kind, mu, v, y, p0, p1, which):
    shape = np.shape(mu)
    v64 = np.ravel(np.asarray(v, dtype=np.float64))
    mu, v = B.arr(np.ravel(mu)), B.arr(v64)
    yt = _targets(B, kind, np.ravel(y))
    p0, p1 = B.c(p0), B.c(p1)
    one, half, two = B.c(1.0), B.c(0.5), B.c(2.0)
    res = {}
    want_ve = any(q in which for q in ("ve", "dmu", "dv", "dp0"))
    sd = B.sqrt(two * v)
    nodes = [(B.c(x), B.c(w), mu + sd * B.c(x)) for x, w in zip(GH_X, GH_W)]
    yv = yt["b"]
    zero = 0 * mu

    def put(name, s):
        if name in which:
            res[name] = (B.out(s.v).reshape(shape), B.out(s.s).reshape(shape))

    if want_ve and kind == "gaussian":
        r = yv - mu
        put("ve", _Sum(B, [-B.c(0.5 * math.log(2.0 * math.pi)) + zero, -(half * B.log(p0)) + zero, -(half * r * r / p0), -(half * v / p0)]))
        put("dmu", _Sum(B, [yv / p0, -(mu / p0)]))
        put("dv", _Sum(B, [-(half / p0) + zero]))
        put("dp0", _Sum(B, [-(half / p0) + zero, half * r * r / (p0 * p0), half * v / (p0 * p0)]))
    elif want_ve and kind in ("poisson", "exponential", "gamma"):
        if kind == "poisson":
            e = B.exp(mu + half * v) * p1
            put("ve", _Sum(B, [yv * mu, -e, -B.lgamma(yv + one), yv * B.log(p1)]))
            put("dmu", _Sum(B, [yv, -e]))
        else:
            e = B.exp(-mu + half * v) * yv
            if kind == "exponential":
                put("ve", _Sum(B, [-e, -mu]))
                put("dmu", _Sum(B, [e, -one + zero]))
            else:
                put("ve", _Sum(B, [-(p0 * mu), -B.lgamma(p0) + zero, (p0 - one) * B.log(yv), -e]))
                put("dmu", _Sum(B, [e, -p0 + zero]))
                put("dp0", _Sum(B, [-mu, -B.digamma(p0) + zero, B.log(yv)]))
        put("dv", _Sum(B, [-(half * e)]))
        if kind != "gamma":
            put("dp0", _Sum(B, [zero]))
    elif want_ve:
        acc = {k: ([], []) for k in ("ve", "dmu", "dv", "dp0")}
        for x, w, f in nodes:
            t, g, gp = _logp(B, kind, f, yt, p0, p1, True)
            for name, terms in (("ve", t), ("dmu", g), ("dv", [gi * x for gi in g]), ("dp0", gp)):
                if terms is not None:
                    s = _Sum(B, terms)
                    acc[name][0].append(w * s.v)
                    acc[name][1].append(w * s.s)
        for name in ("ve", "dmu", "dv", "dp0"):
            if name not in which:
                continue
            if not acc[name][0]:
                res[name] = (B.out(zero).reshape(shape), B.out(zero).reshape(shape))
                continue
            val, sc = B.node_sum(acc[name][0]), B.node_sum(acc[name][1])
            if name == "dv":          # (v = 0: no finite gradient, the element is masked out — quantity_masks)
                sdd = B.where(v64 == 0.0, one + zero, sd)
                val, sc = val / sdd, sc / sdd
            res[name] = (B.out(val).reshape(shape), B.out(sc).reshape(shape))
    if "ld" in which:
        if kind == "gaussian":
            vv, r = v + p0, yv - mu
            put("ld", _Sum(B, [-B.c(0.5 * math.log(2.0 * math.pi)) + zero, -(half * B.log(vv)), -(half * r * r / vv)]))
        elif kind == "bernoulli":
            t, _, _ = _logp(B, kind, mu / B.sqrt(one + v), yt, p0, p1, False)
            put("ld", _Sum(B, t))
        else:
            vals, wts = [], []
            for x, w, f in nodes:
                s = _Sum(B, _logp(B, kind, f, yt, p0, p1, False)[0])
                e = w * B.exp(s.v)
                vals.append(e)
                wts.append(e * s.s)
            tot = B.node_sum(vals)
            ld = B.log(tot)
            res["ld"] = (B.out(ld).reshape(shape), B.out(B.abs(ld) + one + B.node_sum(wts) / tot).reshape(shape))
    if "pm" in which or "pv" in which:
        if kind == "gaussian":
            put("pm", _Sum(B, [mu]))
            put("pv", _Sum(B, [v, p0 + zero]))
        elif kind == "bernoulli":
            p = _probit(B, mu / B.sqrt(one + v))
            put("pm", _Sum(B, [p]))
            put("pv", _Sum(B, [p, -(p * p)]))
        else:
            es, qs, ea = [], [], []
            for x, w, f in nodes:
                cm, cv = _cond(B, kind, f, p0, p1)
                es.append(w * cm)
                ea.append(w * B.abs(cm))
                qs.append(w * (cv + cm * cm))
            e, q = B.node_sum(es), B.node_sum(qs)
            if "pm" in which:
                res["pm"] = (B.out(e).reshape(shape), B.out(B.node_sum(ea)).reshape(shape))
            put("pv", _Sum(B, [q, -(e * e)]))
    return res


# ------------------------------------------------------------------------------------------------ MultiClass (RobustMax, eps = 1e-3)
MC_EPS = 1e-3


def multiclass(B, mean, var, labels, w=1.0):
    """mean, var (R, K) float64, labels (R,) integers -> {p, ve: ((R,), scale), dmean, dvar: ((R, K), scale)}; dmean / dvar are the
    adjoints of the loss -w ve the device stores.  Clips as upstream: 2 v_y at 1e-10 (so v_y at 0.5e-10), v_k at 1e-10, each with the
    gradient of the clipped side switched off (v > clip passes the gradient)."""
    if issubclass(B, MP):
        with MP._mp().workdps(MP.DPS):
            return _multiclass(B, mean, var, labels, w)
    return _multiclass(B, mean, var, labels, w)


def _multiclass(B, mean, var, labels, w):
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    R, K = mean.shape
    lab = np.asarray(labels).astype(np.int64).reshape(R)
    assert np.all((lab >= 0) & (lab < K))
    rows = np.arange(R)
    one, half, two = B.c(1.0), B.c(0.5), B.c(2.0)
    mu = [B.arr(mean[:, k]) for k in range(K)]
    vk = [B.arr(np.maximum(var[:, k], 1e-10)) for k in range(K)]
    gate_k = [var[:, k] > 1e-10 for k in range(K)]
    mu_y = B.arr(mean[rows, lab])
    vy_raw = var[rows, lab]
    sy = B.sqrt(two * B.arr(np.maximum(vy_raw, 0.5e-10)))
    gate_y = vy_raw > 0.5e-10
    other = [lab != k for k in range(K)]
    rs = [one / B.sqrt(two * vk[k]) for k in range(K)]
    zero = 0 * mu_y
    isp = B.c(1.0 / math.sqrt(math.pi))
    c_cdf, floor = B.c(1.0 - 2e-4), B.c(1e-4)
    p_nodes = []
    g_mu = [[] for _ in range(K)]          # per class: node terms of dp / dmu_k (k != y)
    g_v = [[] for _ in range(K)]           # ... of dp / dv_k
    g_y, g_sy = [], []                     # node terms of dp / dmu_y, dp / dsy (each already summed over the classes)
    for x, wn in zip(GH_X, GH_W):
        x, wn = B.c(x), B.c(wn)
        X = mu_y + x * sy
        u, cdf = [None] * K, [None] * K
        P = one + zero
        for k in B.class_order(K):
            u[k] = (X - mu[k]) * rs[k]
            cdf[k] = B.where(other[k], half * (one + B.erf(u[k])) * c_cdf + floor, one + zero)
            P = P * cdf[k]
        p_nodes.append(wn * P)
        ty, tsy = zero, zero
        for k in B.class_order(K):
            t = B.where(other[k], wn * (P / cdf[k]) * c_cdf * isp * B.exp(-(u[k] * u[k])), zero)       # w_h dP / du_k
            g_mu[k].append(-(t * rs[k]))
            g_v[k].append(B.where(gate_k[k], -(t * u[k] / (two * vk[k])), zero))
            ty = ty + t * rs[k]
            tsy = tsy + t * rs[k] * x
        g_y.append(ty)
        g_sy.append(tsy)
    p = B.node_sum(p_nodes)
    l1, l0 = B.c(math.log(1.0 - MC_EPS)), B.c(math.log(MC_EPS / (K - 1.0)))
    ve = _Sum(B, [p * l1, l0 + zero, -(p * l0)])
    ek = B.c(MC_EPS / (K - 1.0))
    mix = _Sum(B, [p * B.c(1.0 - MC_EPS), ek + zero, -(p * ek)])                 # predictive probability of the labelled class
    ld = B.log(mix.v)
    s = -(B.c(w) * (l1 - l0))
    sabs = B.abs(s)
    dm_v, dm_s, dv_v, dv_s = [], [], [], []
    for k in range(K):
        is_y = ~other[k]
        gm = B.where(is_y, B.node_sum(g_y), B.node_sum(g_mu[k]))
        gm_s = B.where(is_y, B.node_sum([B.abs(t) for t in g_y]), B.node_sum([B.abs(t) for t in g_mu[k]]))
        gvy = B.where(gate_y, B.node_sum(g_sy) / sy, zero)
        gvy_s = B.where(gate_y, B.node_sum([B.abs(t) for t in g_sy]) / sy, zero)
        gv = B.where(is_y, gvy, B.node_sum(g_v[k]))
        gv_s = B.where(is_y, gvy_s, B.node_sum([B.abs(t) for t in g_v[k]]))
        dm_v.append(B.out(s * gm)); dm_s.append(B.out(sabs * gm_s))
        dv_v.append(B.out(s * gv)); dv_s.append(B.out(sabs * gv_s))
    return {"p": (B.out(p), B.out(p)), "ve": (B.out(ve.v), B.out(ve.s)), "ld": (B.out(ld), B.out(B.abs(ld) + mix.s / mix.v)),
            "dmean": (np.stack(dm_v, 1), np.stack(dm_s, 1)), "dvar": (np.stack(dv_v, 1), np.stack(dv_s, 1))}


# ------------------------------------------------------------------------------------------------ measures and bars
def measure(x, truth):
    """worst |x - value| / (eps scale) over the finite-scaled elements; where the scale is 0 the value must be met exactly.
    truth = (value, scale) from the MP backend"""
    val, sc = truth
    x = np.asarray(x, dtype=np.longdouble)
    err = np.abs(x - val)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.where(sc > 0, err / (EPS * sc), np.where(err == 0, 0.0, np.inf))
    m = np.where(np.isfinite(x), m, np.inf)
    return float(np.max(m)) if m.size else 0.0


def bars(cpu_a, cpu_b):
    """{quantity: device_bar(max of the two comparators' measures)}"""
    return {k: device_bar(max(cpu_a[k], cpu_b[k]), 0) for k in cpu_a}


_TRUTH = {}


def element_truth(case):
    """the 40-digit values of every quantity of an element-wise case (tests/likelihood_cases.py), the two comparators' measures and the
    bars; computed once per case"""
    key = case["name"]
    if key not in _TRUTH:
        args = (case["kind"], case["mu"], case["v"], case["y"], case["p0"], case["p1"])
        tr = elementwise(MP, *args)
        a, b = elementwise(NPB, *args), elementwise(THB, *args)
        sel = quantity_masks(case, tr)
        ma = {q: measure(a[q][0][sel[q]], (tr[q][0][sel[q]], tr[q][1][sel[q]])) for q in tr}
        mb = {q: measure(b[q][0][sel[q]], (tr[q][0][sel[q]], tr[q][1][sel[q]])) for q in tr}
        _TRUTH[key] = dict(truth=tr, numpy=ma, torch=mb, bars=bars(ma, mb), masks=sel, numpy_values=a)
    return _TRUTH[key]


def quantity_masks(case, tr):
    """which elements a quantity is measured on: dv not at v = 0 (upstream's sqrt has no finite gradient there), ld where the rule stays
    inside float64's normal range (LD_FLOOR), pv where the kind has a finite conditional variance"""
    v = np.asarray(case["v"])
    full = np.ones(v.shape, dtype=bool)
    out = {q: full for q in tr}
    out["dv"] = v != 0.0
    out["ld"] = np.asarray(tr["ld"][0] > LD_FLOOR)
    return out


_MC_TRUTH = {}


def multiclass_truth(case):
    key = case["name"]
    if key not in _MC_TRUTH:
        S, N, K = case["mean"].shape
        lab = np.tile(case["labels"].reshape(-1), S)
        args = (case["mean"].reshape(S * N, K), case["var"].reshape(S * N, K), lab)
        tr = multiclass(MP, *args)
        a, b = multiclass(NPB, *args), multiclass(THB, *args)
        sel = multiclass_masks(args[1], lab)
        ma = {q: measure(a[q][0][sel[q]], (tr[q][0][sel[q]], tr[q][1][sel[q]])) for q in tr}
        mb = {q: measure(b[q][0][sel[q]], (tr[q][0][sel[q]], tr[q][1][sel[q]])) for q in tr}
        _MC_TRUTH[key] = dict(truth=tr, numpy=ma, torch=mb, bars=bars(ma, mb), masks=sel, labels=lab)
    return _MC_TRUTH[key]


def multiclass_masks(var, lab):
    """dvar is not measured at an exact tie with a clip (v_k == 1e-10, v_y == 0.5e-10): the value only"""
    R, K = var.shape
    is_y = np.arange(K)[None, :] == lab[:, None]
    tie = np.where(is_y, var == 0.5e-10, var == 1e-10)
    return {"p": np.ones(R, bool), "ve": np.ones(R, bool), "ld": np.ones(R, bool), "dmean": np.ones((R, K), bool), "dvar": ~tie}
