"""A plain long-double Adam step with first-order error bounds, the mask classes of a model's parameter vector built from the Python
side alone, and the seeded inputs the direct Adam tests inject (tests/test_adam_reference_cpu.py, tests/test_gpu_adam_direct.py).

Mask classes (csrc/model.hip, `mark`): 0 is never updated (a frozen Parameter, the structurally zero entries above the diagonal of
every q_sqrt), 1 is updated by the optimiser sweep, 2 (kernel variance, lengthscales, white variance, the likelihood's parameter) by
the sweep of the separate launch and by its owner block in the fused tail.

Bounds, u = 2^-53, first order in u, for the float64 evaluation of
    m* = b1 m + c1 g,  v* = b2 v + c2 g^2,  D* = lr_t m* / (sqrt(v*) + eps),  theta* = theta - D*
with c1 = fl(1 - b1), c2 = fl(1 - b2) taken as data (the reference forms them in float64 too):
    B_m     = 2u (|b1 m| + |c1 g|)            two products and a sum; absolute, because the sum may cancel
    B_v     = 4u v*                           g g, c2 (g g), b2 v, the sum: every term non-negative -> (1 + u)^3 < 1 + 4u
    rho_t   = u (4.5 + p2/(1-p2) + 2 p1/(1-p1)),  p_i = b_i^t
              the host's lr_t = lr sqrt(1 - p2) / (1 - p1): pow to 1 ulp (2u p_i on p_i), each subtraction u and the cancellation
              factor p_i / (1 - p_i) on pow's error; the root halves what is under it and adds u, product and quotient u each:
              (2u p2/(1-p2) + u)/2 + u  +  2u p1/(1-p1) + u  +  2u  =  u (4.5 + p2/(1-p2) + 2 p1/(1-p1))
    B_theta = u |theta*| + lr_t/(sqrt(v*)+eps) B_m + (8u + rho_t) |D*|
              the final subtraction; m's error carried through; sqrt, add, divide, multiply (4u) plus B_v/v* halved by the root (2u)
              — the sum sqrt(v*) + eps only shrinks the root's relative error — and 2u of slack on top of the 6u counted so far.
A contraction to fma only removes roundings, so the bounds hold for either code generation.  The asserted bar is TWICE each bound."""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
BAR = 2.0             # asserted bar / first-order bound


def require_extended_precision():
    """the reference has to carry more digits than what it judges (x86 long double: 64-bit significand)"""
    assert np.finfo(LD).nmant >= 63, "np.longdouble is no wider than float64 here: the reference would judge itself"


# ------------------------------------------------------------------------------------------------ mask classes
def host_entries(model):
    """Engine.entries of `model` — (Parameter, offset, count, kind) — from Engine._build_layout on an instance that never opens the
    device (models whose mean functions are Identity, Zero or a Linear map held in theta: the builder then needs no context)"""
    from doubly_stochastic_dgp import settings
    from doubly_stochastic_dgp.engine import Engine
    eng = Engine.__new__(Engine)
    eng.ctx = None
    eng.layers, eng.likelihood, eng.white = list(model.layers), model.likelihood.likelihood, bool(model.white)
    eng.jitter = float(settings.jitter)
    eng._build_layout()
    for p, *_ in eng.entries:                       # leave no owner behind that cannot answer the coherence hooks
        if eng in p._owners:
            p._owners.remove(eng)
    return list(eng.entries), int(eng.n_theta)


def mask_from_model(model, entries=None):
    """Mask class 0 / 1 / 2 of every entry of theta as an int8 array.  entries: Engine.entries (default: the model's engine's)."""
    from doubly_stochastic_dgp.gpflow_compat import likelihood_entry, split_kernel
    if entries is None:
        entries = model.engine().entries
    owned = []                                      # the Parameters whose gradient the tail's owner blocks produce
    for layer in model.layers:
        stat, wk = split_kernel(layer.kern)
        owned += [stat.variance, stat.lengthscales] + ([wk.variance] if wk is not None else [])
    lik_p = likelihood_entry(model.likelihood.likelihood)[1]
    if lik_p is not None:
        owned.append(lik_p)
    n = max(off + cnt for _, off, cnt, _ in entries)
    mask = np.full(n, -1, dtype=np.int8)
    for p, off, cnt, kind in entries:
        assert np.all(mask[off:off + cnt] == -1), "overlapping entries"
        cls = 0 if not p.trainable else (2 if any(p is q for q in owned) else 1)
        blk = np.full(cnt, cls, dtype=np.int8)
        if kind == "qsqrt":
            D, M, M2 = p.shape
            assert M == M2 and cnt == D * M * M
            blk = blk.reshape(D, M, M)
            blk[:, np.triu_indices(M, 1)[0], np.triu_indices(M, 1)[1]] = 0       # j > i
            blk = blk.reshape(-1)
        mask[off:off + cnt] = blk
    assert np.all(mask >= 0), "theta has entries no Parameter owns"
    return mask


def pair_census(mask):
    """-> (set of (class of the even entry, class of the odd entry) over the pairs (2k, 2k+1), n odd?, class of the last entry)"""
    n = mask.size
    ev, od = mask[0:n - (n & 1):2], mask[1::2]
    return set(zip(ev.tolist(), od.tolist())), bool(n & 1), int(mask[-1])


# ------------------------------------------------------------------------------------------------ the step
def lr_t_host(lr, b1, b2, t):
    """adam_lr_t of csrc/model_schedule.hpp, in float64"""
    return lr * math.sqrt(1.0 - math.pow(b2, float(t))) / (1.0 - math.pow(b1, float(t)))


def adam_ld(theta, g, m, v, on, lr, b1, b2, eps, t):
    """One Adam step in long double on float64 inputs -> dict(theta, m, v: long double results, B_theta, B_m, B_v: first-order bounds
    of a float64 evaluation, long double).  Entries with on == False come back unchanged, with bound 0."""
    require_extended_precision()
    on = np.asarray(on, dtype=bool)
    th0, g0, m0, v0 = (np.asarray(a, dtype=np.float64) for a in (theta, g, m, v))
    c1, c2 = 1.0 - b1, 1.0 - b2                                   # float64, as the kernel forms them
    lb1, lb2, lc1, lc2, leps = LD(b1), LD(b2), LD(c1), LD(c2), LD(eps)
    p1, p2 = lb1 ** LD(t), lb2 ** LD(t)
    lrt = LD(lr) * np.sqrt(LD(1) - p2) / (LD(1) - p1)
    rho = LD(U) * (LD(4.5) + p2 / (LD(1) - p2) + LD(2) * p1 / (LD(1) - p1))
    idx = np.flatnonzero(on)
    gl, ml, vl, tl = (a[idx].astype(LD) for a in (g0, m0, v0, th0))
    t1, t2 = lb1 * ml, lc1 * gl
    ms = t1 + t2
    vs = lb2 * vl + lc2 * gl * gl
    gain = lrt / (np.sqrt(vs) + leps)
    ds = gain * ms
    ts = tl - ds
    Bm = LD(2 * U) * (np.abs(t1) + np.abs(t2))
    Bv = LD(4 * U) * vs
    Bt = LD(U) * np.abs(ts) + gain * Bm + (LD(8 * U) + rho) * np.abs(ds)
    out = {}
    for key, base, new, bound in (("theta", th0, ts, Bt), ("m", m0, ms, Bm), ("v", v0, vs, Bv)):
        r = base.astype(LD)
        r[idx] = new
        b = np.zeros(base.size, dtype=LD)
        b[idx] = bound
        out[key], out["B_" + key] = r, b
    out["lr_t"], out["rho_t"] = lrt, rho
    return out


def adam_f64(theta, g, m, v, on, lr, b1, b2, eps, t):
    """the same step in plain float64 numpy, lr_t as the host forms it -> (theta, m, v)"""
    on = np.asarray(on, dtype=bool)
    lrt = lr_t_host(lr, b1, b2, t)
    m1 = np.where(on, b1 * m + (1.0 - b1) * g, m)
    v1 = np.where(on, b2 * v + (1.0 - b2) * g * g, v)
    with np.errstate(invalid="ignore", divide="ignore"):
        th = np.where(on, theta - lrt * m1 / (np.sqrt(v1) + eps), theta)
    return th, m1, v1


def ratios(got, ref, bound, on):
    """|got - ref| / bound per entry in long double (0 where both vanish, inf where only the bound does); 0 off the live entries"""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / bound)
    return np.where(on, r, LD(0))


# ------------------------------------------------------------------------------------------------ inputs
def _signed_log_uniform(rng, n, lo, hi):
    return np.where(rng.rand(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(lo, hi, n)


def make_inputs(mask, seed, b1):
    """Seeded (theta, g, m, v, zero) for a mask: theta in +-10^[-3, 3], g and m in +-10^[-12, 6], v the square of such a number; a tenth
    of the live entries with b1 m = -c1 g (1 + 1e-9 xi), xi uniform in [-1, 1], so that m* cancels (b1 = 0: nothing to cancel against,
    the entries stay as drawn); another tenth with g = m = v = 0 (`zero` marks them).  No subnormals, g^2 <= 1e12.  Class-0 entries
    carry distinct finite non-zero poison in g, m and v — above the diagonal of a q_sqrt as in a frozen Parameter."""
    mask = np.asarray(mask)
    n = mask.size
    rng = np.random.RandomState(seed)
    theta = _signed_log_uniform(rng, n, -3, 3)
    g = _signed_log_uniform(rng, n, -12, 6)
    m = _signed_log_uniform(rng, n, -12, 6)
    v = _signed_log_uniform(rng, n, -12, 6) ** 2
    live = np.flatnonzero(mask != 0)
    pick = rng.permutation(live.size)
    k = live.size // 10
    cancel, zero_i = live[pick[:k]], live[pick[k:2 * k]]
    if b1 != 0.0:
        m[cancel] = -(1.0 - b1) * g[cancel] * (1.0 + 1e-9 * rng.uniform(-1, 1, k)) / b1
    g[zero_i] = m[zero_i] = v[zero_i] = 0.0
    dead = np.flatnonzero(mask == 0)
    g[dead] = 1e5 + dead
    m[dead] = -(2e5 + dead)
    v[dead] = 3e5 + dead
    zero = np.zeros(n, dtype=bool)
    zero[zero_i] = True
    return theta, g, m, v, zero
