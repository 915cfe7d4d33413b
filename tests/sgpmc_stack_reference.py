"""Reference of a stack of sparse sampled layers (dsdgp_stack_propagate, dsdgp_stack_logdensity, csrc/sgpmc_stack.hip; the reference's
DGP_Base over SGPMC_Layer, dgp.py:42-98 and layers.py:249-260) in numpy at a chosen precision: long double is the truth of
tests/test_gpu_sgpmc_stack.py, float64 the same operation sequence at the device's precision.  Every layer is
tests/sparse_cond_reference.py (`forward`, `reverse`); the likelihood terms are tests/likelihood_reference.py, evaluated with 40 digits
on the long-double inputs for the truth and in float64 numpy for the twin.

    row r = s n + i;  Xin_0 = X repeated S times;  per layer  (cm, var) = the sparse conditional of Xin_l,  Fmean = cm + m(Xin_l),
    F = [Xin_l[:, :p] | Fmean + z sqrt(var + jitter)] = Xin_{l+1};  the last layer is not sampled: F = Fmean.
    data = data_scale / S * sum_{r, d} ve(Fmean_L[r, d], var_L[r], Y[r mod n, d]),   prior = sum_l -1/2 sum q_mu_l^2 - 1/2 M_l DO_l log 2 pi
    reverse: gm_L = w dve/dmean, gv_L[r] = w sum_d dve/dvar;  per layer (descending) the sparse conditional's reverse pass, then
    dXin_l = d_X + (gm for Identity, gm A^T for Linear) + [dF[:, :p] | 0];  dF_{l-1} = dXin_l:  gm = dF[:, p:],
    gv_r = sum_o dF[r, p + o] z[r, o] / (2 sqrt(var_r + jitter)).

A case is a dict: `layers` (a list of dicts: kind, ard, white_var, white, M, D, DO, p, mean in {"zero", "identity", "linear"}, A, b, Z,
q_mu, variance, ls), X (n, D_0), Y, n, S, zs (a list, (R, DO_l) per sampled layer), jitter, data_scale, lik = (name, p0, p1)."""
import math

import numpy as np

from tests import likelihood_reference as LR
from tests import sparse_cond_reference as SR

LD = np.longdouble


class MPLD(LR.MP):
    """tests/likelihood_reference.py's 40-digit backend on long-double inputs: every long double is an exact sum of two float64"""
    name = "mpmath on long double"

    @classmethod
    def arr(cls, a):
        mpf = cls._mp().mpf
        a = np.asarray(a, dtype=LD)
        hi = a.astype(np.float64)
        lo = (a - hi.astype(LD)).astype(np.float64)
        return np.array([mpf(float(h)) + mpf(float(l)) for h, l in zip(hi.ravel(), lo.ravel())], dtype=object).reshape(a.shape)

    @classmethod
    def c(cls, x):
        return cls.arr(np.asarray(x, dtype=LD).reshape(1))[0]


def likelihood(lik, mean, var, Y, n, S, w, dtype, want_grad=True):
    """-> (data term w sum ve, gm (R, DY), gv (R,), d data / d p0) on the last layer's mean (R, DY) and its one variance column (R,)"""
    name, p0, p1 = lik
    B = MPLD if dtype is LD else LR.NPB
    R, DY = mean.shape
    varb = np.repeat(np.asarray(var, dtype=dtype)[:, None], DY, 1)
    w = dtype(w)
    if name == "multiclass":
        labels = np.tile(np.asarray(Y).reshape(n), S)
        r = LR.multiclass(B, mean, varb, labels, w=1.0) if dtype is not LD else _multiclass_ld(mean, varb, labels)
        ve = np.asarray(r["ve"][0], dtype=dtype)
        gm, gvar = -w * np.asarray(r["dmean"][0], dtype=dtype), -w * np.asarray(r["dvar"][0], dtype=dtype)
        return w * np.sum(ve), gm, np.sum(gvar, 1), dtype(0.0)
    Yt = np.tile(np.asarray(Y, dtype=np.float64), (S, 1))
    which = ("ve", "dmu", "dv", "dp0") if want_grad else ("ve",)
    r = LR.elementwise(B, name, mean, varb, Yt, p0=p0, p1=p1, which=which)
    ve = np.asarray(r["ve"][0], dtype=dtype)
    if not want_grad:
        return w * np.sum(ve), None, None, None
    gm, gvar = w * np.asarray(r["dmu"][0], dtype=dtype), w * np.asarray(r["dv"][0], dtype=dtype)
    return w * np.sum(ve), gm, np.sum(gvar, 1), w * np.sum(np.asarray(r["dp0"][0], dtype=dtype))


def _multiclass_ld(mean, varb, labels):
    """LR.multiclass rounds its inputs to float64 before anything else: the long-double truth is its first-order correction, the float64
    evaluation at the rounded inputs plus the adjoints times what the rounding dropped — the second-order remainder, 1e-32, is far
    below every bar.  (dmean / dvar themselves are left at the rounded inputs: their own change, 1e-16 relative, is what e64 holds.)"""
    m64, v64 = mean.astype(np.float64), varb.astype(np.float64)
    r = LR.multiclass(LR.MP, m64, v64, labels, w=1.0)
    dm, dv = np.asarray(r["dmean"][0], dtype=LD), np.asarray(r["dvar"][0], dtype=LD)      # adjoints of -ve
    ve = np.asarray(r["ve"][0], dtype=LD) - np.sum(dm * (mean - m64.astype(LD)) + dv * (varb - v64.astype(LD)), 1)
    return dict(r, ve=(ve, r["ve"][1]))


def mean_function(layer, Xin, dtype):
    if layer["mean"] == "identity":
        return Xin
    if layer["mean"] == "linear":
        return Xin @ np.asarray(layer["A"], dtype=dtype) + np.asarray(layer["b"], dtype=dtype)
    return None


def _cond_args(layer, Xin):
    return layer["kind"], layer["Z"], Xin, layer["q_mu"], layer["variance"], layer["ls"]


def propagate(case, dtype=LD):
    """-> dict: `Xin`, `F`, `Fmean`, `var`: lists over the layers ((R, .) arrays; var (R,)); F of the last layer is its Fmean"""
    n, S, jitter = case["n"], case["S"], dtype(case["jitter"])
    Xin = np.tile(np.asarray(case["X"], dtype=dtype), (S, 1))
    out = dict(Xin=[], F=[], Fmean=[], var=[])
    L = len(case["layers"])
    for l, layer in enumerate(case["layers"]):
        r, _ = SR.forward(*_cond_args(layer, Xin), layer["white_var"], case["jitter"], layer["white"], dtype=dtype)
        m = mean_function(layer, Xin, dtype)
        Fmean = r["mean"] if m is None else r["mean"] + m
        if l + 1 < L:
            z = np.asarray(case["zs"][l], dtype=dtype)
            F = np.concatenate([Xin[:, :layer["p"]], Fmean + z * np.sqrt(r["var"] + jitter)[:, None]], 1)
        else:
            F = Fmean
        out["Xin"].append(Xin), out["F"].append(F), out["Fmean"].append(Fmean), out["var"].append(r["var"])
        Xin = F
    return out


def log_prior(case, dtype=LD):
    tot = dtype(0.0)
    log2pi = LD("1.8378770664093454835606594728112353") if dtype is LD else dtype(math.log(2.0 * math.pi))
    for layer in case["layers"]:
        q = np.asarray(layer["q_mu"], dtype=dtype)
        tot = tot + (-dtype(0.5) * np.sum(q * q) - dtype(0.5) * q.size * log2pi)
    return tot


def logdensity(case, dtype=LD, want_grad=True):
    """-> dict: `value`, `data`, `prior`, and with want_grad `grads`: a list over the layers of dicts Z, q_mu, variance, lengthscales,
    diag (the prior's -q_mu added), and `lik`: the gradient in the likelihood's parameter (0 where it has none)"""
    n, S = case["n"], case["S"]
    fw = propagate(case, dtype)
    w = dtype(case["data_scale"]) / dtype(S)
    data, gm, gv, dlik = likelihood(case["lik"], fw["Fmean"][-1], fw["var"][-1], case["Y"], n, S, w, dtype, want_grad)
    prior = log_prior(case, dtype)
    out = dict(value=data + prior, data=data, prior=prior)
    if not want_grad:
        return out
    L = len(case["layers"])
    grads = [None] * L
    jitter = dtype(case["jitter"])
    for l in range(L - 1, -1, -1):
        layer = case["layers"][l]
        r, _ = SR.reverse(*_cond_args(layer, fw["Xin"][l]), layer["ard"], layer["white_var"], case["jitter"], layer["white"], gm, gv,
                          dtype=dtype)
        grads[l] = dict(Z=r["Z"], q_mu=r["q_mu"] - np.asarray(layer["q_mu"], dtype=dtype), variance=np.atleast_1d(r["variance"]),
                        lengthscales=np.atleast_1d(r["lengthscales"]), diag=np.atleast_1d(r["diag"]))
        if l == 0:
            break
        dX = r["X"]
        if layer["mean"] == "identity":
            dX = dX + gm
        elif layer["mean"] == "linear":
            dX = dX + gm @ np.asarray(layer["A"], dtype=dtype).T
        if l + 1 < L and layer["p"]:
            dX = dX.copy()
            dX[:, :layer["p"]] += dF[:, :layer["p"]]
        dF = dX                                         # the adjoint of layer l - 1's F
        low = case["layers"][l - 1]
        z = np.asarray(case["zs"][l - 1], dtype=dtype)
        gm = dF[:, low["p"]:]
        gv = np.sum(gm * z, 1) / (dtype(2.0) * np.sqrt(fw["var"][l - 1] + jitter))
    out["grads"], out["lik"] = grads, np.atleast_1d(dlik)
    return out


def flat_arrays(res):
    """{name: array} of everything `logdensity` returns, one entry per output array"""
    out = {k: np.atleast_1d(res[k]) for k in ("value", "data", "prior")}
    for l, g in enumerate(res.get("grads", [])):
        out.update({"l%d_%s" % (l, k): v for k, v in g.items()})
    if "lik" in res:
        out["lik"] = res["lik"]
    return out
