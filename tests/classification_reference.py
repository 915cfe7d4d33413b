"""CPU side of tests/test_gpu_classification.py: the classification report of the predictive mixture restated in numpy / scipy.

Components: class_probs gives, per mixture component s, the likelihood's predictive class probabilities — MultiClass from the oracle's
MultiClass.predict_mean_and_var (oracle/dgp_oracle.py: RobustMax, 20-point Gauss-Hermite), Bernoulli from the probit closed form
p = Phi(mu / sqrt(1 + v)) (1 - 2e-3) + 1e-3.  The mixture's probabilities are their mean over s:
  MultiClass: pi (N, K), one problem (ND = 1, C = K);  Bernoulli: p (N, D), every output its own problem (ND = D, C = 2), pi = (1 - p, p).
Per item (row i; Bernoulli: (i, d)) with label y (Bernoulli: 1 where the target equals 1, else 0):
  c^ = argmax_c pi_c (numpy.argmax: ties to the lowest c), conf = pi_c^, err = [c^ != y], l = log pi_y,
  brier = sum_c (pi_c - [c = y])^2  (the multi-class definition: a binary problem gives 2 (p - t)^2),
  rank = #{c: pi_c > pi_y} + #{c < y: pi_c == pi_y},  bin = min(B - 1, floor(conf B)).
rows = (N, ND, 4) of [c^, conf, l, brier]; sums = (E, ND), E = 4 + 3 B + C + C^2, laid out as include/dsdgp.h documents; scores = the
dict DGP_Base.classification_report returns."""
import numpy as np
from scipy.special import erf

from oracle import dgp_oracle as O

EPS = 1e-3


def class_probs(kind, mean, var):
    """(S, N, D) predictive class probabilities of every component (Bernoulli: p(y = 1))"""
    mean = np.asarray(mean, dtype=np.float64)
    var = np.broadcast_to(np.asarray(var, dtype=np.float64), mean.shape)
    if kind == "bernoulli":
        return 0.5 * (1.0 + erf(mean / np.sqrt(1.0 + var) / np.sqrt(2.0))) * (1.0 - 2e-3) + 1e-3
    return O.MultiClass(mean.shape[2]).predict_mean_and_var(O.NP, mean, var)[0]


def mixture_probs(kind, mean, var):
    """(N, D): the mean over the components"""
    return class_probs(kind, mean, var).mean(0)


def _one_multiclass_mp(mu, v):
    """the K class probabilities of one component in 30-digit mpmath (numpy's float64 nodes and weights taken as they are)"""
    import mpmath as mp
    K = len(mu)
    gx, gw = np.polynomial.hermite.hermgauss(20)
    mu, v = [mp.mpf(float(x)) for x in mu], [mp.mpf(float(x)) for x in v]
    isp = 1 / mp.sqrt(mp.pi)
    out = []
    for k in range(K):
        sy = mp.sqrt(2 * max(v[k], mp.mpf("0.5e-10")))
        pt = mp.mpf(0)
        for x, w in zip(gx, gw):
            X = mu[k] + mp.mpf(float(x)) * sy
            P = mp.mpf(1)
            for j in range(K):
                if j != k:
                    P *= (1 + mp.erf((X - mu[j]) / mp.sqrt(2 * max(v[j], mp.mpf("1e-10"))))) / 2 * (1 - mp.mpf("2e-4")) + mp.mpf("1e-4")
            pt += mp.mpf(float(w)) * isp * P
        out.append(float(pt * (1 - mp.mpf(EPS)) + (1 - pt) * mp.mpf(EPS) / (K - 1)))
    return out


def _one_multiclass_reordered(mu, v):
    """float64 with another order of every sum: nodes from the outside in (symmetric pairs), the product from the last class down,
    Phi through scipy's ndtr instead of erf"""
    from scipy.special import ndtr
    K = len(mu)
    gx, gw = np.polynomial.hermite.hermgauss(20)
    gw = gw / np.sqrt(np.pi)
    out = []
    for k in range(K):
        sy = np.sqrt(2.0 * max(v[k], 0.5e-10))
        terms = []
        for x, w in zip(gx, gw):
            X = mu[k] + x * sy
            P = 1.0
            for j in range(K - 1, -1, -1):
                if j != k:
                    P *= ndtr((X - mu[j]) / np.sqrt(max(v[j], 1e-10))) * (1.0 - 2e-4) + 1e-4
            terms.append(w * P)
        pt = 0.0
        for a in range(10):
            pt += terms[a] + terms[19 - a]
        out.append(pt * (1.0 - EPS) + (1.0 - pt) * EPS / (K - 1))
    return out


def independent_multiclass_probs(mean, var, erf_budget=12000):
    """A second, independent evaluation of the MultiClass component probabilities on a fixed-stride subsample of the (s, i) pairs, the
    first and the last among them: 30-digit mpmath where it is installed, else float64 with every sum in another order.  At most
    erf_budget erf evaluations (one (s, i) costs 20 K (K - 1)).  -> (flat indices into (S N), (len, K) probabilities, the method's name)"""
    mean = np.asarray(mean, dtype=np.float64)
    var = np.broadcast_to(np.asarray(var, dtype=np.float64), mean.shape)
    S, N, K = mean.shape
    m2, v2 = mean.reshape(S * N, K), var.reshape(S * N, K)
    want = max(2, erf_budget // (20 * K * (K - 1)))
    idx = np.arange(S * N) if S * N <= want else np.unique(np.r_[np.arange(0, S * N, -(-S * N // (want - 1))), S * N - 1])
    try:
        import mpmath  # noqa: F401
        one, name = _one_multiclass_mp, "mpmath, 30 digits"
    except ImportError:
        one, name = _one_multiclass_reordered, "float64, reordered sums"
    return idx, np.array([one(m2[r], v2[r]) for r in idx]), name


def labels(kind, Y, C):
    """(N, ND) integer class of every item: MultiClass labels clamped into 0 .. C - 1, Bernoulli 1 where the target equals 1"""
    Y = np.asarray(Y, dtype=np.float64)
    if kind == "bernoulli":
        return (Y == 1.0).astype(np.int64)
    return np.clip(Y, 0, C - 1).astype(np.int64)


def item_probs(kind, pbar):
    """(N, ND, C) class probabilities of every item"""
    if kind == "bernoulli":
        return np.stack([1.0 - pbar, pbar], axis=-1)
    return pbar[:, None, :]


def item_values(kind, pbar, Y, bins):
    """-> dict of (N, ND) arrays: pred, conf, l, brier, rank, bin, y"""
    pi = item_probs(kind, pbar)
    C = pi.shape[2]
    y = labels(kind, Y, C)
    pred = np.argmax(pi, axis=2)
    conf = np.take_along_axis(pi, pred[..., None], 2)[..., 0]
    piy = np.take_along_axis(pi, y[..., None], 2)[..., 0]
    onehot = (np.arange(C) == y[..., None]).astype(np.float64)
    brier = ((pi - onehot) ** 2).sum(2)
    c = np.arange(C)
    rank = ((pi > piy[..., None]) | ((pi == piy[..., None]) & (c < y[..., None]))).sum(2)
    b = np.minimum(bins - 1, np.floor(conf * bins).astype(np.int64))
    return dict(pred=pred, conf=conf, l=np.log(piy), brier=brier, rank=rank, bin=b, y=y)


def rows(kind, pbar, Y, bins=10):
    v = item_values(kind, pbar, Y, bins)
    return np.stack([v["pred"].astype(np.float64), v["conf"], v["l"], v["brier"]], axis=-1)


def sums(kind, pbar, Y, bins):
    """(E, ND) accumulator"""
    v = item_values(kind, pbar, Y, bins)
    N, ND = v["pred"].shape
    C = 2 if kind == "bernoulli" else pbar.shape[1]
    B = bins
    out = np.zeros((4 + 3 * B + C + C * C, ND))
    ok = v["pred"] == v["y"]
    out[0] = (~ok).sum(0)
    out[1] = v["l"].sum(0)
    out[2] = v["brier"].sum(0)
    out[3] = N
    for b in range(B):
        inb = v["bin"] == b
        out[4 + b] = inb.sum(0)
        out[4 + B + b] = np.where(inb, v["conf"], 0.0).sum(0)
        out[4 + 2 * B + b] = (inb & ok).sum(0)
    for r in range(C):
        out[4 + 3 * B + r] = (v["rank"] == r).sum(0)
    for t in range(C):
        for c in range(C):
            out[4 + 3 * B + C + t * C + c] = ((v["y"] == t) & (v["pred"] == c)).sum(0)
    return out


def count_rows(bins, C):
    """indices q of the accumulator that hold exact integers"""
    B = bins
    return np.r_[0, 3, 4:4 + B, 4 + 2 * B:4 + 3 * B + C + C * C]


def value_rows(bins):
    """indices q that hold floating-point sums: l, brier, confidence per bin"""
    return np.r_[1, 2, 4 + bins:4 + 2 * bins]


def scores(s, bins, C):
    """the dict DGP_Base.classification_report returns (without n, probs, rows), written out independently of the package"""
    B = bins
    s = np.asarray(s, dtype=np.float64)
    ND = s.shape[1]
    n = s[3].sum()

    def rel(bc, bcf, bok):
        cf, ok = np.full(B, np.nan), np.full(B, np.nan)
        ece, mce = 0.0, 0.0
        for b in range(B):
            if bc[b] > 0:
                cf[b], ok[b] = bcf[b] / bc[b], bok[b] / bc[b]
                ece += bc[b] / bc.sum() * abs(ok[b] - cf[b])
                mce = max(mce, abs(ok[b] - cf[b]))
        return cf, ok, ece, mce

    per_out = [rel(s[4:4 + B, d], s[4 + B:4 + 2 * B, d], s[4 + 2 * B:4 + 3 * B, d]) for d in range(ND)]
    pooled = rel(s[4:4 + B].sum(1), s[4 + B:4 + 2 * B].sum(1), s[4 + 2 * B:4 + 3 * B].sum(1))
    conf = s[4 + 3 * B + C:].reshape(C, C, ND).astype(np.int64).transpose(2, 0, 1)      # (ND, true, predicted)
    out = {"error_rate": s[0].sum() / n, "log_density": s[1].sum() / n, "brier": s[2].sum() / n, "ece": pooled[2], "mce": pooled[3],
           "top_k_accuracy": np.cumsum(s[4 + 3 * B:4 + 3 * B + C].sum(1)) / n}
    with np.errstate(divide="ignore", invalid="ignore"):
        diag = np.stack([np.diag(c) for c in conf])
        per_class = {"recall": diag / conf.sum(2), "precision": diag / conf.sum(1), "support": conf.sum(2)}
    relia = {"edges": np.linspace(0.0, 1.0, B + 1), "count": s[4:4 + B].T.astype(np.int64), "confidence": np.stack([p[0] for p in per_out]),
             "accuracy": np.stack([p[1] for p in per_out])}
    if ND == 1:
        out.update(confusion=conf[0], per_class={k: v[0] for k, v in per_class.items()}, reliability={k: (v if k == "edges" else v[0])
                                                                                                      for k, v in relia.items()})
    else:
        out.update(confusion=conf, per_class=per_class, reliability=relia, error_rate_per_output=s[0] / s[3],
                   log_density_per_output=s[1] / s[3], brier_per_output=s[2] / s[3], ece_per_output=np.array([p[2] for p in per_out]))
    return out


def margins(kind, pbar, Y, bins):
    """For every item: the gap between the two largest probabilities, the distance of conf B from the nearest integer, the smallest
    |pi_c - pi_y| over c != y.  While all three exceed a bound, a perturbation of the probabilities below that bound (conf B: B times
    it) can flip neither the predicted class, nor the bin, nor the rank.  -> three (N, ND) arrays"""
    pi = item_probs(kind, pbar)
    C = pi.shape[2]
    y = labels(kind, Y, C)
    srt = np.sort(pi, axis=2)
    top = srt[..., -1] - srt[..., -2]
    cb = srt[..., -1] * bins
    binm = np.abs(cb - np.rint(cb))
    piy = np.take_along_axis(pi, y[..., None], 2)
    d = np.abs(pi - piy)
    d[np.arange(C) == y[..., None]] = np.inf
    return top, binm, d.min(2)
