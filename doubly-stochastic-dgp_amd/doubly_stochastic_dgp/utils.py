"""reparameterize (utils.py:22-51) and BroadcastingLikelihood (utils.py:54-121) of the reference, on the device."""
import ctypes as C

import numpy as np

from . import settings


def reparameterize(mean, var, z, full_cov=False):
    """mean + z * sqrt(var + jitter) for the diagonal case (utils.py:40-41); var=None returns mean (utils.py:37-38)."""
    if var is None:
        return mean
    from . import _lib
    from .engine import Context, ptr
    ctx = Context.get()
    if full_cov:                                                  # utils.py:43-51
        mean = np.asarray(mean, dtype=np.float64)
        S, N, D = mean.shape
        m, v = ctx.to_device(mean), ctx.to_device(var)
        zz = ctx.to_device(np.broadcast_to(z, mean.shape))
        out = ctx.empty(S, N, D)
        _lib.check(ctx.lib.dsdgp_reparameterize_full(ctx.handle, ptr(m), ptr(v), ptr(zz), float(settings.jitter), N, D, S,
                                                     ptr(out)))
        ctx.sync()
        return out.cpu().numpy()
    m, v, zz = (ctx.to_device(np.broadcast_to(a, np.shape(mean))) for a in (mean, var, z))
    out = ctx.empty(*np.shape(mean))
    _lib.check(ctx.lib.dsdgp_reparameterize(ctx.handle, ptr(m), ptr(v), ptr(zz), float(settings.jitter), m.numel(),
                                            ptr(out)))
    ctx.sync()
    return out.cpu().numpy()


def mvhermgauss(H, D):
    """[UPSTREAM] gpflow.quadrature.mvhermgauss: the H**D tensor-product Gauss-Hermite nodes (H**D, D) and weights (H**D,)
    for the weight function exp(-|x|^2) (consumed by DGP_Quad, dgp.py:143-145)."""
    import itertools
    gh_x, gh_w = np.polynomial.hermite.hermgauss(int(H))
    x = np.array(list(itertools.product(*(gh_x,) * int(D))))
    w = np.prod(np.array(list(itertools.product(*(gh_w,) * int(D)))), axis=1)
    return x.reshape(int(H) ** int(D), int(D)), w


GUARD_SENTINEL = -7.25e77      # what the read-outs below fill their guard elements with


def _guarded(ctx, count, guard):
    buf = ctx.empty(count + guard)
    buf.fill_(GUARD_SENTINEL)
    return buf


def lik_elbo_readout(kind, p0, p1, mean, var, Y, w=1.0, weights=None, transposed=False, adjoints=True, ldt=None, guard=0):
    """dsdgp_lik_elbo_readout (verification aid): the training step's element-wise likelihood launch on (S, N, D) mean / var and (N, D)
    targets.  -> dict: part (blocks, 2); row-major form dmean, dvar (S, N, D); transposed form MBt, VBt (D, ldt), ldt = S N rounded up
    to 16 unless given.  guard > 0: every output buffer gets that many sentinel-filled elements behind it, returned as part_guard,
    dmean_guard, ... — untouched memory still reads GUARD_SENTINEL."""
    from . import _lib
    from .engine import Context, ptr
    ctx = Context.get()
    mean = np.asarray(mean, dtype=np.float64)
    S, N, D = mean.shape
    Y = np.asarray(Y, dtype=np.float64)
    if Y.shape != (N, D) or np.shape(var) != mean.shape:
        raise ValueError("mean, var must be (S, N, D) and Y (N, D)")
    m, v, y = ctx.to_device(mean), ctx.to_device(var), ctx.to_device(Y)
    sw = None
    if weights is not None:
        if np.shape(weights) != (S,):
            raise ValueError("sample weights must have shape (S,)")
        sw = ctx.to_device(np.asarray(weights, dtype=np.float64))
    R = S * N
    if ldt is None:
        ldt = -(-R // 16) * 16
    blocks = -(-(ldt * D if transposed else R * D) // 256)
    part = _guarded(ctx, 2 * blocks, guard)
    names = () if not adjoints and not transposed else (("MBt", "VBt") if transposed else ("dmean", "dvar"))
    bufs = [_guarded(ctx, ldt * D if transposed else R * D, guard) for _ in names]
    a, b = (bufs + [None, None])[:2]
    _lib.check(ctx.lib.dsdgp_lik_elbo_readout(ctx.handle, int(kind), float(p0), float(p1), ptr(m), ptr(v), ptr(y), N, S, D, float(w),
                                              ptr(sw), ptr(part), *((ptr(None), ptr(None), ptr(a), ptr(b)) if transposed else
                                                                    (ptr(a), ptr(b), ptr(None), ptr(None))), ldt))
    ctx.sync()
    out = {}
    for name, buf, shape in [("part", part, (blocks, 2))] + [(nm, bf, (D, ldt) if transposed else (S, N, D)) for nm, bf in zip(names, bufs)]:
        h = buf.cpu().numpy()
        out[name] = h[:h.size - guard].reshape(shape)
        if guard:
            out[name + "_guard"] = h[h.size - guard:]
    return out


def multiclass_readout(mean, var, Y, w=1.0, weights=None, guard=0):
    """dsdgp_multiclass_readout (verification aid): the training step's MultiClass launch (and the quadrature-weight launch behind it) on
    (S, N, K) mean / var and (N, 1) labels -> dict: ve (S, N), dmean, dvar (S, N, K) (+ *_guard as lik_elbo_readout).  The labels are
    checked here, before anything is uploaded: the kernel indexes its per-class accumulators with them."""
    from . import _lib
    from .engine import Context, ptr
    mean = np.asarray(mean, dtype=np.float64)
    S, N, K = mean.shape
    Y = np.asarray(Y, dtype=np.float64)
    if Y.shape != (N, 1) or np.shape(var) != mean.shape:
        raise ValueError(f"mean, var must be (S, N, K) and the labels (N, 1), got {Y.shape}")
    if not 2 <= K <= 32:
        raise ValueError(f"MultiClass: K = {K} outside [2, 32]")
    if not np.all(np.isfinite(Y)) or np.any(Y != np.floor(Y)) or np.any(Y < 0) or np.any(Y >= K):
        raise ValueError(f"MultiClass targets must be integer labels in [0, {K})")
    ctx = Context.get()
    m, v, y = ctx.to_device(mean), ctx.to_device(var), ctx.to_device(Y)
    sw = None
    if weights is not None:
        if np.shape(weights) != (S,):
            raise ValueError("sample weights must have shape (S,)")
        sw = ctx.to_device(np.asarray(weights, dtype=np.float64))
    R = S * N
    bufs = {"ve": _guarded(ctx, R, guard), "dmean": _guarded(ctx, R * K, guard), "dvar": _guarded(ctx, R * K, guard)}
    _lib.check(ctx.lib.dsdgp_multiclass_readout(ctx.handle, ptr(m), ptr(v), ptr(y), N, S, K, float(w), ptr(sw), ptr(bufs["ve"]),
                                                ptr(bufs["dmean"]), ptr(bufs["dvar"])))
    ctx.sync()
    out = {}
    for name, buf in bufs.items():
        h = buf.cpu().numpy()
        out[name] = h[:h.size - guard].reshape((S, N) if name == "ve" else (S, N, K))
        if guard:
            out[name + "_guard"] = h[h.size - guard:]
    return out


class BroadcastingLikelihood:
    """Wrapper giving every likelihood method (S,N,D) semantics with Y of shape (N,D) (utils.py:54-121): the Gaussian
    broadcasts Y[None]; every other likelihood is evaluated on the flattened (S*N, D) arrays with Y tiled S times
    (utils.py:76-86).  Evaluated by libdsdgp; `.likelihood` is the wrapped object
    (`model.likelihood.likelihood.variance`)."""

    def __init__(self, likelihood):
        self.likelihood = likelihood
        from . import _lib
        from .gpflow_compat import likelihood_entry
        kind = likelihood_entry(likelihood)[0]      # (a class outside gpflow_compat.LIKELIHOODS raises here)
        self.needs_broadcasting = kind != _lib.LIK_GAUSSIAN
        self.bernoulli = kind == _lib.LIK_BERNOULLI
        # Poisson / Exponential / Gamma (exp link), StudentT, Beta: elementwise like Bernoulli, evaluated by dsdgp_lik_var_exp / dsdgp_lik_predict
        self.generic = kind not in (_lib.LIK_GAUSSIAN, _lib.LIK_MULTICLASS, _lib.LIK_BERNOULLI)

    def generic_args(self):
        """(kind, p0, p1) of dsdgp_lik_var_exp / dsdgp_lik_predict: p0 = StudentT.scale / Gamma.shape / Beta.scale, p1 = Poisson.binsize /
        StudentT.deg_free."""
        return self.mixture_args()

    def mixture_args(self):
        """(kind, p0, p1) of dsdgp_eval_mixture for the wrapped likelihood (gpflow_compat.likelihood_args): p0 = the noise variance for
        the Gaussian, nothing for Bernoulli / MultiClass."""
        from .gpflow_compat import likelihood_args
        return likelihood_args(self.likelihood)

    def evaluate_mixture(self, Fmu, Fvar, Y, rows=False):
        """dsdgp_eval_mixture on (S, N, D) component means / variances and targets Y: the accumulator as a (3, D) array [squared error
        (MultiClass: misclassifications), log density, rows] summed over N, and with rows=True the (N, D, 3) per-row values
        [mixture mean, mixture variance, log density] as well."""
        self.check_targets(Y)
        from . import _lib
        from .engine import Context, ptr
        ctx = Context.get()
        Fmu = np.asarray(Fmu, dtype=np.float64)
        S, N, D = Fmu.shape
        m, v, y = ctx.to_device(Fmu), ctx.to_device(np.broadcast_to(Fvar, Fmu.shape)), ctx.to_device(Y)
        acc = ctx.empty(3, D)
        out = ctx.empty(N, D, 3) if rows else None
        kind, p0, p1 = self.mixture_args()
        _lib.check(ctx.lib.dsdgp_eval_mixture(ctx.handle, kind, p0, p1, ptr(m), ptr(v), ptr(y), N, S, D, ptr(out), ptr(acc), 0))
        ctx.sync()
        return (acc.cpu().numpy(), out.cpu().numpy()) if rows else acc.cpu().numpy()

    def _mixture_noise(self, level, what):
        if level not in ("f", "y"):
            raise ValueError(f"level must be \"f\" or \"y\", not {level!r}")
        if level == "f":
            return 0.0
        if self.needs_broadcasting:
            raise NotImplementedError(f"{what}: the predictive y of {type(self.likelihood).__name__} is not a mixture of Gaussians; "
                                      "only level=\"f\" is covered")
        return float(self.likelihood.variance.value)

    @staticmethod
    def _probs(probs):
        from . import _lib
        probs = np.ascontiguousarray(np.atleast_1d(np.asarray(probs, dtype=np.float64)))
        if probs.ndim != 1 or not 1 <= probs.size <= 16 or not np.all((probs > 0.0) & (probs < 1.0)):
            raise ValueError("probs must hold 1 .. 16 probabilities inside (0, 1)")
        return probs, probs.ctypes.data_as(_lib.c_double_p)

    def mixture_quantiles(self, Fmu, Fvar, probs, level="y"):
        """dsdgp_mixture_quantiles on (S, N, D) component means / variances: the (N, D, P) quantiles of the equally weighted mixture of
        N(Fmu_s, Fvar_s + noise), noise = the Gaussian likelihood's variance for level "y", 0 for level "f"."""
        noise = self._mixture_noise(level, "mixture_quantiles")
        probs, pp = self._probs(probs)
        from . import _lib
        from .engine import Context, ptr
        ctx = Context.get()
        Fmu = np.asarray(Fmu, dtype=np.float64)
        S, N, D = Fmu.shape
        m, v = ctx.to_device(Fmu), ctx.to_device(np.broadcast_to(Fvar, Fmu.shape))
        q = ctx.empty(N, D, probs.size)
        _lib.check(ctx.lib.dsdgp_mixture_quantiles(ctx.handle, ptr(m), ptr(v), noise, N, S, D, pp, probs.size, ptr(q)))
        ctx.sync()
        return q.cpu().numpy()

    def mixture_calibration(self, Fmu, Fvar, Y, probs, rows=False):
        """dsdgp_mixture_calibration on (S, N, D) component means / variances and targets Y (N, D), Gaussian likelihood: the accumulator
        as a (2 + P, D) array [sum of CRPS, rows, #(u <= p_0), ...] summed over N, and with rows=True the (N, D, 2) per-row values
        [u, CRPS] as well."""
        noise = self._mixture_noise("y", "mixture_calibration")
        probs, pp = self._probs(probs)
        from . import _lib
        from .engine import Context, ptr
        ctx = Context.get()
        Fmu = np.asarray(Fmu, dtype=np.float64)
        S, N, D = Fmu.shape
        if np.shape(Y) != (N, D):
            raise ValueError(f"Y has shape {np.shape(Y)}, expected {(N, D)}")
        m, v, y = ctx.to_device(Fmu), ctx.to_device(np.broadcast_to(Fvar, Fmu.shape)), ctx.to_device(Y)
        acc = ctx.empty(2 + probs.size, D)
        out = ctx.empty(N, D, 2) if rows else None
        _lib.check(ctx.lib.dsdgp_mixture_calibration(ctx.handle, ptr(m), ptr(v), noise, ptr(y), N, S, D, pp, probs.size, ptr(out),
                                                     ptr(acc), 0))
        ctx.sync()
        return (acc.cpu().numpy(), out.cpu().numpy()) if rows else acc.cpu().numpy()

    def classification_args(self, what):
        """(kind, C) of dsdgp_mixture_classification for the wrapped likelihood: MultiClass (C = num_classes) or Bernoulli (C = 2, one
        two-class problem per output); every other likelihood has no classes."""
        from . import _lib
        from .gpflow_compat import likelihood_entry
        kind, _, const = likelihood_entry(self.likelihood)
        if kind == _lib.LIK_BERNOULLI:
            return kind, 2
        if kind == _lib.LIK_MULTICLASS:
            return kind, int(const)
        raise NotImplementedError(f"{what}: {type(self.likelihood).__name__} has no classes; MultiClass and Bernoulli are covered")

    def mixture_classification(self, Fmu, Fvar, Y, bins=10, rows=False):
        """dsdgp_mixture_classification on (S, N, D) component means / variances and targets Y (MultiClass: (N, 1) labels, D = K;
        Bernoulli: (N, D), every output its own two-class problem): the accumulator as an (E, ND) array, E = 4 + 3 bins + C + C^2 and
        ND = 1 (MultiClass, C = K) or D (Bernoulli, C = 2), laid out as include/dsdgp.h documents (`dgp.classification_scores` turns it
        into the report), and with rows=True also the mixture class probabilities (N, D) (Bernoulli: p(y = 1)) and the (N, ND, 4)
        per-row values [predicted class, conf, l = log pi_y, brier].  brier is the multi-class sum_c (pi_c - [c = y])^2: a binary
        problem gives 2 (p - t)^2, twice the usual binary score."""
        kind, Cn = self.classification_args("mixture_classification")
        bins = int(bins)
        if not 1 <= bins <= 32:
            raise ValueError("bins must lie in 1 .. 32")
        self.check_targets(Y)
        from . import _lib
        from .engine import Context, ptr
        Fmu = np.asarray(Fmu, dtype=np.float64)
        S, N, D = Fmu.shape
        ND = D if self.bernoulli else 1
        if np.shape(Y) != (N, ND):
            raise ValueError(f"Y has shape {np.shape(Y)}, expected {(N, ND)}")
        if not self.bernoulli and D != Cn:
            raise ValueError(f"Fmu has {D} outputs, the likelihood {Cn} classes")
        ctx = Context.get()
        m, v, y = ctx.to_device(Fmu), ctx.to_device(np.broadcast_to(Fvar, Fmu.shape)), ctx.to_device(Y)
        acc = ctx.empty(4 + 3 * bins + Cn + Cn * Cn, ND)
        probs = ctx.empty(N, D) if rows else None
        out = ctx.empty(N, ND, 4) if rows else None
        _lib.check(ctx.lib.dsdgp_mixture_classification(ctx.handle, kind, ptr(m), ptr(v), ptr(y), N, S, D, bins, ptr(probs), ptr(out),
                                                        ptr(acc), 0))
        ctx.sync()
        return (acc.cpu().numpy(), probs.cpu().numpy(), out.cpu().numpy()) if rows else acc.cpu().numpy()

    def check_targets(self, Y):
        """MultiClass: Y must hold integer class labels in [0, num_classes) — the device kernel indexes its per-class
        accumulators with them ([UPSTREAM] tf.one_hot / gather would error or zero-fill; one-hot or NaN targets are a bug)."""
        if not self.needs_broadcasting:
            return
        Y = np.asarray(Y, dtype=np.float64)
        if self.bernoulli or self.generic:
            # [UPSTREAM] tf.where(tf.equal(Y, 1), p, 1 - p): any finite target is accepted (the reference test draws -1 / 1); the
            # count / positive-target likelihoods evaluate their log densities on whatever finite targets they are given, as upstream
            if Y.ndim != 2 or not np.all(np.isfinite(Y)):
                raise ValueError(f"{type(self.likelihood).__name__} targets must be a finite (N, D) array, got shape {Y.shape}")
            return
        K = self.likelihood.num_classes
        if Y.ndim != 2 or Y.shape[1] != 1:
            raise ValueError(f"MultiClass targets must have shape (N, 1) with labels in [0, {K}), got {Y.shape}")
        if not np.all(np.isfinite(Y)) or np.any(Y != np.floor(Y)) or np.any(Y < 0) or np.any(Y >= K):
            raise ValueError(f"MultiClass targets must be integer labels in [0, {K})")

    def _run(self, mode, Fmu, Fvar, Y, weights=None):
        self.check_targets(Y)
        from . import _lib
        from .engine import Context, ptr
        ctx = Context.get()
        Fmu = np.asarray(Fmu, dtype=np.float64)
        S, N, D = Fmu.shape
        m, v, y = ctx.to_device(Fmu), ctx.to_device(np.broadcast_to(Fvar, Fmu.shape)), ctx.to_device(Y)
        w = None
        if weights is not None:
            if mode != 0 or np.shape(weights) != (S,):
                raise ValueError("sample weights apply to the variational expectations and must have shape (S,)")
            w = ctx.to_device(np.asarray(weights, dtype=np.float64))
        wp = ptr(w) if w is not None else None
        if not self.needs_broadcasting:
            out = ctx.empty(N, D)
            lv = float(self.likelihood.variance.value)
            if mode == 0:
                _lib.check(ctx.lib.dsdgp_gauss_var_exp(ctx.handle, ptr(m), ptr(v), ptr(y), N, S, D, lv, wp, ptr(out)))
            else:
                _lib.check(ctx.lib.dsdgp_gauss_predict_density(ctx.handle, ptr(m), ptr(v), ptr(y), N, S, D, lv, ptr(out)))
        elif self.bernoulli:
            out = ctx.empty(N, D)
            _lib.check(ctx.lib.dsdgp_bernoulli_var_exp(ctx.handle, ptr(m), ptr(v), ptr(y), N, S, D, mode, wp, ptr(out)))
        elif self.generic:
            out = ctx.empty(N, D)
            kind, p0, p1 = self.generic_args()
            _lib.check(ctx.lib.dsdgp_lik_var_exp(ctx.handle, kind, p0, p1, ptr(m), ptr(v), ptr(y), N, S, D, mode, wp, ptr(out)))
        else:
            out = ctx.empty(N, 1)
            _lib.check(ctx.lib.dsdgp_multiclass_var_exp(ctx.handle, ptr(m), ptr(v), ptr(y), N, S, D, mode, wp, ptr(out)))
        ctx.sync()
        return out.cpu().numpy()

    def variational_expectations_mean(self, Fmu, Fvar, Y, weights=None):
        """reduce_mean over S of variational_expectations (dgp.py:89-90); with `weights` (S,) the weighted sum over S of
        DGP_Quad.E_log_p_Y (dgp.py:165-166)."""
        return self._run(0, Fmu, Fvar, Y, weights)

    def predict_density_logmeanexp(self, Fmu, Fvar, Y):
        """logsumexp_S(predict_density) - log S (dgp.py:124-126)."""
        return self._run(1, Fmu, Fvar, Y)

    def predict_mean_and_var(self, Fmu, Fvar):
        from . import _lib
        from .engine import Context, ptr
        ctx = Context.get()
        Fmu = np.asarray(Fmu, dtype=np.float64)
        v = ctx.to_device(np.broadcast_to(np.asarray(Fvar, dtype=np.float64), Fmu.shape))
        if not self.needs_broadcasting:
            out = ctx.empty(*v.shape)
            _lib.check(ctx.lib.dsdgp_add_scalar(ctx.handle, ptr(v), float(self.likelihood.variance.value), v.numel(),
                                                ptr(out)))
            ctx.sync()
            return Fmu, out.cpu().numpy()
        S, N, K = Fmu.shape
        m = ctx.to_device(Fmu)
        om, ov = ctx.empty(S, N, K), ctx.empty(S, N, K)
        if self.bernoulli:
            _lib.check(ctx.lib.dsdgp_bernoulli_predict(ctx.handle, ptr(m), ptr(v), S * N * K, ptr(om), ptr(ov)))
            ctx.sync()
            return om.cpu().numpy(), ov.cpu().numpy()
        if self.generic:
            kind, p0, p1 = self.generic_args()
            _lib.check(ctx.lib.dsdgp_lik_predict(ctx.handle, kind, p0, p1, ptr(m), ptr(v), S * N * K, ptr(om), ptr(ov)))
            ctx.sync()
            return om.cpu().numpy(), ov.cpu().numpy()
        _lib.check(ctx.lib.dsdgp_multiclass_predict(ctx.handle, ptr(m), ptr(v), S * N, K, ptr(om), ptr(ov)))
        ctx.sync()
        return om.cpu().numpy(), ov.cpu().numpy()
