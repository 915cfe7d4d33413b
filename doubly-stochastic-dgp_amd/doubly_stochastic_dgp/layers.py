"""Host mirror of the reference's layer classes (layers.py:36-246): `Layer`, `SVGP_Layer` with the same constructor,
attributes (`q_mu`, `q_sqrt`, `feature.Z`, `kern`, `mean_function`, `num_outputs`, `white`) and methods
(`conditional_ND`, `conditional_SND`, `sample_from_conditional`, `KL`), of the collapsed layers `Collapsed_Layer`, `SGPR_Layer`
(layers.py:296-307, 345-367, 371-525), of the dense layers `GPMC_Layer`, `GPR_Layer` (layers.py:263-293, 310-342) and of the sparse
sampled layer `SGPMC_Layer` (layers.py:249-260).  All arithmetic runs in libdsdgp (HIP)."""
import ctypes as C

import numpy as np

from . import _lib, settings
from .engine import Context, Engine, ptr
from .gpflow_compat import Gaussian, InducingPoints, Parameter, Parameterized, split_kernel
from .utils import reparameterize


def _host_K_symm(kern, Z):
    """kern.compute_K_symm(Z) for the one-off q(u)=p(u) initialisation (layers.py:160-163); the reference does this
    step on the host with numpy too."""
    stat, white = split_kernel(kern)
    ls = np.asarray(stat.lengthscales._value, dtype=np.float64)
    Zs = Z / ls
    d = Zs[:, None, :] - Zs[None, :, :]
    r2 = np.sum(d * d, -1)
    var = float(stat.variance._value)
    if stat.kind == "rbf":
        K = var * np.exp(-0.5 * r2)
    else:
        r = np.sqrt(r2 + 1e-12)
        K = var * (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r2) * np.exp(-np.sqrt(5.0) * r)
    if white is not None:
        K = K + float(white.variance._value) * np.eye(Z.shape[0])
    return K


def concat_input_prop(X, p, samples, mean, var, full_cov=False):
    """layers.py:105-117: prepend the propagated inputs X[..., :p] to the samples and means, and zeros to the variances
    (pure copies — no arithmetic)."""
    X_prop = X[:, :, :p]
    samples = np.concatenate([X_prop, samples], 2)
    mean = np.concatenate([X_prop, mean], 2)
    if full_cov:
        zeros = np.zeros(var.shape[:3] + (p,))
        var = np.concatenate([zeros, var], 3)
    else:
        var = np.concatenate([np.zeros_like(X_prop), var], 2)
    return samples, mean, var


def prepend_input_prop(X, layers, Fs, Fmeans, Fvars):
    """concat_input_prop layer by layer, in place on the lists of per-layer device results: the device hands the concatenated
    [X_prop | F] to the next layer itself, the returned lists get the same copies prepended here.  X: the tiled (S, N, D_in) input."""
    for l, layer in enumerate(layers):
        if layer.input_prop_dim:
            Fs[l], Fmeans[l], Fvars[l] = concat_input_prop(X, layer.input_prop_dim, Fs[l], Fmeans[l], Fvars[l])
        X = Fs[l]


def propagate_layers(layers, F, zs=None, full_cov=False):
    """The layer loop of dgp.py:69-74 on the host, from the tiled (S, N, D_in) input F -> Fs, Fmeans, Fvars.  Every piece of arithmetic
    is a libdsdgp call (the layers' conditionals, utils.reparameterize); zs: a draw (or None) per layer."""
    Fs, Fmeans, Fvars = [], [], []
    for layer, z in zip(layers, zs or [None] * len(layers)):
        F, Fmean, Fvar = layer.sample_from_conditional(F, z=z, full_cov=full_cov)
        Fs.append(F); Fmeans.append(Fmean); Fvars.append(Fvar)
    return Fs, Fmeans, Fvars


def layer_parameters(layer, mean=True):
    """[(Parameter, key), ...] of what a layer owns, in the order of the engine's layout (trainable or not): `Z`, `q_mu`, `q_sqrt`, the
    kernel's `variance` and `lengthscales`, a White part's `white_variance`, and with `mean` the `A`, `b` of a Linear mean that is not a
    fixed map.  What a layer does not have (a dense layer's Z, a sampled layer's q_sqrt) is left out.  Host only."""
    stat, wk = split_kernel(layer.kern)
    out = [(layer.feature.Z, "Z")] if getattr(layer, "feature", None) is not None else []
    out += [(p, k) for k in ("q_mu", "q_sqrt") for p in [getattr(layer, k, None)] if p is not None]
    out += [(stat.variance, "variance"), (stat.lengthscales, "lengthscales")] + ([(wk.variance, "white_variance")] if wk is not None else [])
    mf = layer.mean_function
    if mean and getattr(mf, "kind", None) == "linear" and mf.in_theta():
        out += [(mf.A, "A"), (mf.b, "b")]
    return out


def _refuse_trainable_mean(mean_function, what):
    if getattr(mean_function, "kind", None) == "linear" and (mean_function.A.trainable or mean_function.b.trainable):
        raise NotImplementedError(f"{what}: a trainable Linear mean function — the gradients of its A and b are not "
                                  "formed; fix it with set_trainable(False)")


def _log_prior(layer):
    """the standard-normal prior of q_mu (layers.py:257, 272): -1/2 sum q_mu^2 - 1/2 (rows x outputs) log(2 pi)"""
    q = layer.q_mu.value
    return float(-0.5 * np.sum(q * q) - 0.5 * q.size * np.log(2.0 * np.pi))


class Layer(Parameterized):
    _no_owner = "a layer outside a model owns no random numbers: pass z to sample_from_conditional"

    def __init__(self, input_prop_dim=None, **kwargs):
        """input_prop_dim: the first dimensions of X to propagate (layers.py:36-50); None = no input propagation."""
        self.input_prop_dim = input_prop_dim

    def conditional_ND(self, X, full_cov=False):
        raise NotImplementedError

    def KL(self):
        return 0.0

    def _engine(self):
        """where sample_from_conditional draws when it is given no z: the owning model (its `randn`, under its seeds)"""
        ref = getattr(self, "_model", None)          # a weak reference: the model is not one of the layer's parameters
        model = ref() if ref is not None else None
        if model is None:
            raise RuntimeError(self._no_owner)
        return model

    # layers.py:52-74
    def conditional_SND(self, X, full_cov=False):
        X = np.asarray(X, dtype=np.float64)
        if full_cov:                                              # tf.map_fn over S, layers.py:66-69
            ms, vs = zip(*[self.conditional_ND(X[s], full_cov=True) for s in range(X.shape[0])])
            return np.stack(ms), np.stack(vs)
        S, N, D = X.shape
        mean, var = self.conditional_ND(X.reshape(S * N, D))
        return mean.reshape(S, N, self.num_outputs), var.reshape(S, N, self.num_outputs)

    # layers.py:76-119
    def sample_from_conditional(self, X, z=None, full_cov=False):
        mean, var = self.conditional_SND(X, full_cov=full_cov)
        if z is None:
            z = self._engine().randn(mean.shape)
        z = np.broadcast_to(np.asarray(z, dtype=np.float64), mean.shape)
        samples = reparameterize(mean, var, z, full_cov=full_cov)
        if self.input_prop_dim:                                   # layers.py:105-117
            samples, mean, var = concat_input_prop(np.asarray(X, dtype=np.float64), self.input_prop_dim, samples, mean, var,
                                                   full_cov)
        return samples, mean, var


class SVGP_Layer(Layer):
    def __init__(self, kern, Z, num_outputs, mean_function, white=False, input_prop_dim=None, **kwargs):
        Layer.__init__(self, input_prop_dim, **kwargs)
        Z = np.array(Z, dtype=np.float64)
        self.num_inducing = Z.shape[0]
        self.q_mu = Parameter(np.zeros((self.num_inducing, num_outputs)))                     # layers.py:146-147
        q_sqrt = np.tile(np.eye(self.num_inducing)[None, :, :], [num_outputs, 1, 1])          # layers.py:149
        self.q_sqrt = Parameter(q_sqrt, transform="tril")
        self.feature = InducingPoints(Z)
        self.kern = kern
        self.mean_function = mean_function
        self.num_outputs = int(num_outputs)
        self.white = bool(white)
        if not self.white:                                                                    # layers.py:160-163
            Ku = _host_K_symm(kern, Z)
            Lu = np.linalg.cholesky(Ku + np.eye(Z.shape[0]) * settings.jitter)
            self.q_sqrt = np.tile(Lu[None, :, :], [num_outputs, 1, 1])
        object.__setattr__(self, "_standalone_engine", None)
        object.__setattr__(self, "_model_engine", None)     # (engine, index) once owned by a DGP_Base

    def _engine(self):
        if self._model_engine is not None:
            return self._model_engine[0]
        if self._standalone_engine is None:
            object.__setattr__(self, "_standalone_engine", Engine([self], Gaussian(), self.white))
        return self._standalone_engine

    def _index(self):
        return self._model_engine[1] if self._model_engine is not None else 0

    # layers.py:178-219
    def conditional_ND(self, X, full_cov=False):
        eng = self._engine()
        if full_cov:                                              # layers.py:206-209: var is (N, N, D_out)
            mean, var = eng.layer_conditional_full(self._index(), np.asarray(X, dtype=np.float64))
            eng.ctx.sync()
            return mean.cpu().numpy(), var.cpu().numpy()
        mean, var = eng.layer_conditional(self._index(), np.asarray(X, dtype=np.float64))
        eng.ctx.sync()
        return mean.cpu().numpy(), var.cpu().numpy()

    # layers.py:221-246
    def KL(self):
        return self._engine().layer_kl(self._index())


def _rbf_spec(kern, what):
    """(KernelSpec, its lengthscale array — keep it alive) of a plain RBF kernel; NotImplementedError, saying why, for any other"""
    stat, white = split_kernel(kern)
    if stat.kind != "rbf" or white is not None:
        raise NotImplementedError(f"{what}: the expectations of the kernel under a Gaussian input have a closed form here for a "
                                  f"plain RBF kernel only, not for {type(stat).__name__}" + (" + White" if white is not None else ""))
    ls = np.ascontiguousarray(np.asarray(stat.lengthscales.value, dtype=np.float64).reshape(-1))
    spec = _lib.KernelSpec(kind=_lib.KERN_RBF, input_dim=int(stat.input_dim), ard=int(stat.ARD), has_white=0,
                           variance=float(stat.variance.value), white_variance=0.0, lengthscales=ls.ctypes.data_as(_lib.c_double_p))
    return spec, ls


def _expectation_inputs(what, kern, Z, X_mean, X_var):
    """(context, KernelSpec, its lengthscale array, Z, X_mean, X_var) of kernel_expectations[_grad]: float64 device tensors, shapes checked"""
    spec, ls = _rbf_spec(kern, what)
    ctx = Context.get()
    Zd, mu, s = ctx.as_device(Z), ctx.as_device(X_mean), None if X_var is None else ctx.as_device(X_var)
    if mu.dim() != 2 or Zd.dim() != 2 or mu.shape[1] != spec.input_dim or Zd.shape[1] != spec.input_dim or \
            (s is not None and tuple(s.shape) != tuple(mu.shape)):
        raise ValueError(f"{what}: Z must be (M, D), X_mean and X_var (N, D), D the kernel's input_dim")
    return ctx, spec, ls, Zd, mu, s


def _to_host(ctx, res, scalars):
    """the dict of device tensors res, once the device is done: numpy arrays, and numbers under the keys in scalars"""
    ctx.sync()
    return {k: float(v.cpu().numpy()[0]) if k in scalars else v.cpu().numpy() for k, v in res.items()}


def kernel_expectations(kern, Z, X_mean, X_var=None, on_device=False):
    """The expectations of an RBF kernel under the diagonal Gaussians N(X_mean[n], diag(X_var[n])) — GPflow 1.1.1's
    expectation(DiagonalGaussian, kern), expectation(DiagonalGaussian, (kern, Z)) and the sum over rows of
    expectation(DiagonalGaussian, (kern, Z), (kern, Z)) as layers.py:415-417 uses them — on the device (dsdgp_rbf_expectations):
    (psi0 scalar, psi1 (N, M), psi2 (M, M)).  Z (M, D), X_mean, X_var (N, D): numpy arrays or device tensors; X_var=None is zero
    variance.  on_device: return device tensors (psi0 of shape (1,)) without waiting for them.  The same arguments give the same bits."""
    ctx, spec, ls, Zd, mu, s = _expectation_inputs("kernel_expectations", kern, Z, X_mean, X_var)
    N, M = mu.shape[0], Zd.shape[0]
    psi0, psi1, psi2 = ctx.empty(1), ctx.empty(N, M), ctx.empty(M, M)
    _lib.check(ctx.lib.dsdgp_rbf_expectations(ctx.handle, C.byref(spec), ptr(Zd), M, ptr(mu), ptr(s), N, ptr(psi0), ptr(psi1), M,
                                              ptr(psi2), M))
    if on_device:
        return psi0, psi1, psi2
    ctx.sync()
    return float(psi0.cpu().numpy()[0]), psi1.cpu().numpy(), psi2.cpu().numpy()


def kernel_expectations_grad(kern, Z, X_mean, X_var, g_psi0, g_psi1, g_psi2, on_device=False):
    """The reverse pass of `kernel_expectations` (dsdgp_rbf_expectations_grad): given the adjoints g_psi0 (a number), g_psi1 (N, M) and
    g_psi2 (M, M; need not be symmetric) of a scalar F — either matrix may be None: zero — the gradients of F as a dict
    `X_mean`, `X_var` (N, D), `Z` (M, D), `variance` (a number), `lengthscales` (D entries with ARD, else one).  X_var=None is zero
    variance; `X_var` is then the derivative at zero variance.  Arguments as for `kernel_expectations`; on_device: device tensors
    (`variance` of shape (1,)) without waiting for them.  The same arguments give the same bits."""
    ctx, spec, ls, Zd, mu, s = _expectation_inputs("kernel_expectations_grad", kern, Z, X_mean, X_var)
    g1 = None if g_psi1 is None else ctx.as_device(g_psi1)
    g2 = None if g_psi2 is None else ctx.as_device(g_psi2)
    N, M, D = mu.shape[0], Zd.shape[0], mu.shape[1]
    if (g1 is not None and tuple(g1.shape) != (N, M)) or (g2 is not None and tuple(g2.shape) != (M, M)):
        raise ValueError("kernel_expectations_grad: g_psi1 must be (N, M) and g_psi2 (M, M)")
    d_mu, d_s, d_Z, d_k = ctx.empty(N, D), ctx.empty(N, D), ctx.empty(M, D), ctx.empty(kernel_grad_size(spec, False))
    _lib.check(ctx.lib.dsdgp_rbf_expectations_grad(ctx.handle, C.byref(spec), ptr(Zd), M, ptr(mu), ptr(s), N, float(g_psi0), ptr(g1), M,
                                                   ptr(g2), M, ptr(d_mu), ptr(d_s), ptr(d_Z), ptr(d_k)))
    variance, lengthscales, _ = cut_kernel_grad(spec, d_k)
    out = dict(X_mean=d_mu, X_var=d_s, Z=d_Z, variance=variance, lengthscales=lengthscales)
    return out if on_device else _to_host(ctx, out, ("variance",))


def kernel_grad_size(spec, diag):
    """the entries of a kernel's gradient block: variance, lengthscales (D with ARD, else one) and, with `diag`, a trailing diagonal entry"""
    return 1 + (int(spec.input_dim) if spec.ard else 1) + int(bool(diag))


def cut_kernel_grad(spec, d_k):
    """(variance, lengthscales, the trailing diagonal entry — empty where the block has none) of the kernel gradient block d_k"""
    nls = kernel_grad_size(spec, False) - 1
    return d_k[:1], d_k[1:1 + nls], d_k[1 + nls:]


_KERN_KIND = {"rbf": _lib.KERN_RBF, "matern52": _lib.KERN_MATERN52}


def _kernel_spec(kern):
    """(KernelSpec, its lengthscale array — keep it alive) of an RBF or Matern52 kernel, with or without a White part, at the
    kernel's current values"""
    stat, white = split_kernel(kern)
    ls = np.ascontiguousarray(np.asarray(stat.lengthscales.value, dtype=np.float64).reshape(-1))
    spec = _lib.KernelSpec(kind=_KERN_KIND[stat.kind], input_dim=int(stat.input_dim), ard=int(stat.ARD), has_white=int(white is not None),
                           variance=float(stat.variance.value), white_variance=float(white.variance.value) if white is not None else 0.0,
                           lengthscales=ls.ctypes.data_as(_lib.c_double_p))
    return spec, ls


def kernel_gram_grad(kern, X, X2, G, on_device=False):
    """The reverse pass of the kernel's Gram matrix (dsdgp_gram_grad): G is the adjoint, for a scalar F, of K(X, X2) (N, N2) — or, with
    X2=None, of K(X, X) + diag I (N, N; G need not be symmetric), diag the White variance plus any jitter.  Returns the gradients of F as
    a dict: `X` (N, D), `X2` (N2, D; None with X2=None), `variance` (a number), `lengthscales` (D entries with ARD, else one) and `diag`
    (a number): the gradient in what is added to the diagonal — the White variance, a jitter, a noise variance — sum_i G_ii with X2=None,
    0 otherwise.  kern: RBF or Matern52 (input_dim <= 32), with or without a White part.  X, X2, G: numpy arrays or device tensors;
    on_device: return device tensors (the numbers of shape (1,)) without waiting for them.  The same arguments give the same bits."""
    spec, ls = _kernel_spec(kern)
    ctx = Context.get()
    Xd, Gd = ctx.as_device(X), ctx.as_device(G)
    X2d = None if X2 is None else ctx.as_device(X2)
    D = int(spec.input_dim)
    if Xd.dim() != 2 or Xd.shape[1] != D or (X2d is not None and (X2d.dim() != 2 or X2d.shape[1] != D)) or \
            tuple(Gd.shape) != (Xd.shape[0], Xd.shape[0] if X2d is None else X2d.shape[0]):
        raise ValueError("kernel_gram_grad: X must be (N, D), X2 (N2, D) or None, G (N, N2) — (N, N) with X2=None — D the kernel's input_dim")
    d_X, d_X2, d_k = ctx.empty(Xd.shape[0], D), None if X2d is None else ctx.empty(X2d.shape[0], D), ctx.empty(kernel_grad_size(spec, True))
    ctx.gram_grad(spec, Xd, X2d, Gd, d_X, d_X2, d_k)
    variance, lengthscales, diag = cut_kernel_grad(spec, d_k)
    out = dict(X=d_X, variance=variance, lengthscales=lengthscales, diag=diag)
    if d_X2 is not None:
        out["X2"] = d_X2
    out = out if on_device else _to_host(ctx, out, ("variance", "diag"))
    out.setdefault("X2", None)
    return out


def _mean_on_device(ctx, mean_function, X, num_outputs):
    """m(X) as a device tensor (N, num_outputs), None for Zero: Identity is X itself, Linear one dsdgp_gemm plus its bias"""
    kind = getattr(mean_function, "kind", None)
    if kind == "zero":
        return None
    if kind == "identity":
        if X.shape[1] != num_outputs:
            raise ValueError(f"an Identity mean function needs as many outputs as inputs, not {X.shape[1]} -> {num_outputs}")
        return X
    if kind == "linear":
        A, b = ctx.to_device(mean_function.A.value), ctx.to_device(mean_function.b.value)
        if tuple(A.shape) != (X.shape[1], num_outputs):
            raise ValueError(f"Linear mean function: A is {tuple(A.shape)}, the layer maps {X.shape[1]} -> {num_outputs}")
        out = ctx.empty(X.shape[0], num_outputs)
        ctx.gemm(0, 0, 1.0, X, A, 0.0, out)
        return out + b
    raise NotImplementedError(f"mean function {type(mean_function).__name__}: Zero, Identity and Linear are on the dense layers' path")


class GPMC_Layer(Layer):
    """A dense layer with fixed inputs, sampled rather than optimised (layers.py:263-293): the latent values at the training inputs X
    are f = Lu q_mu + m(X) with Lu = chol(K(X, X) + jitter I) and a standard-normal prior on the whitened `q_mu` (N, num_outputs).  X
    does not change and must be the model's inputs: no minibatches.  Lu is computed ONCE, at construction, on the device
    (dsdgp_gram, dsdgp_potrf; `settings.jitter`) and is a constant afterwards, as in the reference (layers.py:278-279): the layer's
    own kernel hyper-parameters therefore have no gradient, and changing them later does not change Lu."""
    white = True
    _no_owner = "a GPMC_Layer outside a DGP_Heinonen owns no random numbers: pass z to sample_from_conditional"

    def __init__(self, kern, X, num_outputs, mean_function, input_prop_dim=None, **kwargs):
        Layer.__init__(self, input_prop_dim, **kwargs)
        X = np.array(X, dtype=np.float64)
        self.num_data = X.shape[0]
        self.q_mu = Parameter(np.zeros((self.num_data, int(num_outputs))))
        self.kern = kern
        self.mean_function = mean_function
        self.num_outputs = int(num_outputs)
        self.X = X
        ctx = Context.get()
        spec, ls = _kernel_spec(kern)
        Xd, Lu = ctx.to_device(X), ctx.empty(self.num_data, self.num_data)
        ctx.gram(spec, Xd, None, settings.jitter, Lu)
        ctx.potrf(Lu)
        object.__setattr__(self, "_dev", dict(ctx=ctx, spec=spec, ls=ls, X=Xd, Lu=Lu))

    log_prior = _log_prior

    def build_latents(self, on_device=False):
        """f = Lu q_mu + m(X) (N, num_outputs), the propagated columns X[:, :input_prop_dim] prepended (layers.py:282-287)"""
        d = self._dev
        ctx, p = d["ctx"], self.input_prop_dim
        f = ctx.empty(self.num_data, self.num_outputs)
        ctx.gemm(0, 0, 1.0, d["Lu"], ctx.to_device(self.q_mu.value), 0.0, f)
        m = _mean_on_device(ctx, self.mean_function, d["X"], self.num_outputs)
        if m is not None:
            f = f + m
        if p:
            f = ctx.torch.cat([d["X"][:, :p], f], 1).contiguous()
        if on_device:
            return f
        ctx.sync()
        return f.cpu().numpy()

    def latents_vjp(self, dF, on_device=False):
        """The adjoint of q_mu given the adjoint dF of build_latents(): Lu^T dF (one dsdgp_gemm); the adjoints of the propagated columns,
        which are copies of the fixed inputs, are dropped."""
        d = self._dev
        ctx, p = d["ctx"], self.input_prop_dim or 0
        dF = ctx.as_device(dF)
        if tuple(dF.shape) != (self.num_data, p + self.num_outputs):
            raise ValueError(f"latents_vjp: dF must be {(self.num_data, p + self.num_outputs)}")
        dF = dF[:, p:].contiguous()
        out = ctx.empty(self.num_data, self.num_outputs)
        ctx.gemm(1, 0, 1.0, d["Lu"], dF, 0.0, out)
        if on_device:
            return out
        ctx.sync()
        return out.cpu().numpy()

    def conditional_ND(self, Xnew, full_cov=False):
        """The whitened conditional without q_sqrt (layers.py:289-293): mean = K(Xnew, X) Lu^-T q_mu + m(Xnew), variance = Kdiag -
        colsum((Lu^-1 K(X, Xnew))^2) for every output; full_cov: K(Xnew, Xnew) - A^T A as (N*, N*, num_outputs), the layout
        Layer.sample_from_conditional takes."""
        d = self._dev
        return _dense_conditional(d["ctx"], d["spec"], d["X"], d["Lu"], d["ctx"].to_device(self.q_mu.value), self.mean_function, Xnew,
                                  full_cov)


def _dense_conditional(ctx, spec, X, L, W, mean_function, Xnew, full_cov):
    """The prediction both dense layers share (layers.py:289-293, 320-335), from a factor L of the kernel matrix at X and W (N, D_out):
    A = L^-1 K(X, X*), mean = A^T W + m(X*), variance = Kdiag - colsum(A^2) (X*, D_out), or with full_cov K(X*, X*) - A^T A tiled to
    (N*, N*, D_out) -> numpy arrays"""
    Xs = ctx.as_device(Xnew)
    N, ns, DO = X.shape[0], Xs.shape[0], W.shape[1]
    A, mean = ctx.empty(N, ns), ctx.empty(ns, DO)
    ctx.gram(spec, X, Xs, 0.0, A)                # K(X, X*)
    ctx.trsm(L, A)
    ctx.gemm(1, 0, 1.0, A, W, 0.0, mean)
    m = _mean_on_device(ctx, mean_function, Xs, DO)
    if m is not None:
        mean = mean + m
    if full_cov:
        K = ctx.empty(ns, ns)
        ctx.gram(spec, Xs, None, 0.0, K)
        ctx.gemm(1, 0, -1.0, A, A, 1.0, K)
        ctx.sync()
        return mean.cpu().numpy(), np.tile(K.cpu().numpy()[:, :, None], [1, 1, DO])       # layers.py:330-331: a copy per output
    var = ctx.empty(ns, DO)
    ctx.gpr_var(A, float(spec.variance) + (float(spec.white_variance) if spec.has_white else 0.0), var)
    ctx.sync()
    return mean.cpu().numpy(), var.cpu().numpy()


class SGPMC_Layer(Layer):
    """A sparse layer for sampling (layers.py:249-260): an SVGP layer without q_sqrt, whose inducing outputs `q_mu` (M, num_outputs)
    carry a standard-normal prior (white=True: of the whitened values) and are sampled or optimised rather than given a Gaussian
    posterior.  Its conditional is the reference's conditional_ND on the branch `q_sqrt is None` (layers.py:178-219, line 200):
    A = Lu^-1 K(Z, X), mean = A^T W + m(X) with W = q_mu (white) or Lu^-1 q_mu, variance = Kdiag - colsum(A^2) for every output
    (dsdgp_sparse_conditional), and `conditional_vjp` is its reverse pass (dsdgp_sparse_conditional_grad).  Unlike GPMC_Layer nothing is
    frozen at construction: Z and the kernel are read at every evaluation and have gradients.  Constructing the layer touches no
    device.  It lives under a collapsed layer in a DGP_Collapsed, or at every depth of a model_zoo.DGP_SGPMC; the engine does not take it
    (its KL tail reads a q_sqrt)."""
    _no_owner = "an SGPMC_Layer outside a DGP_Collapsed owns no random numbers: pass z to sample_from_conditional"

    def __init__(self, kern, Z, num_outputs, mean_function, white=False, input_prop_dim=None, **kwargs):
        Layer.__init__(self, input_prop_dim, **kwargs)
        split_kernel(kern)
        Z = np.array(Z, dtype=np.float64)
        self.num_inducing = Z.shape[0]
        self.feature = InducingPoints(Z)
        self.q_mu = Parameter(np.zeros((self.num_inducing, int(num_outputs))))
        self.q_sqrt = None
        self.kern = kern
        self.mean_function = mean_function
        self.num_outputs = int(num_outputs)
        self.white = bool(white)

    log_prior = _log_prior

    def _check_mean(self, what):
        _refuse_trainable_mean(self.mean_function, f"SGPMC_Layer.{what}")

    def _operands(self, X):
        ctx = Context.get()
        spec, ls = _kernel_spec(self.kern)
        Xd = ctx.as_device(X)
        if Xd.dim() != 2 or Xd.shape[1] != spec.input_dim or self.feature.Z.shape[1] != spec.input_dim:
            raise ValueError("SGPMC_Layer: X must be (N, D) and Z (M, D), D the kernel's input_dim")
        object.__setattr__(self, "_last_X", Xd)
        return ctx, spec, ls, ctx.to_device(self.feature.Z.value), Xd, ctx.to_device(self.q_mu.value)

    def conditional_device(self, X):
        """(mean (N, num_outputs), var (N,)) as device tensors, without waiting for them: the variance is ONE column, the same for every
        output.  X: a numpy array or a device tensor."""
        self._check_mean("conditional")
        ctx, spec, ls, Z, Xd, q = self._operands(X)
        mean, var = ctx.empty(Xd.shape[0], self.num_outputs), ctx.empty(Xd.shape[0])
        ctx.sparse_conditional(spec, Z, Xd, q, self.white, settings.jitter, mean, var)
        m = _mean_on_device(ctx, self.mean_function, Xd, self.num_outputs)
        return (mean if m is None else mean + m), var

    # layers.py:178-219 with q_sqrt = None
    def conditional_ND(self, X, full_cov=False):
        """full_cov: K(X, X) - A^T A as (N, N, num_outputs), a copy per output, composed from dsdgp_gram / dsdgp_trsm / dsdgp_gemm as
        the dense layers' prediction is"""
        if not full_cov:
            mean, var = self.conditional_device(X)
            Context.get().sync()
            return mean.cpu().numpy(), np.tile(var.cpu().numpy()[:, None], [1, self.num_outputs])
        self._check_mean("conditional")
        ctx, spec, ls, Z, Xd, q = self._operands(X)
        Lu = ctx.empty(self.num_inducing, self.num_inducing)
        ctx.gram(spec, Z, None, settings.jitter, Lu)
        ctx.potrf(Lu)
        if not self.white:
            ctx.trsm(Lu, q)
        return _dense_conditional(ctx, spec, Z, Lu, q, self.mean_function, Xd, True)

    def conditional_vjp(self, dmean, dvar, X=None, on_device=False):
        """The reverse pass of conditional_ND(X) for a scalar F: dmean (N, num_outputs) and dvar (N, num_outputs; or (N,), already
        summed over the outputs) are the adjoints of its mean and variance; X=None: the inputs of the last conditional_ND /
        conditional_device call.  Returns the gradients of F as a dict: `q_mu` (M,
        num_outputs), `Z` (M, D), `X` (N, D), `variance`, `lengthscales` (the kernel's) and, with a White part, `white_variance`.
        A fixed mean function adds its own Jacobian to `X`: dmean for Identity, dmean A^T for Linear.  numpy arrays or device tensors
        in; on_device: device tensors (the numbers of shape (1,)) out, without waiting for them."""
        self._check_mean("conditional_vjp")
        if X is None:
            X = getattr(self, "_last_X", None)
            if X is None:
                raise RuntimeError("SGPMC_Layer.conditional_vjp: no X given and no conditional evaluated yet")
        ctx, spec, ls, Z, Xd, q = self._operands(X)
        gm, gv = ctx.as_device(dmean), ctx.as_device(dvar)
        n, D, M, DO = Xd.shape[0], int(spec.input_dim), self.num_inducing, self.num_outputs
        if gv.dim() == 2:
            gv = gv.sum(1) if gv.shape[1] > 1 else gv[:, 0]
        gv = gv.contiguous()
        if tuple(gm.shape) != (n, DO) or tuple(gv.shape) != (n,):
            raise ValueError(f"conditional_vjp: dmean must be {(n, DO)} and dvar {(n, DO)} or {(n,)}")
        d_q, d_Z, d_X, d_k = ctx.empty(M, DO), ctx.empty(M, D), ctx.empty(n, D), ctx.empty(kernel_grad_size(spec, True))
        ctx.sparse_conditional_grad(spec, Z, Xd, q, self.white, settings.jitter, gm, gv, d_q, d_Z, d_X, d_k)
        mf = self.mean_function
        if mf.kind == "identity":
            d_X = d_X + gm
        elif mf.kind == "linear":
            ctx.gemm(0, 1, 1.0, gm, ctx.to_device(mf.A.value), 1.0, d_X)
        variance, lengthscales, diag = cut_kernel_grad(spec, d_k)
        res = dict(q_mu=d_q, Z=d_Z, X=d_X, variance=variance, lengthscales=lengthscales)
        scalars = ["variance"]
        if spec.has_white:
            res["white_variance"] = diag
            scalars.append("white_variance")
        return res if on_device else _to_host(ctx, res, tuple(scalars))


class Collapsed_Layer(Layer):
    """Extra functions for a collapsed layer (layers.py:296-307): a last layer whose Gaussian posterior is at its exact optimum for
    the data it has been given, so it carries no variational parameters and no KL term of its own."""
    white = False
    _no_owner = "a collapsed layer outside a DGP_Collapsed owns no random numbers: pass z to sample_from_conditional"

    def set_data(self, X_mean, X_var, Y, lik_variance):
        self._X_mean = X_mean
        self._X_var = X_var
        self._Y = Y
        self._lik_variance = lik_variance

    def build_likelihood(self):
        raise NotImplementedError


class SGPR_Layer(Collapsed_Layer):
    """A sparse variational GP layer with a Gaussian likelihood where the GP is integrated out (layers.py:345-367): the bound of
    gplvm_build_likelihood and the prediction of gplvm_build_predict, psi branch (layers.py:405-450, 483-525), with the input noise
    of the last hop integrated analytically through the expectations of the kernel (dsdgp_rbf_expectations).  set_data factorises
    once — L = chol(Kuu), LB = chol(L^-1 psi2 L^-T / s2 + I), c = LB^-1 L^-1 psi1^T Y / s2 stay on the device — and
    build_likelihood / conditional_ND read the factors.  X_var=None is zero variance.  Only a plain RBF kernel has the closed-form
    expectations, and only the Zero mean function is consistent: the reference's psi branch ignores the mean function in the bound
    and adds it in the prediction."""

    def __init__(self, kern, Z, num_outputs, mean_function, **kwargs):
        Collapsed_Layer.__init__(self, **kwargs)
        _rbf_spec(kern, "SGPR_Layer")
        if getattr(mean_function, "kind", None) != "zero":
            raise NotImplementedError(f"SGPR_Layer: mean function {type(mean_function).__name__}: the reference's bound ignores the "
                                      "mean function and its prediction adds it, so only Zero is consistent")
        self.feature = Z if isinstance(Z, InducingPoints) else InducingPoints(np.array(Z, dtype=np.float64))
        self.num_inducing = self.feature.Z.shape[0]
        self.kern = kern
        self.mean_function = mean_function
        self.num_outputs = int(num_outputs)
        object.__setattr__(self, "_factors", None)

    def set_data(self, X_mean, X_var, Y, lik_variance):
        """X_mean, X_var (N, D_in) — numpy or device tensors, X_var may be None — Y (N, D_Y) and the noise variance.  Runs the
        expectations and both factorisations; CholeskyError if Kuu or AAT + I is not positive definite (the layer then holds no data)."""
        object.__setattr__(self, "_factors", None)
        ctx = Context.get()
        mu, Yd = ctx.as_device(X_mean), ctx.as_device(Y)
        s = None if X_var is None else ctx.as_device(X_var)
        N, D = mu.shape
        M, DY = self.num_inducing, Yd.shape[1]
        if Yd.shape[0] != N or (s is not None and tuple(s.shape) != (N, D)) or D != self.feature.Z.shape[1]:
            raise ValueError("set_data: X_mean and X_var must be (N, D_in) and Y (N, D_Y)")
        s2 = float(lik_variance)
        spec, ls = _rbf_spec(self.kern, "SGPR_Layer")
        Z = ctx.to_device(self.feature.Z.value)
        psi0, psi1, psi2 = kernel_expectations(self.kern, Z, mu, s, on_device=True)
        L, G, B, T = ctx.empty(M, M), ctx.empty(M, M), ctx.empty(M, M), psi2
        psi2_kept = ctx.empty(M, M)                  # the first solve overwrites psi2; bound_gradients reads it
        ctx.scale_copy(psi2, psi2_kept)
        ctx.gram(spec, Z, None, settings.jitter, L)
        ctx.potrf(L)                                 # L = chol(Kuu)
        ctx.trsm(L, T)                               # tmp = L^-1 psi2
        ctx.scale_copy(T, G, trans=1)                # tmp^T
        ctx.trsm(L, G)                               # G = L^-1 psi2 L^-T = s2 AAT
        ctx.scale_copy(G, B, div=s2, diag_add=1.0)   # B = AAT + I
        ctx.potrf(B)                                 # LB = chol(B)
        c = ctx.empty(M, DY)
        ctx.gemm(1, 0, 1.0 / s2, psi1, Yd, 0.0, c)   # psi1^T Y / s2
        ctx.trsm(L, c)
        ctx.trsm(B, c)                               # c = LB^-1 L^-1 psi1^T Y / s2
        Collapsed_Layer.set_data(self, mu, s, Yd, s2)
        object.__setattr__(self, "_factors", dict(ctx=ctx, spec=spec, ls=ls, Z=Z, L=L, LB=B, G=G, c=c, psi0=psi0, N=N, DY=DY, s2=s2,
                                                  kdiag=float(spec.variance), psi1=psi1, psi2=psi2_kept))

    def _need_factors(self):
        if self._factors is None:
            raise RuntimeError("SGPR_Layer: call set_data(X_mean, X_var, Y, lik_variance) first")
        return self._factors

    def bound_terms(self):
        """(bound, its six terms) of layers.py:443-448 as the device assembled them."""
        f = self._need_factors()
        ctx = f["ctx"]
        out = ctx.empty(7)
        ctx.collapsed_bound(f["LB"], f["G"], f["c"], self._Y, f["psi0"], f["s2"], out)
        ctx.sync()
        o = out.cpu().numpy()
        return float(o[0]), o[1:].copy()

    def build_likelihood(self):
        return self.bound_terms()[0]

    def bound_gradients(self, on_device=False):
        """The bound of build_likelihood and its gradients with respect to the CONSTRAINED values of everything it depends on, as a
        dict: `bound`, `Z` (M, D), `variance`, `lengthscales` (the kernel's), `lik_variance` (the noise variance given to set_data),
        `X_mean`, `X_var` (N, D; `X_var` is present — the derivative at zero variance — even when the layer was given None).
        numpy arrays and numbers, or device tensors (the scalars of shape (1,)) without waiting for them with on_device=True.
        Read as F(Kuu, psi0, psi1, psi2, s2) with Sigma = Kuu + psi2 / s2 = L B L^T and alpha = Sigma^-1 psi1^T Y / s2 = L^-T LB^-T c,
        the bound has the adjoints (dsdgp_collapsed_adjoints; the inverses from the factors of set_data by dsdgp_trsm / dsdgp_gemm)
            dF/dSigma = -1/2 D_Y Sigma^-1 - 1/2 alpha alpha^T,   g_psi0 = -1/2 D_Y / s2,   g_psi1 = Y alpha^T / s2,
            g_psi2 = dF/dSigma / s2 + 1/2 D_Y Kuu^-1 / s2,   d_Kuu = dF/dSigma + 1/2 D_Y Kuu^-1 - 1/2 D_Y Kuu^-1 psi2 Kuu^-1 / s2,
        and they reach the inputs, Z and the kernel through the reverse pass of the expectations (dsdgp_rbf_expectations_grad): once
        with (g_psi0, g_psi1, g_psi2), and once more for Kuu = K(Z, Z) + jitter I, which is psi1 at X_mean = Z with zero variance —
        g_psi1 = d_Kuu, and both of its input adjoints belong to Z (the jitter is a constant).  The same data give the same bits."""
        f = self._need_factors()
        ctx, M, DY, N, s2 = f["ctx"], self.num_inducing, f["DY"], f["N"], f["s2"]
        Z, L, LB, c, psi0, psi2, Y = f["Z"], f["L"], f["LB"], f["c"], f["psi0"], f["psi2"], self._Y
        zeros = ctx.torch.zeros(M, M, dtype=ctx.torch.float64, device=Z.device)
        Li, W, Si, Ki, tmp, KpK = (ctx.empty(M, M) for _ in range(6))
        ctx.scale_copy(zeros, Li, diag_add=1.0)      # I
        ctx.trsm(L, Li)                              # L^-1
        ctx.scale_copy(Li, W)
        ctx.trsm(LB, W)                              # LB^-1 L^-1
        ctx.gemm(1, 0, 1.0, W, W, 0.0, Si)           # Sigma^-1
        ctx.gemm(1, 0, 1.0, Li, Li, 0.0, Ki)         # Kuu^-1
        ctx.gemm(0, 0, 1.0, Ki, psi2, 0.0, tmp)
        ctx.gemm(0, 0, 1.0, tmp, Ki, 0.0, KpK)       # Kuu^-1 psi2 Kuu^-1
        alpha = ctx.empty(M, DY)
        ctx.scale_copy(c, alpha)
        ctx.trsm(LB, alpha, trans=1)
        ctx.trsm(L, alpha, trans=1)                  # alpha = L^-T LB^-T c
        g1, g2, dK, out, bound = ctx.empty(N, M), ctx.empty(M, M), ctx.empty(M, M), ctx.empty(8), ctx.empty(7)
        ctx.gemm(0, 1, 1.0 / s2, Y, alpha, 0.0, g1)  # Y alpha^T / s2
        ctx.collapsed_adjoints(Si, Ki, KpK, psi2, alpha, c, Y, psi0, s2, g2, dK, out)
        ctx.collapsed_bound(LB, f["G"], c, Y, psi0, s2, bound)
        spec = f["spec"]
        D, nk = int(spec.input_dim), kernel_grad_size(spec, False)
        d_mu, d_s, d_Z, d_k = ctx.empty(N, D), ctx.empty(N, D), ctx.empty(M, D), ctx.empty(nk)
        k_mu, k_Z, k_k = ctx.empty(M, D), ctx.empty(M, D), ctx.empty(nk)
        grad = lambda *args: _lib.check(ctx.lib.dsdgp_rbf_expectations_grad(ctx.handle, C.byref(spec), ptr(Z), M, *args))
        grad(ptr(self._X_mean), ptr(self._X_var), N, -0.5 * DY / s2, ptr(g1), M, ptr(g2), M, ptr(d_mu), ptr(d_s), ptr(d_Z), ptr(d_k))
        grad(ptr(Z), None, M, 0.0, ptr(dK), M, None, 0, ptr(k_mu), None, ptr(k_Z), ptr(k_k))
        d_Z = d_Z + (k_Z + k_mu)                     # element-wise sums of the two calls' results, on the context's stream
        variance, lengthscales, _ = cut_kernel_grad(spec, d_k + k_k)
        res = dict(bound=bound[:1], Z=d_Z, variance=variance, lengthscales=lengthscales, lik_variance=out[:1], X_mean=d_mu, X_var=d_s)
        return res if on_device else _to_host(ctx, res, ("bound", "variance", "lik_variance"))

    # layers.py:483-525
    def conditional_ND(self, Xnew, full_cov=False):
        f = self._need_factors()
        ctx, M, DY = f["ctx"], self.num_inducing, f["DY"]
        Xs = ctx.as_device(Xnew)
        ns = Xs.shape[0]
        tmp1, tmp2, mean = ctx.empty(M, ns), ctx.empty(M, ns), ctx.empty(ns, DY)
        ctx.gram(f["spec"], f["Z"], Xs, 0.0, tmp1)   # K(Z, X*)
        ctx.trsm(f["L"], tmp1)
        ctx.scale_copy(tmp1, tmp2)
        ctx.trsm(f["LB"], tmp2)
        ctx.gemm(1, 0, 1.0, tmp2, f["c"], 0.0, mean)
        if full_cov:
            K = ctx.empty(ns, ns)
            ctx.gram(f["spec"], Xs, None, 0.0, K)
            ctx.gemm(1, 0, 1.0, tmp2, tmp2, 1.0, K)
            ctx.gemm(1, 0, -1.0, tmp1, tmp1, 1.0, K)
            ctx.sync()
            return mean.cpu().numpy(), np.tile(K.cpu().numpy()[:, :, None], [1, 1, DY])       # layers.py:518-519: a copy per output
        var = ctx.empty(ns, DY)
        ctx.collapsed_var(tmp1, tmp2, f["kdiag"], var)
        ctx.sync()
        return mean.cpu().numpy(), var.cpu().numpy()


class GPR_Layer(Collapsed_Layer):
    """A dense GP layer with a Gaussian likelihood where the GP is integrated out (layers.py:310-342): exact GP regression on the
    inputs it is given, no inducing points.  set_data factorises once — L = chol(k(F, F) + s2 I) (dsdgp_gram with the noise variance as
    its diagonal add, dsdgp_potrf) and V = L^-1 (Y - m(F)) stay on the device — and build_likelihood / conditional_ND /
    bound_gradients read the factors.  X_var is ignored, as in the reference.  Kernels: RBF or Matern52, with or without a White
    part; mean functions: Zero, Identity, Linear."""

    def __init__(self, kern, mean_function, num_outputs, **kwargs):
        Collapsed_Layer.__init__(self, **kwargs)
        split_kernel(kern)
        self.kern = kern
        self.mean_function = mean_function
        self.num_outputs = int(num_outputs)
        object.__setattr__(self, "_factors", None)

    def set_data(self, X_mean, X_var, Y, lik_variance):
        """X_mean (N, D_in), Y (N, D_Y) — numpy or device tensors — and the noise variance; X_var is ignored.  Runs the Gram matrix,
        its factorisation and one solve; CholeskyError if k(F, F) + s2 I is not positive definite (the layer then holds no data)."""
        object.__setattr__(self, "_factors", None)
        ctx = Context.get()
        F, Yd = ctx.as_device(X_mean), ctx.as_device(Y)
        spec, ls = _kernel_spec(self.kern)
        if F.dim() != 2 or Yd.dim() != 2 or Yd.shape[0] != F.shape[0] or F.shape[1] != spec.input_dim:
            raise ValueError("set_data: X_mean must be (N, D_in), D_in the kernel's input_dim, and Y (N, D_Y)")
        N, DY = Yd.shape
        s2 = float(lik_variance)
        L = ctx.empty(N, N)
        ctx.gram(spec, F, None, s2, L)
        ctx.potrf(L)                                 # L = chol(K + s2 I)
        m = _mean_on_device(ctx, self.mean_function, F, DY)
        V = (Yd.clone() if m is None else Yd - m).contiguous()
        ctx.trsm(L, V)                               # V = L^-1 (Y - m(F))
        Collapsed_Layer.set_data(self, F, None, Yd, s2)
        object.__setattr__(self, "_factors", dict(ctx=ctx, spec=spec, ls=ls, L=L, V=V, N=N, DY=DY, s2=s2))

    def _need_factors(self):
        if self._factors is None:
            raise RuntimeError("GPR_Layer: call set_data(X_mean, X_var, Y, lik_variance) first")
        return self._factors

    def bound_terms(self):
        """(bound, its three terms -1/2 N D_Y log 2 pi, -D_Y sum log L_ii, -1/2 sum V^2) as the device assembled them (dsdgp_gpr_bound)"""
        f = self._need_factors()
        ctx = f["ctx"]
        out = ctx.empty(4)
        ctx.gpr_bound(f["L"], f["V"], out)
        ctx.sync()
        o = out.cpu().numpy()
        return float(o[0]), o[1:].copy()

    def build_likelihood(self):
        return self.bound_terms()[0]

    def bound_gradients(self, on_device=False):
        """The bound of build_likelihood and its gradients with respect to the CONSTRAINED values of everything it depends on, as a
        dict: `bound`, `variance`, `lengthscales` (the kernel's), `white_variance` (if the kernel has a White part), `lik_variance`
        (the noise variance given to set_data), `X_mean`, `X_var` (N, D_in; `X_var` is all zeros: the layer ignores it).  numpy arrays
        and numbers, or device tensors (the scalars of shape (1,)) without waiting for them with on_device=True.
        With alpha = L^-T V = K^-1 (Y - m) the bound has dF/dK = 1/2 (alpha alpha^T - D_Y K^-1): K^-1 from the factor (dsdgp_trsm of
        the identity, one dsdgp_gemm), then one dsdgp_gemm with beta = -1/2 D_Y into it, and one symmetric dsdgp_gram_grad takes it to
        the inputs and the kernel; its diagonal entry is at once the gradient in the noise variance and in the White variance.  The
        mean function adds dF/dm = alpha through its own Jacobian: alpha for Identity, alpha A^T (one dsdgp_gemm) for Linear.  A Linear
        mean with trainable A or b raises NotImplementedError: their gradients are not formed."""
        f = self._need_factors()
        mf = self.mean_function
        _refuse_trainable_mean(mf, "GPR_Layer.bound_gradients")
        ctx, N, DY, L, V, spec = f["ctx"], f["N"], f["DY"], f["L"], f["V"], f["spec"]
        F = self._X_mean
        D = int(spec.input_dim)
        alpha = V.clone()
        ctx.trsm(L, alpha, trans=1)                  # alpha = L^-T V
        zeros = ctx.torch.zeros(N, N, dtype=ctx.torch.float64, device=F.device)
        Li, dK = ctx.empty(N, N), ctx.empty(N, N)
        ctx.scale_copy(zeros, Li, diag_add=1.0)      # I
        ctx.trsm(L, Li)                              # L^-1
        ctx.gemm(1, 0, 1.0, Li, Li, 0.0, dK)         # K^-1
        ctx.gemm(0, 1, 0.5, alpha, alpha, -0.5 * DY, dK)      # dF/dK = 1/2 (alpha alpha^T - D_Y K^-1)
        d_X, d_k, bound = ctx.empty(N, D), ctx.empty(kernel_grad_size(spec, True)), ctx.empty(4)
        ctx.gram_grad(spec, F, None, dK, d_X, None, d_k)
        if mf.kind == "identity":
            d_X = d_X + alpha
        elif mf.kind == "linear":
            ctx.gemm(0, 1, 1.0, alpha, ctx.to_device(mf.A.value), 1.0, d_X)
        ctx.gpr_bound(L, V, bound)
        variance, lengthscales, diag = cut_kernel_grad(spec, d_k)
        res = dict(bound=bound[:1], variance=variance, lengthscales=lengthscales, lik_variance=diag, X_mean=d_X,
                   X_var=ctx.torch.zeros_like(d_X))
        scalars = ["bound", "variance", "lik_variance"]
        if spec.has_white:
            res["white_variance"] = diag
            scalars.append("white_variance")
        return res if on_device else _to_host(ctx, res, tuple(scalars))

    # layers.py:320-335
    def conditional_ND(self, Xnew, full_cov=False):
        f = self._need_factors()
        return _dense_conditional(f["ctx"], f["spec"], self._X_mean, f["L"], f["V"], self.mean_function, Xnew, full_cov)
