"""Host mirror of the reference's model_zoo.py:25-88: `DGP_Collapsed`, a DGP whose last layer is a collapsed one (layers.SGPR_Layer, or
the dense layers.GPR_Layer: exact GP regression on top, no inducing inputs, gradients through the reverse pass of the Gram matrix), and
`DGP_Heinonen` (at the end of this file), the dense two-layer model sampled by training.HMC.  What follows describes `DGP_Collapsed`.
Its bound is the one of the reference's `_build_likelihood`: the last layer at its exact optimum over the WHOLE training set, the input
noise of the last hop integrated analytically through the kernel expectations, minus the KL terms of the inner layers.  The inner
layers run as one device Engine over `layers[:-1]` (`inner_engine()`; S = 1 on the full training set, explicit `zs` accepted); the
last layer is the host layer loop that `DGP_Base.propagate(full_cov=True)` uses.  What the collapsed layer itself owns — its
inducing inputs, its kernel, the noise variance — has gradients (`compute_log_likelihood_gradients`, the reverse pass of the kernel
expectations); with `inner=True` the adjoints of the last layer's input mean and variance go on through the inner layers' engine
(`Engine.forward_saved` / `backward_adjoints`, the library's dsdgp_model_forward_saved / dsdgp_model_backward_adjoints), so every
trainable parameter of every layer has its gradient of the collapsed bound, as TensorFlow gives the reference.  Training is
`training.ScipyOptimizer` (L-BFGS-B; `inner=True` for all layers) or `training.CollapsedAdamOptimizer` (full-batch Adam).  The
minibatch machinery of a sampled bound — `train_step`, `AdamOptimizer`, `NatGradOptimizer`, `_build_likelihood(with_grad=True)` —
still raises NotImplementedError: `supports_gradients` stays False, the bound being that of the whole training set.  A `DGP` trained
on the sampled bound can also be read as a collapsed model through `DGP_Collapsed.from_dgp(model)`.  There is no engine over ALL
layers (the collapsed layer has no variational parameters to put into one), so `engine()` and the device-side scoring methods built
on it (`evaluate`, `predict_quantiles`, `calibration`, `classification_report`) raise NotImplementedError as well: score a collapsed
model from `predict_y` / `predict_density`."""
import ctypes as C
import weakref

import numpy as np

from . import _lib
from .dgp import DGP_Base
from .gpflow_compat import Gaussian
from .layers import Collapsed_Layer, GPMC_Layer, GPR_Layer, SGPMC_Layer, SGPR_Layer, _to_host, concat_input_prop


class DGP_Collapsed(DGP_Base):
    supports_gradients = False

    def __init__(self, X, Y, likelihood, layers, **kwargs):
        if kwargs.get("minibatch_size") is not None:
            raise ValueError("DGP_Collapsed: minibatch_size must be None — the last layer is optimal for the whole training set "
                             "(model_zoo.py:54)")
        if not isinstance(likelihood, Gaussian):
            raise NotImplementedError(f"DGP_Collapsed: the last layer is collapsed against a Gaussian likelihood, not "
                                      f"{type(likelihood).__name__}")
        layers = list(layers)
        if not layers or not isinstance(layers[-1], Collapsed_Layer):
            raise ValueError("DGP_Collapsed: the last layer must be a Collapsed_Layer (SGPR_Layer, GPR_Layer)")
        if any(isinstance(layer, Collapsed_Layer) for layer in layers[:-1]):
            raise ValueError("DGP_Collapsed: only the last layer is collapsed")
        sgpmc = any(isinstance(layer, SGPMC_Layer) for layer in layers[:-1])
        if sgpmc and len(layers) != 2:
            raise NotImplementedError("DGP_Collapsed: an SGPMC_Layer is the ONE inner layer of a two-layer model, [SGPMC_Layer, SGPR_Layer] "
                                      f"or [SGPMC_Layer, GPR_Layer], not one of {len(layers) - 1} inner layers: the collapsed layer takes "
                                      "the marginal mean and variance of its inputs, which below a second inner layer need draws — "
                                      "that is the engine's work, and the engine takes no layer without q_sqrt (an SVGP layer beside an "
                                      "SGPMC layer needs it as well)")
        DGP_Base.__init__(self, X, Y, likelihood, layers, **kwargs)
        object.__setattr__(self, "_sgpmc", sgpmc)
        if sgpmc:
            object.__setattr__(layers[0], "_model", weakref.ref(self))
        self.white = bool(layers[0].white) if len(layers) > 1 else False
        object.__setattr__(layers[-1], "_model", weakref.ref(self))          # the last layer draws its samples through this model's seeds

    @classmethod
    def from_dgp(cls, model):
        """The collapsed view of a trained DGP: the inner layers, the last layer's kernel and inducing inputs and the likelihood are
        SHARED with `model` (not copied), its last SVGP_Layer is replaced by an SGPR_Layer."""
        last = model.layers[-1]
        top = SGPR_Layer(last.kern, last.feature, last.num_outputs, last.mean_function)
        return cls(model.X_data, model.Y_data, model.likelihood.likelihood, list(model.layers[:-1]) + [top])

    # ------------------------------------------------------------------ what has no meaning without an engine over all layers
    def _no_full_engine(self, what):
        raise NotImplementedError(f"DGP_Collapsed.{what}: there is no device engine over all layers (the collapsed last layer is not "
                                  "part of one); use predict_f / predict_y / predict_density")

    def engine(self):
        self._no_full_engine("engine")

    def evaluate(self, *args, **kwargs):
        self._no_full_engine("evaluate")

    def predict_quantiles(self, *args, **kwargs):
        self._no_full_engine("predict_quantiles")

    def calibration(self, *args, **kwargs):
        self._no_full_engine("calibration")

    def classification_report(self, *args, **kwargs):
        self._no_full_engine("classification_report")

    def next_minibatch(self):
        self._no_full_engine("next_minibatch")

    # ------------------------------------------------------------------ engine over the inner layers
    def inner_engine(self):
        if len(self.layers) == 1:
            raise RuntimeError("a one-layer DGP_Collapsed has no inner layers and no engine")
        if self._sgpmc:
            raise RuntimeError("a DGP_Collapsed over an SGPMC_Layer has no engine: the layer's conditional is a call of its own")
        if self._eng is None:
            from .engine import Engine
            inner = self.layers[:-1]
            for layer in inner:                       # a shared layer's own engine may hold newer values than the host copy
                for p in layer.parameters():
                    p.value
            eng = Engine(inner, self.likelihood.likelihood, self.white, n_max=self.X_data.shape[0], s_max=1)
            for i, layer in enumerate(inner):
                if getattr(layer, "_model_engine", None) is None:
                    object.__setattr__(layer, "_model_engine", (eng, i))
            object.__setattr__(self, "_eng", eng)
        return self._eng

    def _context(self):
        from .engine import Context
        return Context.get()

    def _device_data(self):
        if self._dev_data is None:
            ctx = self._context()
            object.__setattr__(self, "_dev_data", (ctx.to_device(self.X_data), ctx.to_device(self.Y_data)))
        return self._dev_data

    def randn(self, shape, seed=None):
        """N(0, 1) draws for the last layer's samples (Layer.sample_from_conditional without z) under this model's seed sequence:
        stream len(layers) - 1 of `_draw_seed()`, as the engine numbers the streams of the layers it draws for."""
        ctx = self._context()
        n = int(np.prod(shape))
        out = ctx.empty(n)
        _lib.check(ctx.lib.dsdgp_randn(ctx.handle, C.c_uint64(self._draw_seed() if seed is None else seed),
                                       C.c_uint64(len(self.layers) - 1), n, C.c_void_p(out.data_ptr())))
        ctx.sync()
        return out.cpu().numpy().reshape(shape)

    def _refresh(self):
        """Parameters that another engine (the DGP the inner layers are shared with) has trained since the last evaluation: reading
        `.value` pulls them to the host; if the inner engine's parameter vector then differs from the one it last saw, it uploads.
        (Whether the other engine still counts itself as newer than the host says nothing: any earlier read has settled that.)"""
        if len(self.layers) == 1 or self._sgpmc:
            return
        eng = self.inner_engine()
        for p, *_ in eng.entries:
            p.value
        theta = eng._pack_host()
        seen = getattr(self, "_theta_seen", None)
        if seen is None or not np.array_equal(theta, seen):
            eng.mark_host_dirty()
            object.__setattr__(self, "_theta_seen", theta)

    # ------------------------------------------------------------------ model_zoo.py:26-44
    def inner_layers_propagate(self, X, full_cov=False, S=1, zs=None):
        X = np.asarray(X.cpu().numpy() if hasattr(X, "data_ptr") else X, dtype=np.float64)
        sX = np.tile(X[None], [int(S), 1, 1])
        if len(self.layers) == 1:                                   # model_zoo.py:30-31
            return [sX], [sX], [np.zeros_like(sX)]
        inner = self.layers[:-1]
        zs = list(zs)[:len(inner)] if zs is not None else None
        self._refresh()
        if full_cov or self._sgpmc:                                 # the host layer loop; an SGPMC_Layer is in no engine
            F, Fs, Fmeans, Fvars = sX, [], [], []
            for layer, z in zip(inner, zs or [None] * len(inner)):
                F, Fmean, Fvar = layer.sample_from_conditional(F, z=z, full_cov=full_cov)
                Fs.append(F); Fmeans.append(Fmean); Fvars.append(Fvar)
            return Fs, Fmeans, Fvars
        eng = self.inner_engine()
        Fs, Fmeans, Fvars = eng.propagate(X, int(S), zs=zs, seed=self._draw_seed())
        eng.ctx.sync()
        Fs, Fmeans, Fvars = self._np(Fs), self._np(Fmeans), self._np(Fvars)
        Fin = sX
        for l, layer in enumerate(inner):                           # layers.py:105-117, as DGP_Base.propagate
            if layer.input_prop_dim:
                Fs[l], Fmeans[l], Fvars[l] = concat_input_prop(Fin, layer.input_prop_dim, Fs[l], Fmeans[l], Fvars[l])
            Fin = Fs[l]
        return Fs, Fmeans, Fvars

    def _set_data(self, zs=None, seed=None):
        """model_zoo.py:48-49, 54-55: the marginal mean and variance of the last layer's inputs at the training set (S = 1) become
        the collapsed layer's data.  One layer: the inputs themselves, zero variance.  The statistics go from the engine to the
        layer as device tensors (unless the last inner layer propagates inputs: that concatenation is a host copy).  seed: the Philox
        seed of the hidden layers' draws where zs gives none (None: the model's next)."""
        lik_var = float(self.likelihood.likelihood.variance.value)
        Xd, Yd = self._device_data()
        if len(self.layers) == 1:
            self.layers[-1].set_data(Xd, None, Yd, lik_var)
            return
        if self._sgpmc:                 # the layer's conditional at the training inputs: nothing is drawn, nothing leaves the device
            low = self.layers[0]
            mean, var = low.conditional_device(Xd)
            var = var[:, None].expand(-1, low.num_outputs)
            p = low.input_prop_dim
            if p:
                torch = self._context().torch
                mean, var = torch.cat([Xd[:, :p], mean], 1), torch.cat([torch.zeros_like(Xd[:, :p]), var], 1)
            self.layers[-1].set_data(mean.contiguous(), var.contiguous(), Yd, lik_var)
            return
        if self.layers[-2].input_prop_dim:
            _, ms, vs = self.inner_layers_propagate(self.X_data, full_cov=False, S=1, zs=zs)
            self.layers[-1].set_data(ms[-1][0], vs[-1][0], Yd, lik_var)
            return
        self._refresh()
        eng = self.inner_engine()
        zs = list(zs)[:len(self.layers) - 1] if zs is not None else None
        _, ms, vs = eng.propagate(Xd, 1, zs=zs, seed=self._draw_seed() if seed is None else seed, want=("mean", "var"))
        self.layers[-1].set_data(ms[-1][0], vs[-1][0], Yd, lik_var)

    # ------------------------------------------------------------------ model_zoo.py:46-50
    def propagate(self, X, full_cov=False, S=1, zs=None):
        """zs: explicit draws per layer for the propagation of X (they are shaped for X, not for the training set); the statistics
        of the training set (S = 1) use fresh draws — with one inner layer they do not depend on any."""
        self._set_data()
        if len(self.layers) == 1:
            Fs, Fmeans, Fvars = [], [], []
            F = np.tile(np.asarray(X, dtype=np.float64)[None], [int(S), 1, 1])
        else:
            Fs, Fmeans, Fvars = self.inner_layers_propagate(X, full_cov=full_cov, S=S, zs=zs)
            F = Fs[-1]
        z = zs[len(self.layers) - 1] if zs is not None and len(zs) >= len(self.layers) else None
        F, Fmean, Fvar = self.layers[-1].sample_from_conditional(F, z=z, full_cov=full_cov)
        return Fs + [F], Fmeans + [Fmean], Fvars + [Fvar]

    def _build_predict(self, X, full_cov=False, S=1, zs=None):
        _, Fmeans, Fvars = self.propagate(X, full_cov=full_cov, S=S, zs=zs)
        return Fmeans[-1], Fvars[-1]

    # ------------------------------------------------------------------ model_zoo.py:52-57
    def _build_likelihood(self, X=None, Y=None, zs=None, with_grad=False, **kwargs):
        if X is not None or Y is not None:
            raise ValueError("DGP_Collapsed: the bound is that of the whole training set (model_zoo.py:54); no minibatch is taken")
        if with_grad:
            raise NotImplementedError("DGP_Collapsed._build_likelihood(with_grad=True) would leave a gradient in an engine over all layers, "
                                      "which a collapsed model does not have; the reverse pass of the collapsed bound through the inner "
                                      "layers is compute_log_likelihood_gradients(inner=True)")
        self._set_data(zs=zs)
        bound = self.layers[-1].build_likelihood()
        KL = sum(layer.KL() for layer in self.layers[:-1])
        return bound - KL

    def compute_log_likelihood_gradients(self, zs=None, inner=False):
        """(bound, [(Parameter, gradient), ...], {"X_mean": ..., "X_var": ...}): the bound of `compute_log_likelihood` and its
        gradients with respect to the constrained values of the parameters the collapsed last layer owns — its `feature.Z`,
        `kern.variance` and `kern.lengthscales` — and of the likelihood's `variance` (SGPR_Layer.bound_gradients; each gradient has its
        Parameter's shape).  These four are exact at any depth: the inner layers do not depend on them, and the KL terms do not either.
        The bound reaches the inner layers' OWN parameters only through the mean and the variance of the last layer's inputs, whose
        adjoints are the third result, `X_mean` and `X_var` (N, D_in).  zs: as for `compute_log_likelihood`.
        inner=True: those adjoints seed the reverse pass of the inner layers' engine (Engine.forward_saved / backward_adjoints, on the
        hidden layers' draws the bound was evaluated with: the same `zs`, or the same seed), and the list goes on,
        behind the four pairs, with every trainable parameter of the inner layers in the engine's order — per layer `feature.Z`,
        `q_mu`, `q_sqrt` (lower-triangular), the kernel's `variance` and `lengthscales`, a White part's `variance`, a trainable Linear
        mean's `A` and `b` — again the gradient of the bound, the KL terms included, with respect to the constrained value.  A one-layer
        model has no inner layers: the same four pairs.  NotImplementedError when the last inner layer propagates inputs
        (`input_prop_dim`): the adjoints of the propagated columns would have to re-enter the layer below.
        A GPR_Layer on top: the pairs are those of `top_parameters()` — the kernel's `variance` and `lengthscales`, a White part's
        `variance`, the likelihood's `variance`; there is no `feature.Z` — and `X_var` is all zeros (GPR_Layer.bound_gradients)."""
        inner = bool(inner) and len(self.layers) > 1
        top = self.layers[-1]
        if self._sgpmc:
            return self._sgpmc_gradients(inner)
        if inner:
            if self.layers[-2].input_prop_dim:
                raise NotImplementedError("DGP_Collapsed.compute_log_likelihood_gradients(inner=True): the last inner layer propagates "
                                          "inputs (input_prop_dim); the adjoints of the propagated columns of X_mean / X_var would have "
                                          "to re-enter the layer below, which the engine's reverse pass does not take")
        seed = self._draw_seed() if inner else None        # (one seed per evaluation either way)
        self._set_data(zs=zs, seed=seed)
        if inner:
            # The bound keeps the statistics of compute_log_likelihood (the engine's forward-only pass: same bits, same four pairs as
            # without `inner`); the pass that keeps what the reverse pass reads repeats the layers on the same draws.  Its statistics
            # differ from those by rounding only, and nothing below touches the engine before the reverse pass.
            eng = self.inner_engine()
            eng.forward_saved(self._device_data()[0], 1, zs=list(zs)[:len(self.layers) - 1] if zs is not None else None, seed=seed)
            g = top.bound_gradients(on_device=True)
            eng.backward_adjoints(g["X_mean"][None], g["X_var"][None], sync=False)
            g = _to_host(eng.ctx, g, ("bound", "variance", "lik_variance", "white_variance"))
        else:
            g = top.bound_gradients()
        KL = sum(layer.KL() for layer in self.layers[:-1])
        pairs = [(p, np.asarray(g[k], dtype=np.float64).reshape(p.shape)) for p, k in self.top_parameters()]
        if inner:
            pairs += self._inner_pairs(eng)
        return g["bound"] - KL, pairs, {"X_mean": g["X_mean"], "X_var": g["X_var"]}

    def _sgpmc_gradients(self, inner):
        """compute_log_likelihood_gradients over an SGPMC_Layer: the top layer's adjoints in X_mean and X_var (the propagated columns'
        dropped: they are copies of the fixed inputs) pushed through SGPMC_Layer.conditional_vjp, all on the device; with `inner` the
        pairs go on with the layer's `feature.Z`, `q_mu`, kernel `variance`, `lengthscales` and a White part's `variance`."""
        from .gpflow_compat import split_kernel
        top, low = self.layers[-1], self.layers[0]
        self._set_data()
        g = top.bound_gradients(on_device=True)
        scalars = ["bound", "variance", "lik_variance", "white_variance"]
        low_pairs = []
        if inner:
            p = low.input_prop_dim or 0
            v = low.conditional_vjp(g["X_mean"][:, p:].contiguous(), g["X_var"][:, p:].contiguous(), X=self._device_data()[0],
                                    on_device=True)
            stat, wk = split_kernel(low.kern)
            low_pairs = [(low.feature.Z, "Z"), (low.q_mu, "q_mu"), (stat.variance, "variance"), (stat.lengthscales, "lengthscales")] + \
                        ([(wk.variance, "white_variance")] if wk is not None else [])
            g.update({"low_" + k: v[k] for _, k in low_pairs})
            scalars += ["low_variance", "low_white_variance"]
        g = _to_host(self._context(), g, tuple(scalars))
        pairs = [(p, np.asarray(g[k], dtype=np.float64).reshape(p.shape)) for p, k in self.top_parameters()]
        pairs += [(p, np.asarray(g["low_" + k], dtype=np.float64).reshape(p.shape)) for p, k in low_pairs]
        return g["bound"], pairs, {"X_mean": g["X_mean"], "X_var": g["X_var"]}

    def _need_sgpmc(self, what):
        if not self._sgpmc:
            raise NotImplementedError(f"DGP_Collapsed.{what}: a log density needs a sampled inner layer with a prior — an SGPMC_Layer "
                                      "below the collapsed layer (or a DGP_Heinonen)")

    def compute_log_prior(self):
        """the standard-normal prior of the SGPMC_Layer's q_mu"""
        self._need_sgpmc("compute_log_prior")
        return self.layers[0].log_prior()

    def compute_log_density(self):
        """compute_log_likelihood() + compute_log_prior(): the target of training.HMC and, with inner=True, of training.ScipyOptimizer"""
        self._need_sgpmc("compute_log_density")
        return self.compute_log_likelihood() + self.compute_log_prior()

    def compute_log_density_gradients(self):
        """(log density, [(Parameter, gradient), ...]): compute_log_likelihood_gradients(inner=True) with the prior added — -q_mu to
        q_mu's pair"""
        self._need_sgpmc("compute_log_density_gradients")
        bound, pairs, _ = self.compute_log_likelihood_gradients(inner=True)
        low = self.layers[0]
        return bound + low.log_prior(), [(p, g - low.q_mu.value if p is low.q_mu else g) for p, g in pairs]

    def top_parameters(self):
        """[(Parameter, its key in the last layer's bound_gradients), ...]: what the collapsed last layer owns and the likelihood's
        variance.  SGPR_Layer: `feature.Z`, the kernel's `variance` and `lengthscales`, the noise variance.  GPR_Layer: no inducing
        inputs; the kernel's `variance` and `lengthscales`, a White part's `variance`, the noise variance."""
        from .gpflow_compat import split_kernel
        top = self.layers[-1]
        stat, wk = split_kernel(top.kern)
        lik = self.likelihood.likelihood
        if isinstance(top, GPR_Layer):
            return [(stat.variance, "variance"), (stat.lengthscales, "lengthscales")] + \
                   ([(wk.variance, "white_variance")] if wk is not None else []) + [(lik.variance, "lik_variance")]
        return [(top.feature.Z, "Z"), (stat.variance, "variance"), (stat.lengthscales, "lengthscales"), (lik.variance, "lik_variance")]

    def inner_parameters(self):
        """The Parameters of the inner layers in the order of the engine's layout (trainable or not) — per layer `feature.Z`, `q_mu`,
        `q_sqrt`, the kernel's `variance` and `lengthscales`, a White part's `variance`, and `A`, `b` of a Linear mean that is not a
        fixed map.  Host only: no engine is built."""
        from .gpflow_compat import split_kernel
        out = []
        for layer in self.layers[:-1]:
            stat, wk = split_kernel(layer.kern)
            out += [layer.feature.Z, layer.q_mu] + ([layer.q_sqrt] if layer.q_sqrt is not None else []) + [stat.variance, stat.lengthscales]
            if wk is not None:
                out.append(wk.variance)
            mf = layer.mean_function
            if mf.kind == "linear" and mf.in_theta():
                out += [mf.A, mf.b]
        return out

    def _inner_pairs(self, eng):
        """[(Parameter, gradient), ...] of the inner layers' trainable parameters from the engine's gradient buffer, which holds
        d(-bound)/d(unconstrained): sign flipped, a positive parameter's entry divided by d theta / dx (gpflow_compat.positive_slope)."""
        from .gpflow_compat import positive_slope
        eng.ctx.sync()
        out4 = eng.out4.cpu().numpy()
        if out4[3] != 0.0:
            raise _lib.CholeskyError(f"Cholesky decomposition was not successful (Kuu pivot {int(out4[3])})")
        grad = eng.grad.cpu().numpy()
        lik_p = self.likelihood.likelihood.variance
        pairs = []
        for p, off, cnt, kind in eng.entries:
            if p is lik_p or not p.trainable:
                continue
            gp = -grad[off:off + cnt].reshape(p.shape)
            if kind == "pos":
                gp = gp / positive_slope(p._value)
            elif kind == "qsqrt":
                gp = np.tril(gp)
            pairs.append((p, gp))
        return pairs

    def train_step(self, *args, **kwargs):
        raise NotImplementedError("DGP_Collapsed.train_step takes a minibatch step of the sampled bound; the collapsed bound is that of "
                                  "the whole training set, and its reverse pass through the inner layers is "
                                  "compute_log_likelihood_gradients(inner=True) — train with training.ScipyOptimizer(inner=True) or "
                                  "training.CollapsedAdamOptimizer")


class DGP_Heinonen(DGP_Collapsed):
    """A dense two-layer DGP with HMC for inference over the inner layer (model_zoo.py:60-88; Heinonen et al., Non-stationary Gaussian
    process regression with Hamiltonian Monte Carlo, AISTATS 2016): a GPMC_Layer whose whitened latents `q_mu` carry a standard-normal
    prior, under a GPR_Layer that is exact GP regression on those latents.  Two layers, a Gaussian likelihood, no minibatches.
    `compute_log_likelihood()` is log p(Y | q_mu), `compute_log_prior()` the prior of q_mu, `compute_log_density()` their sum — the
    target of `training.HMC` and what `training.ScipyOptimizer` maximises for this model (MAP).  Prediction is the host layer loop of
    DGP_Base.propagate over both layers, as in the reference."""

    def __init__(self, X, Y, likelihood, layers, **kwargs):
        layers = list(layers)
        if len(layers) != 2:                                            # model_zoo.py:77-80
            raise ValueError(f"DGP_Heinonen: two layers, not {len(layers)}")
        if not isinstance(likelihood, Gaussian):
            raise NotImplementedError(f"DGP_Heinonen: a Gaussian likelihood, not {type(likelihood).__name__}")
        if not isinstance(layers[0], GPMC_Layer) or not isinstance(layers[1], GPR_Layer):
            raise ValueError("DGP_Heinonen: layers must be [GPMC_Layer, GPR_Layer]")
        DGP_Collapsed.__init__(self, X, Y, likelihood, layers, **kwargs)
        if layers[0].num_data != self.X_data.shape[0]:
            raise ValueError("DGP_Heinonen: the GPMC_Layer must be built on the model's inputs X")
        object.__setattr__(layers[0], "_model", weakref.ref(self))

    def inner_engine(self):
        raise RuntimeError("DGP_Heinonen has no engine: its inner layer is a GPMC_Layer")

    def _refresh(self):
        pass

    # model_zoo.py:85-88
    def inner_layers_propagate(self, X, full_cov=False, S=1, zs=None):
        f = self.layers[0].build_latents()[None, :, :]
        return [f], [f], [np.zeros_like(f)]

    def _set_data(self, zs=None, seed=None):
        _, Yd = self._device_data()
        self.layers[-1].set_data(self.layers[0].build_latents(on_device=True), None, Yd, float(self.likelihood.likelihood.variance.value))

    def propagate(self, X, full_cov=False, S=1, zs=None):
        """model_zoo.py:46-50: the latents at the training inputs become the GPR_Layer's data, then DGP_Base.propagate's loop over the
        layers (dgp.py:61-76) on the host, each layer's arithmetic on the device."""
        self._set_data()
        F = np.tile(np.asarray(X, dtype=np.float64)[None], [int(S), 1, 1])
        Fs, Fmeans, Fvars = [], [], []
        for layer, z in zip(self.layers, zs or [None] * len(self.layers)):
            F, Fmean, Fvar = layer.sample_from_conditional(F, z=z, full_cov=full_cov)
            Fs.append(F); Fmeans.append(Fmean); Fvars.append(Fvar)
        return Fs, Fmeans, Fvars

    def compute_log_prior(self):
        return self.layers[0].log_prior()

    def compute_log_density(self):
        return self.compute_log_likelihood() + self.compute_log_prior()

    def compute_log_likelihood_gradients(self, zs=None, inner=False):
        """(bound, [(Parameter, gradient), ...], {"X_mean": ..., "X_var": ...}): log p(Y | q_mu) and its gradients with respect to the
        constrained values of `layers[0].q_mu` (the GPR_Layer's input adjoint taken through Lu: GPMC_Layer.latents_vjp), the top
        kernel's `variance` and `lengthscales` (and White `variance`) and the likelihood's `variance`; the third result is the adjoint of
        the latents.  The GPMC_Layer's own kernel has no gradient: its factor Lu is a constant (layers.py:278-279).  zs and inner are
        accepted for the signature of DGP_Collapsed and ignored: nothing is sampled, and q_mu is always among the pairs."""
        self._set_data()
        top, low = self.layers[-1], self.layers[0]
        g = top.bound_gradients(on_device=True)
        dq = low.latents_vjp(g["X_mean"], on_device=True)
        g = _to_host(self._context(), dict(g, q_mu=dq), ("bound", "variance", "lik_variance", "white_variance"))
        pairs = [(low.q_mu, g["q_mu"])] + [(p, np.asarray(g[k], dtype=np.float64).reshape(p.shape)) for p, k in self.top_parameters()]
        return g["bound"], pairs, {"X_mean": g["X_mean"], "X_var": g["X_var"]}

    def compute_log_density_gradients(self):
        """(log density, [(Parameter, gradient), ...]): compute_log_likelihood_gradients with the prior added — -q_mu to q_mu's pair"""
        bound, pairs, _ = self.compute_log_likelihood_gradients()
        low = self.layers[0]
        return bound + low.log_prior(), [(p, g - low.q_mu.value if p is low.q_mu else g) for p, g in pairs]
