"""Host mirror of the reference's model_zoo.py:25-88: `DGP_Collapsed`, a DGP whose last layer is a collapsed one (layers.SGPR_Layer, or
the dense layers.GPR_Layer: exact GP regression on top, no inducing inputs, gradients through the reverse pass of the Gram matrix), and
`DGP_Heinonen`, the dense two-layer model sampled by training.HMC, and (at the end of this file) `DGP_SGPMC`, the reference's DGP_Base
over SGPMC layers (dgp.py:42-98), sampled by training.SGHMC.  What follows describes `DGP_Collapsed`.
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
from .engine import ptr
from .gpflow_compat import Gaussian, likelihood_args, likelihood_entry, positive_slope, split_kernel
from .layers import (Collapsed_Layer, GPMC_Layer, GPR_Layer, SGPMC_Layer, SGPR_Layer, _to_host, layer_parameters, prepend_input_prop,
                     propagate_layers)


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

    def randn(self, shape, seed=None):
        """N(0, 1) draws for the last layer's samples (Layer.sample_from_conditional without z) under this model's seed sequence:
        stream len(layers) - 1 of `_draw_seed()`, as the engine numbers the streams of the layers it draws for."""
        return self._randn(shape, self._draw_seed() if seed is None else seed, len(self.layers) - 1)

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
            return propagate_layers(inner, sX, zs, full_cov=full_cov)
        eng = self.inner_engine()
        Fs, Fmeans, Fvars = eng.propagate(X, int(S), zs=zs, seed=self._draw_seed())
        eng.ctx.sync()
        Fs, Fmeans, Fvars = self._np(Fs), self._np(Fmeans), self._np(Fvars)
        prepend_input_prop(sX, inner, Fs, Fmeans, Fvars)            # layers.py:105-117, as DGP_Base.propagate
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
        top, low = self.layers[-1], self.layers[0]
        self._set_data()
        g = top.bound_gradients(on_device=True)
        scalars = ["bound", "variance", "lik_variance", "white_variance"]
        low_pairs = []
        if inner:
            p = low.input_prop_dim or 0
            v = low.conditional_vjp(g["X_mean"][:, p:].contiguous(), g["X_var"][:, p:].contiguous(), X=self._device_data()[0],
                                    on_device=True)
            low_pairs = layer_parameters(low, mean=False)
            g.update({"low_" + k: v[k] for _, k in low_pairs})
            scalars += ["low_variance", "low_white_variance"]
        g = _to_host(self._context(), g, tuple(scalars))
        pairs = [(p, np.asarray(g[k], dtype=np.float64).reshape(p.shape)) for p, k in self.top_parameters()]
        pairs += [(p, np.asarray(g["low_" + k], dtype=np.float64).reshape(p.shape)) for p, k in low_pairs]
        return g["bound"], pairs, {"X_mean": g["X_mean"], "X_var": g["X_var"]}

    def _prior_layer(self, what):
        """the layer whose q_mu carries the prior of a log density: the SGPMC_Layer (DGP_Heinonen: the GPMC_Layer) below the top"""
        if not hasattr(self.layers[0], "log_prior"):
            raise NotImplementedError(f"DGP_Collapsed.{what}: a log density needs a sampled inner layer with a prior — an SGPMC_Layer "
                                      "below the collapsed layer (or a DGP_Heinonen)")
        return self.layers[0]

    def compute_log_prior(self):
        """the standard-normal prior of the sampled layer's q_mu"""
        return self._prior_layer("compute_log_prior").log_prior()

    def compute_log_density(self):
        """compute_log_likelihood() + compute_log_prior(): the target of training.HMC and, with inner=True, of training.ScipyOptimizer"""
        self._prior_layer("compute_log_density")
        return self.compute_log_likelihood() + self.compute_log_prior()

    def compute_log_density_gradients(self):
        """(log density, [(Parameter, gradient), ...]): compute_log_likelihood_gradients(inner=True) with the prior added — -q_mu to
        q_mu's pair"""
        low = self._prior_layer("compute_log_density_gradients")
        bound, pairs, _ = self.compute_log_likelihood_gradients(inner=True)
        return bound + low.log_prior(), [(p, g - low.q_mu.value if p is low.q_mu else g) for p, g in pairs]

    def top_parameters(self):
        """[(Parameter, its key in the last layer's bound_gradients), ...]: what the collapsed last layer owns and the likelihood's
        variance.  SGPR_Layer: `feature.Z`, the kernel's `variance` and `lengthscales`, the noise variance.  GPR_Layer: no inducing
        inputs; the kernel's `variance` and `lengthscales`, a White part's `variance`, the noise variance."""
        return layer_parameters(self.layers[-1], mean=False) + [(self.likelihood.likelihood.variance, "lik_variance")]

    def inner_parameters(self):
        """The Parameters of the inner layers in the order of the engine's layout (trainable or not) — per layer `feature.Z`, `q_mu`,
        `q_sqrt`, the kernel's `variance` and `lengthscales`, a White part's `variance`, and `A`, `b` of a Linear mean that is not a
        fixed map.  Host only: no engine is built."""
        return [p for layer in self.layers[:-1] for p, _ in layer_parameters(layer)]

    def _inner_pairs(self, eng):
        """[(Parameter, gradient), ...] of the inner layers' trainable parameters from the engine's gradient buffer, which holds
        d(-bound)/d(unconstrained): sign flipped, a positive parameter's entry divided by d theta / dx (gpflow_compat.positive_slope)."""
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
        return propagate_layers(self.layers, np.tile(np.asarray(X, dtype=np.float64)[None], [int(S), 1, 1]), zs, full_cov=full_cov)

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


class DGP_SGPMC(DGP_Base):
    """The doubly-stochastic DGP with sampling in place of the Gaussian posterior: the reference's
    `DGP_Base(X, Y, likelihood, [SGPMC_Layer, ...], minibatch_size, num_samples)` (dgp.py:42-98 over layers.py:249-260) — layers without
    q_sqrt at every depth, a draw between them, the last layer not sampled — whose density is
    `num_data / N * sum E_q[log p(y | f)]` over a minibatch of N rows plus the standard-normal priors of every `q_mu`, the target of
    `training.SGHMC`.  Any likelihood of the project, MultiClass and Bernoulli included.  Every evaluation is ONE library call over the
    whole stack (dsdgp_stack_propagate, dsdgp_stack_logdensity: csrc/sgpmc_stack.hip) in a scratch block this model holds; the
    parameters are read from the host Parameters at every evaluation.  There is no engine (its KL tail reads a q_sqrt): `engine()`,
    `train_step`, `training.AdamOptimizer`, `NatGradOptimizer`, `ScipyOptimizer` and `HMC` refuse the model.
    `compute_log_likelihood(X, Y, zs)` is the data term, `compute_log_prior()` the priors, `compute_log_density(...)` their sum and
    `compute_log_density_gradients(...)` the sum with `[(Parameter, gradient), ...]` in the constrained values: per layer `feature.Z`,
    `q_mu`, the kernel's `variance` and `lengthscales`, a White part's `variance` — the pairs DGP_Collapsed over an SGPMC layer gives —
    then the likelihood's parameter where it has one.  X = Y = None: the next minibatch.  zs: explicit draws per sampled layer,
    broadcastable to (S, N, D_out); else Philox draws under the model's next seed, or under the seed `fix_draws(seed)` pinned
    (`fix_draws(None)` releases it), so that finite differences and replays see one function.  Test sets go through in row batches
    that fit `scratch_budget` bytes of scratch."""
    supports_gradients = False
    scratch_budget = 1 << 30

    def __init__(self, X, Y, likelihood, layers, minibatch_size=None, num_samples=1, num_data=None, **kwargs):
        layers = list(layers)
        if not layers or len(layers) > _lib.DSDGP_MAX_LAYERS:
            raise ValueError(f"DGP_SGPMC: 1 .. {_lib.DSDGP_MAX_LAYERS} layers, not {len(layers)}")
        for layer in layers:
            if not isinstance(layer, SGPMC_Layer):
                raise ValueError(f"DGP_SGPMC: every layer is an SGPMC_Layer, not {type(layer).__name__}: layers with a q_sqrt are the "
                                 "engine's (DGP), dense and collapsed ones DGP_Heinonen's and DGP_Collapsed's")
            layer._check_mean("DGP_SGPMC")
        if layers[-1].input_prop_dim:
            raise ValueError("DGP_SGPMC: the last layer propagates no inputs (input_prop_dim): its outputs are the likelihood's")
        likelihood_entry(likelihood)
        DGP_Base.__init__(self, X, Y, likelihood, layers, minibatch_size=minibatch_size, num_samples=num_samples, num_data=num_data, **kwargs)
        for layer in layers:
            object.__setattr__(layer, "_model", weakref.ref(self))
        object.__setattr__(self, "_fixed_seed", None)
        object.__setattr__(self, "_scratch", None)

    def engine(self):
        raise NotImplementedError("DGP_SGPMC.engine: there is no device engine over SGPMC layers — the engine's KL tail reads a q_sqrt from "
                                  "every layer record; the stack runs as one library call of its own (dsdgp_stack_propagate / "
                                  "dsdgp_stack_logdensity): use propagate, predict_*, compute_log_density[_gradients], training.SGHMC")

    def train_step(self, *args, **kwargs):
        raise NotImplementedError("DGP_SGPMC.train_step: the model is sampled, not optimised on a bound: training.SGHMC")

    _score_context = DGP_Base._context

    def randn(self, shape, seed=None):
        """N(0, 1) draws for Layer.sample_from_conditional without z, under this model's seed sequence"""
        return self._randn(shape, self._eval_seed() if seed is None else seed, 0)

    def fix_draws(self, seed):
        """pin the Philox seed of every evaluation that is given no zs (None: back to a fresh seed per evaluation)"""
        object.__setattr__(self, "_fixed_seed", None if seed is None else int(seed))

    def _eval_seed(self):
        return self._draw_seed() if self._fixed_seed is None else self._fixed_seed

    # ------------------------------------------------------------------ the library's view of the model
    def parameter_list(self):
        """[(Parameter, its block of the flat gradient: layer index or None, key)] in the order of compute_log_density_gradients: per
        layer `feature.Z`, `q_mu`, kernel `variance`, `lengthscales`, a White part's `variance`; then the likelihood's parameter"""
        out = [(p, l, k) for l, layer in enumerate(self.layers) for p, k in layer_parameters(layer, mean=False)]
        par = likelihood_entry(self.likelihood.likelihood)[1]
        return out + ([(par, None, "lik")] if par is not None else [])

    def _stack_desc(self, ctx):
        """(StackDesc at the Parameters' current values, what its pointers point to: keep it until the device is done)"""
        from . import settings
        from .layers import _kernel_spec
        keep = []
        if ctx.lib.dsdgp_sizeof_stack_desc() != C.sizeof(_lib.StackDesc):
            raise _lib.DsdgpError("_lib.StackDesc does not mirror dsdgp_stack_desc as the library was compiled")
        d = _lib.StackDesc()
        d.L = len(self.layers)
        d.lik_kind, d.lik_p0, d.lik_p1 = likelihood_args(self.likelihood.likelihood)
        d.lik_width = self.layers[-1].num_outputs
        d.jitter = float(settings.jitter)
        mean_kind = {"zero": _lib.MEAN_ZERO, "identity": _lib.MEAN_IDENTITY, "linear": _lib.MEAN_LINEAR}
        for l, layer in enumerate(self.layers):
            layer._check_mean("DGP_SGPMC")
            spec, ls = _kernel_spec(layer.kern)
            Z, q = ctx.to_device(layer.feature.Z.value), ctx.to_device(layer.q_mu.value)
            if Z.shape[1] != spec.input_dim:
                raise ValueError(f"DGP_SGPMC: layer {l}: Z is {tuple(Z.shape)}, the kernel's input_dim {spec.input_dim}")
            y = d.layers[l]
            y.kern, y.Z, y.q_mu = spec, Z.data_ptr(), q.data_ptr()
            y.M, y.DO, y.white, y.input_prop_dim = Z.shape[0], layer.num_outputs, int(layer.white), int(layer.input_prop_dim or 0)
            kind = getattr(layer.mean_function, "kind", None)
            if kind not in mean_kind:
                raise NotImplementedError(f"DGP_SGPMC: mean function {type(layer.mean_function).__name__}: Zero, Identity and a fixed Linear")
            y.mean_kind = mean_kind[kind]
            keep += [ls, Z, q]
            if kind == "linear":
                A = ctx.to_device(layer.mean_function.A.value)
                if tuple(A.shape) != (spec.input_dim, layer.num_outputs):
                    raise ValueError(f"DGP_SGPMC: layer {l}: Linear mean function: A is {tuple(A.shape)}, the layer maps "
                                     f"{spec.input_dim} -> {layer.num_outputs}")
                y.mean_A = A.data_ptr()
                keep.append(A)
                if np.any(layer.mean_function.b.value != 0.0):
                    b = ctx.to_device(layer.mean_function.b.value)
                    y.mean_b = b.data_ptr()
                    keep.append(b)
            elif kind == "identity" and spec.input_dim != layer.num_outputs:
                raise ValueError(f"DGP_SGPMC: layer {l}: an Identity mean function needs as many outputs as inputs, not "
                                 f"{spec.input_dim} -> {layer.num_outputs}")
        return d, keep

    def _scratch_bytes(self, ctx, d, n, S, reverse):
        """the scratch the stack takes on n rows, or None where the library refuses the size"""
        need = C.c_int64()
        rc = ctx.lib.dsdgp_stack_scratch_bytes(C.byref(d), n, S, int(reverse), C.byref(need))
        if rc == _lib.ERR_UNSUPPORTED and not reverse:
            return None
        _lib.check(rc)
        return need.value

    def _scratch_block(self, ctx, nbytes):
        if self._scratch is None or self._scratch.numel() * 8 < nbytes:
            object.__setattr__(self, "_scratch", None)
            object.__setattr__(self, "_scratch", ctx.empty(nbytes // 8 + 32))
        return self._scratch

    def _device_zs(self, ctx, zs, n, S, keep):
        """the ctypes array of L draw pointers ((S n, D_out) each, row s n + i) from zs (None, or per layer None / an array or tensor
        broadcastable to (S, n, D_out))"""
        L = len(self.layers)
        arr = (C.c_void_p * L)()
        if zs is None:
            return arr
        for l, z in enumerate(list(zs)[:L - 1]):
            if z is None:
                continue
            DO = self.layers[l].num_outputs
            if hasattr(z, "data_ptr"):
                t = ctx.as_device(z).expand(S, n, DO).reshape(S * n, DO).contiguous()
            else:
                t = ctx.to_device(np.broadcast_to(np.asarray(z, dtype=np.float64), (S, n, DO)).reshape(S * n, DO))
            keep.append(t)
            arr[l] = t.data_ptr()
        return arr

    # ------------------------------------------------------------------ dgp.py:61-76
    def propagate_device(self, X, S=1, zs=None, want=("F", "mean", "var"), seed=None):
        """dsdgp_stack_propagate on X (numpy or a device tensor, (n, D_in)) -> {"F", "mean", "var"}: per asked-for key the list over the
        layers of device tensors (S n, .), row s n + i — F with its propagated columns, var ONE column (S n,) — without waiting for
        them.  CholeskyError if some layer's Ku is not positive definite: nothing is written then."""
        ctx = self._context()
        Xd = ctx.as_device(X)
        n, S, L = Xd.shape[0], int(S), len(self.layers)
        d, keep = self._stack_desc(ctx)
        nbytes = self._scratch_bytes(ctx, d, n, S, False)
        if nbytes is None:
            raise _lib.DsdgpError(f"DGP_SGPMC: {n} rows x {S} samples take more than 8 GB of scratch: pass the rows in batches")
        scr = self._scratch_block(ctx, nbytes)
        out, ptrs = {}, {}
        for k in ("F", "mean", "var"):
            ptrs[k] = (C.c_void_p * L)()
            if k in want:
                out[k] = []
                for l, layer in enumerate(self.layers):
                    w = layer.num_outputs + (int(layer.input_prop_dim or 0) if k == "F" else 0)
                    t = ctx.empty(S * n) if k == "var" else ctx.empty(S * n, w)
                    out[k].append(t)
                    ptrs[k][l] = t.data_ptr()
        zarr = self._device_zs(ctx, zs, n, S, keep)
        _lib.check(ctx.lib.dsdgp_stack_propagate(ctx.handle, C.byref(d), C.c_void_p(Xd.data_ptr()), n, S, zarr,
                                                 C.c_uint64(self._eval_seed() if seed is None else int(seed)), C.c_void_p(scr.data_ptr()),
                                                 nbytes, ptrs["F"], ptrs["mean"], ptrs["var"], C.byref(C.c_int(0))))
        object.__setattr__(self, "_keep", (keep, Xd))
        return out

    def _row_batch(self, ctx, N, S):
        """rows per batch: the most (up to N) whose scratch fits scratch_budget"""
        d, keep = self._stack_desc(ctx)
        nb = N
        while nb > 1:
            need = self._scratch_bytes(ctx, d, nb, S, False)
            if need is not None and need <= self.scratch_budget:
                break
            nb = (nb + 1) // 2
        return nb

    def _batches(self, X, S, zs):
        """(a, b, the batch's zs) over the row batches of X"""
        ctx = self._context()
        N = X.shape[0]
        nb = self._row_batch(ctx, N, int(S))
        for a in range(0, N, nb):
            b = min(a + nb, N)
            zb = None
            if zs is not None:
                zb = [z if z is None or np.ndim(z) < 2 or np.shape(z)[-2] == 1 else z[..., a:b, :] for z in zs]
            yield a, b, zb

    def propagate(self, X, full_cov=False, S=1, zs=None):
        S = int(S)
        Xh = X.cpu().numpy() if hasattr(X, "data_ptr") else np.asarray(X, dtype=np.float64)
        if full_cov:                                                # the host layer loop of dgp.py:69-74, as DGP_Base.propagate
            return propagate_layers(self.layers, np.tile(Xh[None], [S, 1, 1]), zs, full_cov=True)
        ctx = self._context()
        N, L = Xh.shape[0], len(self.layers)
        widths = [(layer.num_outputs, int(layer.input_prop_dim or 0)) for layer in self.layers]
        Fs, Fmeans, Fvars = ([np.empty((S, N, DO)) for DO, p in widths] for _ in range(3))
        for a, b, zb in self._batches(Xh, S, zs):
            r = self.propagate_device(Xh[a:b], S, zs=zb)
            ctx.sync()
            for l, (DO, p) in enumerate(widths):
                Fs[l][:, a:b] = r["F"][l].cpu().numpy().reshape(S, b - a, p + DO)[:, :, p:]     # its propagated columns come back below
                Fmeans[l][:, a:b] = r["mean"][l].cpu().numpy().reshape(S, b - a, DO)
                Fvars[l][:, a:b] = r["var"][l].cpu().numpy().reshape(S, b - a, 1)
        prepend_input_prop(np.tile(Xh[None], [S, 1, 1]), self.layers, Fs, Fmeans, Fvars)       # layers.py:105-117
        return Fs, Fmeans, Fvars

    def _build_predict(self, X, full_cov=False, S=1, zs=None):
        _, Fmeans, Fvars = self.propagate(X, full_cov=full_cov, S=S, zs=zs)
        return Fmeans[-1], Fvars[-1]

    # ------------------------------------------------------------------ dgp.py:92-98 and the priors of layers.py:257
    def log_density_device(self, X=None, Y=None, zs=None, with_grad=False, seed=None):
        """dsdgp_stack_logdensity -> (out, grad): device tensors, out (4,) = [log density, data term, priors, 0], grad flat in the
        library's layout or None; the host has waited for neither.  CholeskyError: nothing was written."""
        ctx = self._context()
        if X is None:
            Xd, Yd = self.next_minibatch()
        else:
            if not hasattr(Y, "data_ptr"):
                self.likelihood.check_targets(Y)
            Xd, Yd = ctx.as_device(X), ctx.as_device(Y)
        n, S = Xd.shape[0], self.num_samples
        if Yd.dim() != 2 or Yd.shape[0] != n:
            raise ValueError(f"X has {n} rows, Y {tuple(Yd.shape)}")
        d, keep = self._stack_desc(ctx)
        nbytes = self._scratch_bytes(ctx, d, n, S, with_grad)
        scr = self._scratch_block(ctx, nbytes)
        out = ctx.empty(4)
        grad = None
        if with_grad:
            grad = ctx.empty(self._gradient_layout()[2])
        zarr = self._device_zs(ctx, zs, n, S, keep)
        _lib.check(ctx.lib.dsdgp_stack_logdensity(ctx.handle, C.byref(d), C.c_void_p(Xd.data_ptr()), C.c_void_p(Yd.data_ptr()), n, S, zarr,
                                                  C.c_uint64(self._eval_seed() if seed is None else int(seed)),
                                                  float(self.num_data) / float(n), C.c_void_p(scr.data_ptr()), nbytes,
                                                  C.c_void_p(out.data_ptr()), C.c_void_p(grad.data_ptr() if with_grad else 0),
                                                  C.byref(C.c_int(0))))
        object.__setattr__(self, "_keep", (keep, Xd, Yd))
        return out, grad

    def _out4(self, X, Y, zs):
        out, _ = self.log_density_device(X, Y, zs)
        self._context().sync()
        return out.cpu().numpy()

    def _build_likelihood(self, X=None, Y=None, zs=None, with_grad=False, **kwargs):
        if with_grad:
            raise NotImplementedError("DGP_SGPMC._build_likelihood(with_grad=True) would leave a gradient in an engine, which the model "
                                      "does not have: compute_log_density_gradients")
        return float(self._out4(X, Y, zs)[1])

    def compute_log_prior(self):
        """the standard-normal priors of every layer's q_mu (layers.py:257); host arithmetic on the Parameters"""
        return float(sum(layer.log_prior() for layer in self.layers))

    def compute_log_density(self, X=None, Y=None, zs=None):
        return float(self._out4(X, Y, zs)[0])

    def _gradient_layout(self):
        return stack_gradient_layout([(*layer.feature.Z.shape, layer.num_outputs, bool(split_kernel(layer.kern)[0].ARD))
                                      for layer in self.layers])

    def split_gradient(self, grad):
        """the flat gradient of the library (a numpy array) as [(Parameter, gradient), ...] in the order of parameter_list()"""
        blocks, lik, _ = self._gradient_layout()
        out = []
        for p, l, k in self.parameter_list():
            at, shape = blocks[l][k] if l is not None else (lik, (1,))
            out.append((p, np.array(grad[at:at + int(np.prod(shape))], dtype=np.float64).reshape(p.shape)))
        return out

    def compute_log_density_gradients(self, X=None, Y=None, zs=None):
        """(log density, [(Parameter, gradient), ...]) of one evaluation: the next minibatch (or X, Y), S = num_samples draws"""
        out, grad = self.log_density_device(X, Y, zs, with_grad=True)
        self._context().sync()
        return float(out.cpu().numpy()[0]), self.split_gradient(grad.cpu().numpy())

    # ------------------------------------------------------------------ scoring over posterior samples
    def _states(self, run):
        """the kept states of a run of training.SGHMC as a list of assignments [(Parameter, value), ...]; None: the current state"""
        if run is None:
            return [[]]
        T = len(run["logprobs"])
        return [[(p, run["samples"][name][t]) for name, p in zip(run["names"], run["variables"])] for t in range(T)]

    def components_device(self, Xs, S, run=None, zs=None):
        """The last layer's mean and variance (T S N, D_Y each — the one variance column repeated — row (t S + s) N + i) as device
        tensors: every kept state of `run` set in turn (the model is left at the last), S components each.  The form every mixture
        primitive takes, with T S components."""
        ctx = self._context()
        means, vars_ = [], []
        DY = self.layers[-1].num_outputs
        for state in self._states(run):
            for p, v in state:
                p.assign(v)
            r = self.propagate_device(Xs, S, zs=zs, want=("mean", "var"))
            means.append(r["mean"][-1])
            vars_.append(r["var"][-1][:, None].expand(-1, DY))
        return ctx.torch.cat(means, 0).contiguous(), ctx.torch.cat(vars_, 0).contiguous(), len(means) * int(S)

    def _score_batches(self, ctx, Xd, Yd, S, batch_size=None, run=None):
        """(a, b, launch) over the row batches of Xd that fit the scratch, then one synchronisation: DGP_Base's scoring bodies on
        components_device.  launch(what, ...) is the batch's one mixture call _MIXTURE[what] on the T S components of its rows."""
        # (kind, p0, p1) are read before a state of `run` is assigned: the states may move the likelihood's parameter
        fixed = dict(lik=likelihood_args(self.likelihood.likelihood), D=self.layers[-1].num_outputs)
        N = Xd.shape[0]
        nb = self._row_batch(ctx, N, S)
        keep = []
        for a in range(0, N, nb):
            b = min(a + nb, N)
            mean, var, comps = self.components_device(Xd[a:b], S, run)
            m = dict(fixed, mean=mean, var=var, Y=None if Yd is None else Yd[a:b].contiguous(), n=b - a, comps=comps)
            keep.append(m)
            yield a, b, lambda what, *args, **kw: _MIXTURE[what](ctx, m, *args, **kw)
        ctx.sync()

    def predict_y_samples(self, Xs, S, run):
        """(mean, variance) of y for every component: (T S, N*, D_Y) arrays, the likelihood's predict_mean_and_var of each kept state's
        S components (dgp.py:116-119)"""
        ctx = self._context()
        Xd = ctx.as_device(Xs)
        N, DY = Xd.shape[0], self.layers[-1].num_outputs
        if N < 1:
            raise ValueError(f"Xs has {N} rows, Ys None")
        outs = [(a, b, launch("components")) for a, b, launch in self._score_batches(ctx, Xd, None, int(S), run=run)]
        comps = outs[0][2]["comps"]
        m, v = np.empty((comps, N, DY)), np.empty((comps, N, DY))
        for a, b, r in outs:
            m[:, a:b], v[:, a:b] = self.likelihood.predict_mean_and_var(r["mean"].cpu().numpy().reshape(comps, b - a, DY),
                                                                        r["var"].cpu().numpy().reshape(comps, b - a, DY))
        return m, v

    def predict_density(self, Xnew, Ynew, num_samples, run=None):
        """dgp.py:121-126: logsumexp over the components of log p(y | f) minus the logarithm of their number, (N*, D); with `run` the
        components are the T num_samples of its kept states"""
        if run is None:
            return DGP_Base.predict_density(self, Xnew, Ynew, num_samples)
        ctx = self._context()
        N, DY = Xnew.shape[0], self.layers[-1].num_outputs
        mean, var, comps = self.components_device(Xnew, num_samples, run)
        ctx.sync()
        return self.likelihood.predict_density_logmeanexp(mean.cpu().numpy().reshape(comps, N, DY), var.cpu().numpy().reshape(comps, N, DY),
                                                          np.asarray(Ynew, dtype=np.float64))

    def evaluate(self, Xs, Ys, S, run=None, Y_std=1.0, return_rows=False):
        """Held-out scores of the mixture of the T S components of `run` (None: the S of the current state) by dsdgp_eval_mixture: the
        dict of DGP_Base.evaluate — `rmse` / `rmse_per_output` (MultiClass: `error_rate`), `log_density`, `n`, and with return_rows
        `rows` (N*, D, 3)."""
        return self._evaluate(Xs, Ys, S, Y_std, return_rows, run=run)

    def predict_quantiles(self, Xnew, S, probs=(0.025, 0.5, 0.975), level="y", run=None, Y_std=1.0, Y_mean=0.0):
        """Quantiles of the predictive mixture of the T S Gaussians of `run` (dsdgp_mixture_quantiles): (N*, D, P), as
        DGP_Base.predict_quantiles"""
        return self._predict_quantiles(Xnew, S, probs, level, Y_std, Y_mean, run=run)

    def calibration(self, Xs, Ys, S, probs=(0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975), run=None, Y_std=1.0, return_rows=False):
        """Calibration scores of held-out targets under the mixture of the T S Gaussians of `run` (dsdgp_mixture_calibration; Gaussian
        likelihood): the dict of DGP_Base.calibration"""
        return self._calibration(Xs, Ys, S, probs, Y_std, return_rows, run=run)

    def classification_report(self, Xs, Ys, S, bins=10, run=None, return_rows=False):
        """The classification report of the mixture class probabilities over the T S components of `run`
        (dsdgp_mixture_classification; MultiClass or Bernoulli): the dict of DGP_Base.classification_report"""
        return self._classification_report(Xs, Ys, S, bins, return_rows, run=run)


# What one batch of DGP_SGPMC's scoring launches for a reduction, with the trailing arguments of Engine.<what>_batch.  m: the batch's
# device means and variances (comps n, D), its targets, and the likelihood's (kind, p0, p1): p0 is the Gaussian's noise variance, which
# level "y" of the quantiles and the calibration (both refused for any other likelihood) add to every component.
def _mixture_evaluate(ctx, m, acc, accumulate, rows=None):
    _lib.check(ctx.lib.dsdgp_eval_mixture(ctx.handle, *m["lik"], ptr(m["mean"]), ptr(m["var"]), ptr(m["Y"]), m["n"], m["comps"], m["D"],
                                          ptr(rows), ptr(acc), int(accumulate)))


def _mixture_quantiles(ctx, m, probs, q, level=1):
    _lib.check(ctx.lib.dsdgp_mixture_quantiles(ctx.handle, ptr(m["mean"]), ptr(m["var"]), m["lik"][1] if level else 0.0, m["n"], m["comps"],
                                               m["D"], probs.ctypes.data_as(_lib.c_double_p), probs.size, ptr(q)))


def _mixture_calibration(ctx, m, probs, acc, accumulate, rows=None):
    _lib.check(ctx.lib.dsdgp_mixture_calibration(ctx.handle, ptr(m["mean"]), ptr(m["var"]), m["lik"][1], ptr(m["Y"]), m["n"], m["comps"],
                                                 m["D"], probs.ctypes.data_as(_lib.c_double_p), probs.size, ptr(rows), ptr(acc),
                                                 int(accumulate)))


def _mixture_classification(ctx, m, bins, acc, accumulate, probs=None, rows=None):
    _lib.check(ctx.lib.dsdgp_mixture_classification(ctx.handle, m["lik"][0], ptr(m["mean"]), ptr(m["var"]), ptr(m["Y"]), m["n"], m["comps"],
                                                    m["D"], bins, ptr(probs), ptr(rows), ptr(acc), int(accumulate)))


_MIXTURE = {"evaluate": _mixture_evaluate, "quantiles": _mixture_quantiles, "calibration": _mixture_calibration,
            "classification": _mixture_classification, "components": lambda ctx, m: m}


def stack_gradient_layout(shapes):
    """The flat gradient of dsdgp_stack_logdensity, stated once: per layer (M, D, DO, ard) the blocks `Z` (M D), `q_mu` (M DO),
    `variance`, `lengthscales` (D with ARD, else one), `white_variance`, then one entry for the likelihood
    -> ([{key: (offset, shape)} per layer], the likelihood's offset, the total)."""
    layers, at = [], 0
    for M, D, DO, ard in shapes:
        blocks = {}
        for key, shape in (("Z", (M, D)), ("q_mu", (M, DO)), ("variance", (1,)), ("lengthscales", (D if ard else 1,)), ("white_variance", (1,))):
            blocks[key] = (at, shape)
            at += int(np.prod(shape))
        layers.append(blocks)
    return layers, at, at + 1
