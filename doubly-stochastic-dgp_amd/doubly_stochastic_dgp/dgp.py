"""Host mirror of the reference's model classes (dgp.py:35-192): `DGP_Base`, `DGP` with the same constructors and the
`propagate / _build_predict / E_log_p_Y / _build_likelihood / compute_log_likelihood / predict_*` surface.  Every
evaluation is one libdsdgp call (HIP kernels on gfx950); this file holds shapes, minibatching and bookkeeping only."""
import ctypes as C

import numpy as np

from . import _lib
from .engine import Context
from .gpflow_compat import Gaussian, MultiClass, Parameterized, Zero
from .layer_initializations import greedy_inducing, init_layers_linear, kmeans_inducing
from .layers import prepend_input_prop, propagate_layers
from .distributed import shard_terms
from .utils import BroadcastingLikelihood


class Minibatch:
    """[UPSTREAM] gpflow.params.Minibatch(value, batch_size, seed): epoch-wise shuffled minibatches.  X and Y use the
    same seed (dgp.py:51-52) so rows stay paired; TF's shuffle order itself is not reproducible, so this uses its own
    numpy Generator.  The data stays resident on the device; only the int64 row indices are produced on the host."""

    def __init__(self, n_rows, batch_size, seed=0):
        self.n_rows, self.batch_size = int(n_rows), int(batch_size)
        self.rng = np.random.default_rng(seed)
        self._perm = None
        self._pos = 0
        self._epoch = 0

    def _new_epoch(self):
        """Draw the next epoch's permutation.  EVERY regeneration bumps the epoch counter: callers key their device copy of
        the permutation on it (a minibatch that straddles an epoch boundary regenerates inside next_indices)."""
        self._perm = self.rng.permutation(self.n_rows)
        self._pos = 0
        self._epoch += 1

    def next_span(self):
        """(epoch permutation, start) of the next minibatch when it lies inside one epoch, else None (caller falls back to
        next_indices).  Lets the device keep one uploaded permutation per epoch instead of one index upload per step."""
        if self._perm is None or self._pos >= self.n_rows:
            self._new_epoch()
        if self._pos + self.batch_size > self.n_rows:
            return None
        start = self._pos
        self._pos += self.batch_size
        return self._perm, start, self._epoch

    def next_chunk(self, k):
        """The indices of the next k minibatches, concatenated (k * batch_size,)."""
        return np.concatenate([self.next_indices() for _ in range(int(k))])

    def next_indices(self):
        out = []
        need = self.batch_size
        while need > 0:
            if self._perm is None or self._pos >= self.n_rows:
                self._new_epoch()
            take = min(need, self.n_rows - self._pos)
            out.append(self._perm[self._pos:self._pos + take])
            self._pos += take
            need -= take
        return np.concatenate(out).astype(np.int64)


class DGP_Base(Parameterized):
    """dgp.py:35-126."""

    def __init__(self, X, Y, likelihood, layers, minibatch_size=None, num_samples=1, num_data=None, **kwargs):
        self.num_samples = int(num_samples)
        self.X_data = np.ascontiguousarray(X, dtype=np.float64)
        self.Y_data = np.ascontiguousarray(Y, dtype=np.float64)
        self.num_data = num_data or self.X_data.shape[0]                        # dgp.py:49
        self.minibatch_size = int(minibatch_size) if minibatch_size else None
        self._minibatch = Minibatch(self.X_data.shape[0], self.minibatch_size, seed=0) if self.minibatch_size else None
        self.likelihood = BroadcastingLikelihood(likelihood)                    # dgp.py:57
        self.likelihood.check_targets(self.Y_data)
        self.layers = list(layers)                                              # dgp.py:59
        self.white = bool(self.layers[0].white) if self.layers else False
        object.__setattr__(self, "_eng", None)
        object.__setattr__(self, "_dev_data", None)
        self._seed = 0
        # data-parallel hooks (distributed.py): (rank, world_size, all_reduce_fn)
        object.__setattr__(self, "_dist", None)

    # ------------------------------------------------------------------ engine / data plumbing
    def engine(self):
        if self._eng is None:
            from .engine import Engine
            n0 = self.minibatch_size or self.X_data.shape[0]
            eng = Engine(self.layers, self.likelihood.likelihood, self.white, n_max=n0, s_max=self.num_samples)
            for i, layer in enumerate(self.layers):
                object.__setattr__(layer, "_model_engine", (eng, i))
            object.__setattr__(self, "_eng", eng)
        return self._eng

    def _context(self):
        return Context.get()

    def _device_data(self):
        if self._dev_data is None:
            ctx = self._context()
            object.__setattr__(self, "_dev_data", (ctx.to_device(self.X_data), ctx.to_device(self.Y_data)))
        return self._dev_data

    def _randn(self, shape, seed, stream):
        """dsdgp_randn(seed, stream) as a numpy array: where a model without an engine over all its layers draws for
        Layer.sample_from_conditional without z"""
        ctx = self._context()
        n = int(np.prod(shape))
        out = ctx.empty(n)
        _lib.check(ctx.lib.dsdgp_randn(ctx.handle, C.c_uint64(seed), C.c_uint64(stream), n, C.c_void_p(out.data_ptr())))
        ctx.sync()
        return out.cpu().numpy().reshape(shape)

    def _next_seed(self):
        self._seed += 1
        return self._seed

    def _draw_seed(self):
        """Philox seed of the next device evaluation: distinct across calls and across the ranks of a data-parallel run (every call
        draws the streams 0 .. L-1 under it).  One formula at every call site: a prediction seed of plain _next_seed() equalled an
        earlier training seed t * world + rank of its own rank or of another one once world > 1.  (world = 1: 1, 2, 3, ...)"""
        rank, world = self._dist[:2] if self._dist else (0, 1)
        return self._next_seed() * world + rank

    def _next_index_span(self):
        """(device index tensor, offset, n) of the next minibatch.  The row indices of the next CHUNK minibatches are drawn on the
        host in one go and uploaded once (pinned, asynchronous); a step then only moves an offset.  One upload per epoch (or per step
        when a minibatch straddles an epoch boundary — 2 of every 7 steps at 7372 / 1000) stalled the host behind the stream and the
        GPU behind the host: ~50 us on each such step."""
        Xd, _ = self._device_data()
        ctx = self._context()
        mb = self._minibatch
        if getattr(self, "_idx_src", None) is not mb or self._idx_pos >= self._idx_cnt:
            k = max(1, min(512, (1 << 18) // max(1, mb.batch_size)))
            host = ctx.torch.from_numpy(mb.next_chunk(k))
            try:
                host = host.pin_memory()
            except RuntimeError:
                pass
            self._idx_host = host                                  # alive until the copy has run
            # on the library's stream (ctx.tstream), whatever stream the caller has made current: the gather that reads the indices
            # is ordered behind this copy only there
            with ctx.torch.cuda.stream(ctx.tstream):
                self._idx_dev = host.to(Xd.device, non_blocking=True)
            self._idx_src, self._idx_pos, self._idx_cnt = mb, 0, k
        off = self._idx_pos * mb.batch_size
        self._idx_pos += 1
        return self._idx_dev, off, mb.batch_size

    def next_minibatch(self):
        """Device tensors (Xb, Yb) of the next minibatch (dgp.py:51-52), or the full data when not minibatching."""
        Xd, Yd = self._device_data()
        if self._minibatch is None:
            return Xd, Yd
        ctx = self._context()
        idx, off, n = self._next_index_span()
        Xb, Yb = ctx.empty(n, Xd.shape[1]), ctx.empty(n, Yd.shape[1])
        _lib.check(ctx.lib.dsdgp_gather_rows2(ctx.handle, C.c_void_p(Xd.data_ptr()), Xd.shape[1], C.c_void_p(Xb.data_ptr()),
                                              C.c_void_p(Yd.data_ptr()), Yd.shape[1], C.c_void_p(Yb.data_ptr()),
                                              C.c_void_p(idx.data_ptr()), n, off))
        self._keep_idx = idx
        return Xb, Yb

    @staticmethod
    def _np(ts):
        return [t.cpu().numpy() for t in ts]

    # ------------------------------------------------------------------ dgp.py:61-76
    def propagate(self, X, full_cov=False, S=1, zs=None):
        eng = self.engine()
        if full_cov:
            # plotting path (dgp.py:104-114): the layer loop of dgp.py:69-74 with (S,N,N,D) covariances, on the host
            return propagate_layers(self.layers, np.tile(np.asarray(X, dtype=np.float64)[None], [int(S), 1, 1]), zs, full_cov=True)
        Fs, Fmeans, Fvars = eng.propagate(X, int(S), zs=zs, seed=self._draw_seed())
        eng.ctx.sync()
        Fs, Fmeans, Fvars = self._np(Fs), self._np(Fmeans), self._np(Fvars)
        if any(layer.input_prop_dim for layer in self.layers):
            Xh = X.cpu().numpy() if hasattr(X, "data_ptr") else np.asarray(X, dtype=np.float64)
            prepend_input_prop(np.tile(Xh[None], [int(S), 1, 1]), self.layers, Fs, Fmeans, Fvars)
        return Fs, Fmeans, Fvars

    # dgp.py:78-81
    def _build_predict(self, X, full_cov=False, S=1, zs=None):
        if full_cov:
            _, Fmeans, Fvars = self.propagate(X, full_cov=True, S=S, zs=zs)
            return Fmeans[-1], Fvars[-1]
        eng = self.engine()
        _, Fmeans, Fvars = eng.propagate(X, int(S), zs=zs, seed=self._draw_seed(), want=("mean", "var"))
        eng.ctx.sync()
        return Fmeans[-1].cpu().numpy(), Fvars[-1].cpu().numpy()

    # dgp.py:83-90
    def E_log_p_Y(self, X, Y, zs=None):
        Fmean, Fvar = self._build_predict(X, full_cov=False, S=self.num_samples, zs=zs)
        return self.likelihood.variational_expectations_mean(Fmean, Fvar, np.asarray(Y, dtype=np.float64))

    # dgp.py:92-98
    def _build_likelihood(self, X=None, Y=None, zs=None, with_grad=False, grad_from_layer=0, grad_q_only=False):
        eng = self.engine()
        if X is None:
            X, Y = self.next_minibatch()
        elif not hasattr(Y, "data_ptr"):
            self.likelihood.check_targets(Y)
        n_local = X.shape[0]
        rank, world, allreduce = self._dist if self._dist else (0, 1, None)
        scale, klw = shard_terms(self.num_data, n_local, world)                 # dgp.py:96-97
        hook = getattr(self, "_dist_before_elbo", None)
        if hook is not None and allreduce is not None:
            eng._ensure(n_local, self.num_samples)
            eng._upload_if_needed()            # may re-create the device model (layout / jitter change): before the hook looks at it
            hook(eng)
        out = eng.elbo(X, Y, self.num_samples, zs=zs, seed=self._draw_seed(), data_scale=scale,
                       kl_weight=klw, with_grad=with_grad, sync=allreduce is None, grad_from_layer=grad_from_layer,
                       grad_q_only=grad_q_only)
        if allreduce is not None:
            out = allreduce(eng, with_grad)
            if out[3] != 0.0:          # every rank factorises the same Kuu ([UPSTREAM] tf.cholesky raises)
                raise _lib.CholeskyError(f"Cholesky decomposition was not successful (Kuu pivot {int(out[3])})")
        return float(out[0])

    def compute_log_likelihood(self, X=None, Y=None, zs=None):
        """[UPSTREAM] Model.compute_log_likelihood: evaluates _build_likelihood (one MC draw of the ELBO)."""
        return self._build_likelihood(X, Y, zs)

    def train_step(self, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, X=None, Y=None, zs=None, sync=False):
        """One optimiser step of -ELBO: minibatch gather + forward + reverse-mode gradient + Adam
        (one `session.run(opt_op)` of demos/demo_regression_UCI.ipynb:324).  Returns the ELBO if sync=True."""
        eng = self.engine()
        rank, world, allreduce = self._dist if self._dist else (0, 1, None)
        if X is None and zs is None and allreduce is None and self._minibatch is not None:
            # the whole step — minibatch gather, ELBO, gradient, Adam — in one library call
            Xd, Yd = self._device_data()
            idx, off, n = self._next_index_span()
            scale, klw = shard_terms(self.num_data, n, 1)
            eng.train_step_minibatch(Xd, Yd, idx, off, n, self.num_samples, seed=self._draw_seed(), data_scale=scale, kl_weight=klw,
                                     lr=lr, beta1=beta1, beta2=beta2, eps=eps)
            return self._sync_result(eng, None, world) if sync else None
        if X is None:
            X, Y = self.next_minibatch()
        elif not hasattr(Y, "data_ptr"):
            self.likelihood.check_targets(Y)
        n_local = X.shape[0]
        scale, klw = shard_terms(self.num_data, n_local, world)
        if allreduce is None:
            # single process: ELBO, gradient and Adam update in one library call (the update rides in the reverse pass's last launch)
            eng.train_step(X, Y, self.num_samples, zs=zs, seed=self._draw_seed(), data_scale=scale, kl_weight=klw, lr=lr, beta1=beta1,
                           beta2=beta2, eps=eps)
            out = None
        else:
            hook = getattr(self, "_dist_before_elbo", None)
            if hook is not None:
                eng._ensure(n_local, self.num_samples)
                eng._upload_if_needed()
                hook(eng)
            out = eng.elbo(X, Y, self.num_samples, zs=zs, seed=self._draw_seed(), data_scale=scale,
                           kl_weight=klw, with_grad=True, sync=False)
            out = allreduce(eng, True, sync=sync)
            eng.adam_step(lr, beta1, beta2, eps)
        return self._sync_result(eng, out, world) if sync else None

    @staticmethod
    def _sync_result(eng, out, world):
        eng.ctx.sync()
        o = eng.out4.cpu().numpy() if out is None else out
        if out is None and world > 1:
            o = o.copy(); o[3] /= world
        if o[3] != 0.0:      # asynchronous steps report a failed Kuu factorisation here ([UPSTREAM] tf.cholesky raises)
            raise _lib.CholeskyError(f"Cholesky decomposition was not successful (Kuu pivot {int(o[3])})")
        return float(o[0])

    # ------------------------------------------------------------------ dgp.py:100-126
    def predict_f(self, Xnew, num_samples):
        return self._build_predict(Xnew, full_cov=False, S=num_samples)

    def predict_f_full_cov(self, Xnew, num_samples):
        return self._build_predict(Xnew, full_cov=True, S=num_samples)

    def predict_all_layers(self, Xnew, num_samples):
        return self.propagate(Xnew, full_cov=False, S=num_samples)

    def predict_all_layers_full_cov(self, Xnew, num_samples):
        return self.propagate(Xnew, full_cov=True, S=num_samples)

    def predict_y(self, Xnew, num_samples):
        Fmean, Fvar = self._build_predict(Xnew, full_cov=False, S=num_samples)
        return self.likelihood.predict_mean_and_var(Fmean, Fvar)

    def predict_density(self, Xnew, Ynew, num_samples):
        Fmean, Fvar = self._build_predict(Xnew, full_cov=False, S=num_samples)
        return self.likelihood.predict_density_logmeanexp(Fmean, Fvar, np.asarray(Ynew, dtype=np.float64))

    def sample_functions(self, num_functions=1, num_features=1024, seed=0):
        """num_functions consistent draws of the model's functions (pathwise.PathwiseFunctions): fs(Xs) is (S, N, D_out), fs.all_layers(Xs)
        every layer's, the same S functions at any inputs in any number of calls; a snapshot, which later training does not change.
        num_features: the frequencies of each layer's random Fourier basis (fs.basis_error(l) says whether they are enough).  No
        reference counterpart.  NotImplementedError for anything but SVGP_Layers under DGP / DGP_Quad without input propagation;
        CholeskyError where a layer's Ku is not positive definite."""
        from .pathwise import PathwiseFunctions
        return PathwiseFunctions(self, num_functions=num_functions, num_features=num_features, seed=seed)

    # ------------------------------------------------------------------ held-out scoring: one front end for every model
    # Each of evaluate, predict_quantiles, calibration and classification_report has ONE body (_evaluate, ...), shared with
    # model_zoo.DGP_SGPMC: refusals before any device is touched, uploads, the accumulator and `rows`, the batch loop, one
    # synchronisation, the host finish.  A model supplies _score_context() and _score_batches(): how rows become batches and what one
    # batch launches for a reduction.  `how` is what the model's _score_batches cuts by: batch_size and zs here, run there.
    MAX_PROBS = 16
    MAX_BINS = 32

    def _score_context(self):
        """the context a scoring call works in, asked for once its arguments have passed: the engine models build their engine here"""
        return self.engine().ctx

    @staticmethod
    def _zs_on_device(ctx, zs):
        if zs is None:
            return None
        return [z if z is None or hasattr(z, "data_ptr") else ctx.to_device(np.asarray(z, dtype=np.float64)) for z in zs]

    def _score_batches(self, ctx, Xd, Yd, S, batch_size=1000, zs=None):
        """(a, b, launch) over the row batches [a, b) of Xd in order, then one synchronisation.  launch(what, ...) is the batch's library
        call Engine.<what>_batch on its rows with zs = the batch's rows of every draw that is not broadcast over rows and seed = one
        `_draw_seed()` per batch, in batch order.  What the calls return (the arrays their asynchronous launches read) is kept alive
        until the synchronisation."""
        eng, zs, keep = self.engine(), self._zs_on_device(ctx, zs), []
        for a in range(0, Xd.shape[0], batch_size):
            b = min(a + batch_size, Xd.shape[0])
            zb = None if zs is None else [z if z is None or z.shape[1] == 1 else z[:, a:b].contiguous() for z in zs]
            seed, data = self._draw_seed(), (Xd[a:b],) if Yd is None else (Xd[a:b], Yd[a:b])
            yield a, b, lambda what, *args, **kw: keep.append(getattr(eng, what + "_batch")(*data, S, *args, zs=zb, seed=seed, **kw))
        ctx.sync()

    @staticmethod
    def _batch_args(num_samples, batch_size):
        S, batch_size = int(num_samples), int(batch_size)
        if batch_size < 1 or S < 1:
            raise ValueError("batch_size and num_samples must be positive")
        return S, batch_size

    def _zs_args(self, zs):
        if zs is not None:
            if len(zs) != len(self.layers):
                raise ValueError("zs needs one entry (or None) per layer")
            if any(z is not None and len(_shape(z)) != 3 for z in zs):
                raise ValueError("z must be rank-3, broadcastable to (S, N, D_out)")

    def _row_args(self, X, Y, width, hint, zs):
        if len(_shape(X)) != 2 or _shape(X)[0] < 1:
            raise ValueError("X must be a non-empty (N, D_in) array")
        if Y is not None and _shape(Y) != (_shape(X)[0], width):
            raise ValueError(f"Ys has shape {_shape(Y)}, expected {(_shape(X)[0], width)}{hint}")
        self._zs_args(zs)

    def evaluate(self, Xs, Ys, num_samples, batch_size=1000, Y_std=1.0, zs=None, return_rows=False):
        """Held-out scores as demos/run_regression.py:108-123 computes them, without leaving the device: over row batches of
        `batch_size` (a ragged last one allowed) the forward pass and the reduction over the `num_samples` mixture components add into
        one device accumulator, read back once at the end.  Xs / Ys: numpy arrays or device tensors.  zs: explicit N(0, 1) draws per
        layer, broadcastable to (S, N*, D_out) (dgp.py:62,68); else one `_draw_seed()` per batch, in batch order.
        Returns a dict: `rmse` = Y_std sqrt(mean((Ys - mhat)^2)) over rows and outputs (run_regression.py:121) and `rmse_per_output`
        (MultiClass: `error_rate` of argmax_k of the mixture class probabilities instead), `log_density` = the mean over rows and
        outputs of logsumexp_S log p(y | .) - log S (dgp.py:121-126), `n`, and with return_rows the (N*, D, 3) array `rows` of
        [mixture mean, mixture variance, log density]."""
        return self._evaluate(Xs, Ys, num_samples, Y_std, return_rows, batch_size=batch_size, zs=zs)

    def _evaluate(self, Xs, Ys, num_samples, Y_std, return_rows, **how):
        S, how["batch_size"] = self._batch_args(num_samples, how.get("batch_size", 1))
        gaussian = not self.likelihood.needs_broadcasting
        Y_std = float(Y_std)
        if not Y_std > 0.0 or (not gaussian and Y_std != 1.0):
            raise ValueError("Y_std rescales a Gaussian density only (and must be positive)")
        if not hasattr(Ys, "data_ptr"):
            self.likelihood.check_targets(Ys)
        N = _shape(Xs)[0]
        if N < 1 or _shape(Ys)[0] != N:
            raise ValueError(f"Xs has {N} rows, Ys {_shape(Ys)[0]}")
        self._zs_args(how.get("zs"))
        ctx = self._score_context()
        Xd, Yd = ctx.as_device(Xs), ctx.as_device(Ys)
        D = self.layers[-1].num_outputs
        acc = ctx.empty(3, D)
        rows = ctx.empty(N, D, 3) if return_rows else None
        for a, b, launch in self._score_batches(ctx, Xd, Yd, S, **how):
            launch("evaluate", acc, a > 0, rows=rows[a:b] if return_rows else None)
        out = {"n": N, **evaluation_scores(acc.cpu().numpy(), isinstance(self.likelihood.likelihood, MultiClass), gaussian, Y_std)}
        if return_rows:
            out["rows"] = rows.cpu().numpy()
        return out

    # ------------------------------------------------------------------ calibration of the predictive mixture
    def _calibration_args(self, what, X, num_samples, probs, batch_size, Y_std, zs, needs_gaussian, Y=None):
        """Everything predict_quantiles / calibration can refuse without a device: (S, batch_size, Y_std, probs as a float64 array).
        Called before any device is touched, so a machine without a GPU reports the bad argument and not the missing device."""
        if needs_gaussian and self.likelihood.needs_broadcasting:
            raise NotImplementedError(f"{what}: the predictive y of {type(self.likelihood.likelihood).__name__} is not a mixture of "
                                      "Gaussians; only level=\"f\" (the latent function) is covered")
        probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        if probs.ndim != 1 or not 1 <= probs.size <= self.MAX_PROBS:
            raise ValueError(f"probs must hold 1 .. {self.MAX_PROBS} probabilities")
        if not np.all((probs > 0.0) & (probs < 1.0)):
            raise ValueError("every probability must lie inside (0, 1)")
        S, batch_size = self._batch_args(num_samples, batch_size)
        Y_std = float(Y_std)
        if not (Y_std > 0.0 and np.isfinite(Y_std)):
            raise ValueError("Y_std must be positive")
        self._row_args(X, Y, self.layers[-1].num_outputs, " (rows of Xs x outputs of the last layer)", zs)
        return S, batch_size, Y_std, np.ascontiguousarray(probs)

    def predict_quantiles(self, Xnew, num_samples, probs=(0.025, 0.5, 0.975), level="y", batch_size=1000, Y_std=1.0, Y_mean=0.0,
                          zs=None):
        """Quantiles of the predictive mixture of `num_samples` Gaussians (dgp.py:116-126), solved on the device: the (N*, D, P) array
        Y_mean + Y_std q with F(q[i, d, k]) = probs[k] — exact where demos/using_natural_gradients.ipynb cell 9 takes np.percentile of
        100 draws and demos/demo_step_function.ipynb:83-85 / demos/priors.ipynb:1020 use mean +- 1.96 sqrt(var).  level "y": the
        observations (Gaussian likelihood only; the noise variance is added), "f": the latent function of any likelihood.  Xnew: numpy
        or a device tensor, in row batches of `batch_size` (a ragged last one allowed).  zs as in `evaluate`; else one `_draw_seed()`
        per batch, in batch order."""
        return self._predict_quantiles(Xnew, num_samples, probs, level, Y_std, Y_mean, batch_size=batch_size, zs=zs)

    def _predict_quantiles(self, Xnew, num_samples, probs, level, Y_std, Y_mean, **how):
        if level not in ("f", "y"):
            raise ValueError(f"level must be \"f\" or \"y\", not {level!r}")
        S, how["batch_size"], Y_std, probs = self._calibration_args("predict_quantiles", Xnew, num_samples, probs, how.get("batch_size", 1),
                                                                    Y_std, how.get("zs"), level == "y")
        ctx = self._score_context()
        Xd = ctx.as_device(Xnew)
        q = ctx.empty(Xd.shape[0], self.layers[-1].num_outputs, probs.size)
        for a, b, launch in self._score_batches(ctx, Xd, None, S, **how):
            launch("quantiles", probs, q[a:b], level=1 if level == "y" else 0)
        return float(Y_mean) + Y_std * q.cpu().numpy()

    def calibration(self, Xs, Ys, num_samples, probs=(0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975), batch_size=1000, Y_std=1.0, zs=None,
                    return_rows=False):
        """Calibration scores of held-out targets under the predictive mixture (Gaussian likelihood), reduced on the device into one
        accumulator over the row batches and read back once.  Returns a dict: `crps` = Y_std x the mean over rows and outputs of the
        closed-form continuous ranked probability score and `crps_per_output`; `pit_le`, (P, D): the fraction of targets whose
        probability integral transform u = F(y) is <= probs[k] (a calibrated model gives probs[k]); `coverage`: for every pair p, 1 - p
        both in probs, {1 - 2p: fraction of targets with p < u <= 1 - p}, the coverage of the central interval, over rows and outputs;
        `n`; with return_rows the (N*, D, 2) array `rows` of [u, CRPS] in model units."""
        return self._calibration(Xs, Ys, num_samples, probs, Y_std, return_rows, batch_size=batch_size, zs=zs)

    def _calibration(self, Xs, Ys, num_samples, probs, Y_std, return_rows, **how):
        S, how["batch_size"], Y_std, probs = self._calibration_args("calibration", Xs, num_samples, probs, how.get("batch_size", 1), Y_std,
                                                                    how.get("zs"), True, Y=Ys)
        ctx = self._score_context()
        Xd, Yd = ctx.as_device(Xs), ctx.as_device(Ys)
        N, D = Xd.shape[0], self.layers[-1].num_outputs
        acc = ctx.empty(2 + probs.size, D)
        rows = ctx.empty(N, D, 2) if return_rows else None
        for a, b, launch in self._score_batches(ctx, Xd, Yd, S, **how):
            launch("calibration", probs, acc, a > 0, rows=rows[a:b] if return_rows else None)
        out = calibration_scores(acc.cpu().numpy(), probs, Y_std)
        out["n"] = N
        if return_rows:
            out["rows"] = rows.cpu().numpy()
        return out

    # ------------------------------------------------------------------ classification report (MultiClass / Bernoulli)
    def _classification_args(self, X, Y, num_samples, bins, batch_size, zs):
        """Everything classification_report can refuse without a device -> (kind, C, ND, S, bins, batch_size); called before any
        device is touched."""
        kind, Cn = self.likelihood.classification_args("classification_report")
        bins = int(bins)
        if not 1 <= bins <= self.MAX_BINS:
            raise ValueError(f"bins must lie in 1 .. {self.MAX_BINS}")
        S, batch_size = self._batch_args(num_samples, batch_size)
        ND = self.layers[-1].num_outputs if self.likelihood.bernoulli else 1
        self._row_args(X, Y, ND, "", zs)
        if not hasattr(Y, "data_ptr"):
            self.likelihood.check_targets(Y)
        return kind, Cn, ND, S, bins, batch_size

    def classification_report(self, Xs, Ys, num_samples, bins=10, batch_size=1000, zs=None, return_rows=False):
        """Is the classifier calibrated, and which classes does it confuse?  Held-out labels scored under the mixture class probabilities
        pi = mean over the `num_samples` components of the likelihood's predictive probabilities (MultiClass: C = K classes, Ys (N*, 1)
        labels; Bernoulli: C = 2 per output, Ys (N*, D), class 1 where Ys == 1), on the device: over row batches of `batch_size` one
        launch forms the probabilities of all classes and components, a second the report, added into one accumulator that is read
        back once.  Xs / Ys: numpy arrays or device tensors.  zs as in `evaluate`; else one `_draw_seed()` per batch, in batch order.
        Returns a dict: `n`; `error_rate` of argmax_c pi_c (ties: the lowest c); `log_density` = mean log pi_y (evaluate's);
        `brier` = mean sum_c (pi_c - [c = y])^2 (the multi-class definition: a binary problem gives 2 (p - t)^2, twice the usual binary
        score); `ece` = sum_b (n_b / n) |accuracy_b - confidence_b| over the non-empty ones of `bins` equal-width bins of the
        confidence max_c pi_c, `mce` the largest such gap; `reliability` = {"edges" (B + 1,), "count", "confidence", "accuracy" (B,)},
        nan in the last two where a bin is empty; `top_k_accuracy` (C,): the fraction of rows whose label is among the k + 1 most
        probable classes; `confusion` (C, C) int64, [true, predicted]; `per_class` = {"recall", "precision", "support"}.  Bernoulli
        with D > 1 outputs: the scalars pooled over outputs, `error_rate_per_output`, `log_density_per_output`, `brier_per_output`,
        `ece_per_output`, `confusion` (D, 2, 2), the reliability and per_class arrays with a leading D.  With return_rows: `probs`
        (N*, K) (Bernoulli: (N*, D), p(y = 1)) and `rows` (N*, ND, 4) = [predicted class, confidence, log pi_y, brier]."""
        return self._classification_report(Xs, Ys, num_samples, bins, return_rows, batch_size=batch_size, zs=zs)

    def _classification_report(self, Xs, Ys, num_samples, bins, return_rows, **how):
        kind, Cn, ND, S, bins, how["batch_size"] = self._classification_args(Xs, Ys, num_samples, bins, how.get("batch_size", 1),
                                                                             how.get("zs"))
        ctx = self._score_context()
        Xd, Yd = ctx.as_device(Xs), ctx.as_device(Ys)
        N, D = Xd.shape[0], self.layers[-1].num_outputs
        acc = ctx.empty(4 + 3 * bins + Cn + Cn * Cn, ND)
        probs = ctx.empty(N, D) if return_rows else None
        rows = ctx.empty(N, ND, 4) if return_rows else None
        for a, b, launch in self._score_batches(ctx, Xd, Yd, S, **how):
            launch("classification", bins, acc, a > 0, probs=probs[a:b] if return_rows else None, rows=rows[a:b] if return_rows else None)
        out = classification_scores(acc.cpu().numpy(), bins, Cn)
        out["n"] = N
        if return_rows:
            out["probs"] = probs.cpu().numpy()
            out["rows"] = rows.cpu().numpy()
        return out


def _shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else np.shape(a)


def evaluation_scores(sums, multiclass, gaussian, Y_std=1.0):
    """The dict of DGP_Base.evaluate (without `n` and `rows`) from the (3, D) accumulator of dsdgp_model_evaluate / dsdgp_eval_mixture."""
    if multiclass:
        cnt = float(sums[2, 0])
        return {"error_rate": float(sums[0, 0]) / cnt, "log_density": float(sums[1, 0]) / cnt}
    cnt = float(sums[2].sum())
    # the model lives in standardised units y = y_orig / Y_std; the density of y_orig is that of y divided by Y_std,
    # N(y c | m c, v c^2) = N(y | m, v) / c, component by component, hence also for the mixture: log p(y_orig) = l - log Y_std
    # (run_regression.py:122 scales targets, means and standard deviations by Y_std before norm.logpdf)
    return {"rmse": Y_std * float(np.sqrt(sums[0].sum() / cnt)), "rmse_per_output": Y_std * np.sqrt(sums[0] / sums[2]),
            "log_density": float(sums[1].sum()) / cnt - (np.log(Y_std) if gaussian else 0.0)}


def classification_scores(sums, bins, C):
    """The dict of DGP_Base.classification_report (without `n`, `probs` and `rows`) from the (4 + 3 bins + C + C^2, ND) accumulator of
    dsdgp_mixture_classification."""
    B, C = int(bins), int(C)
    sums = np.asarray(sums, dtype=np.float64).reshape(4 + 3 * B + C + C * C, -1)
    ND = sums.shape[1]
    cnt = sums[3]
    bc, bcf, bok = sums[4:4 + B], sums[4 + B:4 + 2 * B], sums[4 + 2 * B:4 + 3 * B]
    rank = sums[4 + 3 * B:4 + 3 * B + C]
    conf = np.rint(sums[4 + 3 * B + C:]).astype(np.int64).reshape(C, C, ND)

    def reliability(bc, bcf, bok):      # bins on the leading axis
        with np.errstate(divide="ignore", invalid="ignore"):
            cf, ok = np.where(bc > 0, bcf / bc, np.nan), np.where(bc > 0, bok / bc, np.nan)
        gap = np.where(bc > 0, np.abs(ok - cf), 0.0)
        return cf, ok, (bc / bc.sum(0) * gap).sum(0), gap.max(0)

    cf, ok, ece, mce = reliability(bc.sum(1), bcf.sum(1), bok.sum(1))
    out = {"error_rate": float(sums[0].sum() / cnt.sum()), "log_density": float(sums[1].sum() / cnt.sum()),
           "brier": float(sums[2].sum() / cnt.sum()), "ece": float(ece), "mce": float(mce),
           "top_k_accuracy": np.cumsum(rank.sum(1)) / cnt.sum()}
    edges = np.arange(B + 1) / B
    with np.errstate(divide="ignore", invalid="ignore"):
        per_class = {"recall": np.einsum("ttd->dt", conf) / conf.sum(1).T, "precision": np.einsum("ttd->dt", conf) / conf.sum(0).T,
                     "support": conf.sum(1).T}
    if ND == 1:
        out["reliability"] = {"edges": edges, "count": np.rint(bc[:, 0]).astype(np.int64), "confidence": cf, "accuracy": ok}
        out["confusion"] = conf[..., 0]
        out["per_class"] = {k: v[0] for k, v in per_class.items()}
        return out
    cfo, oko, eceo, _ = reliability(bc, bcf, bok)
    out.update(error_rate_per_output=sums[0] / cnt, log_density_per_output=sums[1] / cnt, brier_per_output=sums[2] / cnt,
               ece_per_output=eceo, confusion=np.ascontiguousarray(conf.transpose(2, 0, 1)), per_class=per_class,
               reliability={"edges": edges, "count": np.rint(bc.T).astype(np.int64), "confidence": cfo.T, "accuracy": oko.T})
    return out


def calibration_scores(sums, probs, Y_std=1.0):
    """The dict of DGP_Base.calibration (without `n` and `rows`) from the (2 + P, D) accumulator of dsdgp_mixture_calibration."""
    cnt = sums[1]
    out = {"crps": Y_std * float(sums[0].sum() / cnt.sum()), "crps_per_output": Y_std * sums[0] / cnt, "pit_le": sums[2:] / cnt,
           "coverage": {}}
    tot = sums[2:].sum(1) / cnt.sum()
    for k, p in enumerate(probs):
        for l, r in enumerate(probs):
            if p < 0.5 and abs(r - (1.0 - p)) <= 1e-12:      # (1 - 0.025 and 0.975 differ in the last bit)
                out["coverage"][float(1.0 - 2.0 * p)] = float(tot[l] - tot[k])
    return out


class DGP_Quad(DGP_Base):
    """A DGP evaluated with Gauss-Hermite quadrature over the inner layers instead of Monte-Carlo samples (dgp.py:129-166):
    H**D_quad deterministic whitened points, D_quad = the summed inner-layer widths, injected through `zs` with shape
    (S,1,D) and combined with the quadrature weights in place of the mean over S.  Exponential in D_quad — a test oracle for
    the sampler (tests/test_dgp.py:120-174), evaluated (and differentiated) by the same device path as DGP."""

    def __init__(self, *args, H=100, **kwargs):
        DGP_Base.__init__(self, *args, **kwargs)
        from .utils import mvhermgauss
        self.H = int(H)
        self.D_quad = sum(layer.q_mu.shape[1] for layer in self.layers[:-1])        # dgp.py:142
        gh_x, gh_w = mvhermgauss(self.H, self.D_quad)
        gh_x = gh_x * 2.0 ** 0.5                                                     # dgp.py:144
        self.gh_w = gh_w * np.pi ** (-0.5 * self.D_quad)                             # dgp.py:145
        self.gh_x, s = [], 0
        for layer in self.layers[:-1]:                                               # dgp.py:149-154: (S,1,D) slices
            e = s + layer.q_mu.shape[1]
            self.gh_x.append(np.ascontiguousarray(gh_x[:, None, s:e]))
            s = e
        self.gh_x.append(np.zeros((1, 1, 1)))                                        # dgp.py:157 (never used)
        self.num_samples = self.H ** self.D_quad                                     # dgp.py:164

    def engine(self):
        eng = DGP_Base.engine(self)
        if getattr(eng, "_sample_w", None) is None:
            eng.set_sample_weights(eng.ctx.to_device(self.gh_w))
        return eng

    def E_log_p_Y(self, X, Y, zs=None):                                              # dgp.py:160-166
        Fmean, Fvar = self._build_predict(X, full_cov=False, S=self.num_samples, zs=self.gh_x)
        return self.likelihood.variational_expectations_mean(Fmean, Fvar, np.asarray(Y, dtype=np.float64), weights=self.gh_w)

    def _build_likelihood(self, X=None, Y=None, zs=None, with_grad=False, grad_from_layer=0, grad_q_only=False):
        return DGP_Base._build_likelihood(self, X, Y, zs=self.gh_x, with_grad=with_grad, grad_from_layer=grad_from_layer,
                                          grad_q_only=grad_q_only)

    def train_step(self, *args, **kwargs):
        kwargs["zs"] = self.gh_x
        return DGP_Base.train_step(self, *args, **kwargs)


class DGP(DGP_Base):
    """The doubly-stochastic DGP with linear/identity mean functions (dgp.py:169-192).  Z: the (M, D) inducing inputs, or an integer M
    for kmeans_inducing(X, M, seed=0) — the kmeans2 call of demos/run_regression.py:57, on the device.  inducing (read only when Z is
    an integer): "kmeans", or "greedy" for greedy_inducing(X, M, kernels[0]) — the conditional-variance rule under the first layer's
    kernel; ValueError if fewer than M rows pass its threshold (settings.jitter).  pca: "host" (np.linalg.svd, as the reference) or
    "device" (layer_initializations.pca_map) for the step-down mean functions of init_layers_linear."""

    def __init__(self, X, Y, Z, kernels, likelihood, num_outputs=None, mean_function=None, white=False, inducing="kmeans", pca="host",
                 **kwargs):
        if pca not in ("host", "device"):
            raise ValueError(f"pca = {pca!r}: 'host' or 'device'")
        if isinstance(Z, (int, np.integer)) and not isinstance(Z, bool):
            if inducing not in ("kmeans", "greedy"):
                raise ValueError(f"inducing = {inducing!r}: 'kmeans' or 'greedy'")
            if inducing == "greedy":
                M = int(Z)
                Z = greedy_inducing(X, M, kernels[0])
                if Z.shape[0] < M:
                    raise ValueError(f"inducing='greedy': only {Z.shape[0]} of the M = {M} rows asked for have a conditional variance "
                                     "above the threshold (settings.jitter); ask for fewer")
            else:
                Z = kmeans_inducing(X, int(Z), seed=0)
        layers = init_layers_linear(X, Y, Z, kernels, num_outputs=num_outputs,
                                    mean_function=Zero() if mean_function is None else mean_function, white=white, pca=pca)
        DGP_Base.__init__(self, X, Y, likelihood, layers, **kwargs)
