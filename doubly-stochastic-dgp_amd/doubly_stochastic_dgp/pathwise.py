"""Pathwise (Matheron) draws of a trained deep GP's FUNCTIONS (Wilson, Borovitskiy, Terenin, Mostowsky and Deisenroth, "Efficiently
sampling functions from Gaussian process posteriors", ICML 2020) on the device: dsdgp_pathwise_weights once per layer at draw time,
dsdgp_pathwise_eval per layer and row batch afterwards (csrc/pathwise.hip).  The reference has no counterpart: it draws rows independently
(layers.py:76-119) or jointly through an n x n factor per sample and output (utils.py:43-51).

A layer's draw is  f(x)_o = f0(x)_o + sum_m k(x, z_m) v_mo + m(x)_o  with
  f0(x)_o = sqrt(s2 / L) sum_j [a_jo cos theta_j(x) + b_jo sin theta_j(x)],  theta_j(x) = sum_d (x_d - c_d) Omega_dj,
  v = Ku^-1 (u - f0(Z)),  Ku = K(Z, Z) + (White variance + jitter) I,  u_o = q_mu_o + q_sqrt_o eps_o (white: Lu times that),
and a stack's draw is the composition: layer l + 1 is evaluated at layer l's output, rows r = s n + i as DGP_Base.propagate has them.

The basis.  Omega (D x L) and the origin c = Z[0] are drawn ONCE per layer and shared by the layer's outputs and by all S draws; the draws
are independent GIVEN the basis (their weights a, b and eps are), not marginally.  One generator np.random.default_rng(seed) serves the
layers in order; layer l takes from it g = standard_normal((D, L)) and then, for Matern52 only, c = chisquare(5, L): omega_j = g_j for
the RBF kernel, g_j sqrt(5 / c_j) for Matern52 (the multivariate Student-t with 5 degrees of freedom, one c_j per frequency), and row d
is divided by the lengthscale l_d.

The normal draws are dsdgp_randn(seed, stream, count) in these streams and layouts, which are part of the interface (oracle/philox.py:
randn_reference replays them on the CPU):  stream 3l: a = Wc (S, L, DO);  stream 3l + 1: b = Ws (S, L, DO);  stream 3l + 2: eps (S, M, DO).

The White part of a kernel enters Ku only: a draw is of the function WITHOUT its white component.
"""
import ctypes as C

import numpy as np

from . import _lib, settings
from .gpflow_compat import split_kernel

_MEANS = ("zero", "identity", "linear")


def sample_basis(kind, D, L, lengthscales, rng):
    """Omega (D, L) of the random Fourier basis of an RBF ('rbf') or Matern52 ('matern52') kernel, divided by the lengthscales (one value
    or D of them) row by row, from the numpy generator rng: see the module's docstring for the order of the draws"""
    g = rng.standard_normal((int(D), int(L)))
    if kind == "matern52":
        g = g * np.sqrt(5.0 / rng.chisquare(5, size=int(L)))[None, :]
    elif kind != "rbf":
        raise NotImplementedError(f"sample_basis: the spectral density of the kernel kind {kind!r} is not known here")
    ls = np.broadcast_to(np.asarray(lengthscales, dtype=np.float64).reshape(-1), (int(D),))
    return np.ascontiguousarray(g / ls[:, None])


def _refuse(model):
    """NotImplementedError, before any device is touched, for everything sample_functions does not cover"""
    from .layers import SVGP_Layer
    from .model_zoo import DGP_Collapsed, DGP_SGPMC
    if isinstance(model, (DGP_Collapsed, DGP_SGPMC)):
        raise NotImplementedError(f"sample_functions: pathwise draws are built for DGP and DGP_Quad over SVGP_Layers, not for "
                                  f"{type(model).__name__}")
    for l, layer in enumerate(model.layers):
        if type(layer) is not SVGP_Layer:
            raise NotImplementedError(f"sample_functions: layer {l} is a {type(layer).__name__}; pathwise draws are built for "
                                      "SVGP_Layer only")
        if layer.input_prop_dim:
            raise NotImplementedError(f"sample_functions: layer {l} propagates {layer.input_prop_dim} input dimensions "
                                      "(input_prop_dim), which the pathwise draws do not carry")
        split_kernel(layer.kern)                       # NotImplementedError for anything but <RBF | Matern52> [+ White]
        if getattr(layer.mean_function, "kind", None) not in _MEANS:
            raise NotImplementedError(f"sample_functions: layer {l} has a {type(layer.mean_function).__name__} mean function; Zero, "
                                      "Identity and Linear are covered")


class _LayerDraw:
    """what one layer of a draw holds: the snapshot of the layer and its part of the S functions, on the device"""


class PathwiseFunctions:
    """S consistent function draws of a deep GP, a snapshot of the model at the time of the draw: later training does not change them.
    fs(Xs) evaluates the S functions of the last layer at Xs, (S, N, D_out); fs.all_layers(Xs) every layer's; any inputs, any number of
    calls, the same functions.  Built by DGP_Base.sample_functions."""

    def __init__(self, model, num_functions=1, num_features=1024, seed=0):
        _refuse(model)
        S, L = int(num_functions), int(num_features)
        if S < 1 or L < 1:
            raise ValueError("sample_functions: num_functions and num_features must be at least 1")
        from .engine import Context
        from .layers import _kernel_spec
        ctx = Context.get()
        self.ctx, self.num_functions, self.num_features, self.seed = ctx, S, L, int(seed)
        self.input_dim = int(split_kernel(model.layers[0].kern)[0].input_dim)
        self.layers = []
        rng = np.random.default_rng(self.seed)
        jitter = float(settings.jitter)
        with ctx.torch.cuda.stream(ctx.tstream):      # torch's allocations and copies on the library's stream, whatever stream is current
            for l, layer in enumerate(model.layers):
                d = _LayerDraw()
                stat = split_kernel(layer.kern)[0]
                d.spec, d.ls = _kernel_spec(layer.kern)
                d.kind, d.D, d.DO, d.L = stat.kind, int(stat.input_dim), int(layer.num_outputs), L
                Z = np.array(layer.feature.Z.value, dtype=np.float64)
                d.M = Z.shape[0]
                d.Z_host, d.origin_host = Z, Z[0].copy()
                d.variance = float(stat.variance.value)
                d.ls_host = np.array(stat.lengthscales.value, dtype=np.float64).reshape(-1)
                d.Omega_host = sample_basis(d.kind, d.D, L, d.ls_host, rng)
                d.Z, d.Omega, d.origin = ctx.to_device(Z), ctx.to_device(d.Omega_host), ctx.to_device(d.origin_host)
                d.mean = layer.mean_function.kind
                if d.mean == "identity" and d.D != d.DO:
                    raise ValueError(f"sample_functions: layer {l} has an Identity mean function between {d.D} and {d.DO} dimensions")
                if d.mean == "linear":                       # read at draw time, trainable or not
                    d.A = ctx.to_device(np.array(layer.mean_function.A.value, dtype=np.float64).reshape(d.D, d.DO))
                    d.b = ctx.to_device(np.array(layer.mean_function.b.value, dtype=np.float64).reshape(1, d.DO))
                d.Wc, d.Ws, eps = (self._randn(3 * l + k, S * (L if k < 2 else d.M) * d.DO) for k in range(3))
                q_mu = ctx.to_device(np.array(layer.q_mu.value, dtype=np.float64))
                q_sqrt = ctx.to_device(np.tril(np.array(layer.q_sqrt.value, dtype=np.float64)))
                d.V = ctx.empty(S * d.M * d.DO)
                need = C.c_int64()
                _lib.check(ctx.lib.dsdgp_pathwise_scratch_bytes(d.M, d.D, d.DO, S, C.byref(need)))
                scratch = ctx.empty(need.value // 8 + 32)
                # CholeskyError where Ku is not positive definite
                _lib.check(ctx.lib.dsdgp_pathwise_weights(ctx.handle, C.byref(d.spec), _p(d.Z), d.M, _p(d.Omega), _p(d.origin), L, _p(d.Wc),
                                                          _p(d.Ws), S, _p(q_mu), _p(q_sqrt), _p(eps), d.DO, int(bool(layer.white)), jitter,
                                                          _p(scratch), need.value, _p(d.V), C.byref(C.c_int(0))))
                d.basis_error = None
                self.layers.append(d)
        ctx.sync()                                       # the uploads and the scratch blocks may go

    def _randn(self, stream, count):
        out = self.ctx.empty(count)
        _lib.check(self.ctx.lib.dsdgp_randn(self.ctx.handle, C.c_uint64(self.seed), C.c_uint64(stream), count, _p(out)))
        return out

    def _layer(self, d, Xin, nb, per_draw):
        """layer d at Xin — (nb, D) for every draw, or (S nb, D) with per_draw — as a tensor (S nb, DO)"""
        ctx, S = self.ctx, self.num_functions
        x_stride = nb * d.D if per_draw else 0
        add, ld_add, add_stride = None, 0, 0
        if d.mean == "identity":
            add, ld_add, add_stride = Xin, d.D, x_stride
        elif d.mean == "linear":
            add = ctx.empty(Xin.shape[0], d.DO)
            add[:] = d.b
            ctx.gemm(0, 0, 1.0, Xin, d.A, 1.0, add)
            ld_add, add_stride = d.DO, nb * d.DO if per_draw else 0
        out = ctx.empty(S * nb, d.DO)
        _lib.check(ctx.lib.dsdgp_pathwise_eval(ctx.handle, C.byref(d.spec), _p(Xin), nb, x_stride, S, _p(d.Omega), _p(d.origin), d.L,
                                               _p(d.Wc), _p(d.Ws), _p(d.Z), d.M, _p(d.V), d.DO, _p(add), ld_add, add_stride, _p(out), d.DO))
        return out

    def all_layers(self, Xs, batch_size=8192, on_device=False):
        """every layer's S functions at Xs (N, D): a list of (S, N, D_l), layer l + 1 evaluated at layer l's values.  Xs: a numpy array or
        a device tensor; the rows go through all layers in batches of batch_size, and the result has the same bits for every batch_size
        and for any split of Xs into calls.  on_device: device tensors, without waiting for them."""
        ctx, S = self.ctx, self.num_functions
        with ctx.torch.cuda.stream(ctx.tstream):
            X = ctx.as_device(Xs)
            if X.dim() != 2 or X.shape[1] != self.input_dim or X.shape[0] < 1:
                raise ValueError(f"PathwiseFunctions: Xs must be (N, {self.input_dim}) with N >= 1, not {tuple(X.shape)}")
            N, step = X.shape[0], max(1, int(batch_size))
            outs = [ctx.empty(S, N, d.DO) for d in self.layers]
            for i0 in range(0, N, step):
                nb = min(step, N - i0)
                F = X[i0:i0 + nb]
                for l, d in enumerate(self.layers):
                    F = self._layer(d, F, nb, per_draw=l > 0)
                    outs[l][:, i0:i0 + nb, :] = F.view(S, nb, d.DO)
        if on_device:
            return outs
        ctx.sync()
        return [t.cpu().numpy() for t in outs]

    def __call__(self, Xs, batch_size=8192, on_device=False):
        """the S functions of the last layer at Xs: (S, N, D_out); see all_layers"""
        return self.all_layers(Xs, batch_size=batch_size, on_device=on_device)[-1]

    def basis_error(self, l):
        """max |K^(Z, Z) - K(Z, Z)| of layer l, K^ the basis kernel s2 / L sum_j cos(theta_j(z) - theta_j(z')): is num_features large
        enough?  The update multiplies this error by the norm of Ku^-1, so inducing inputs that nearly coincide need more features.
        Computed on the host at the first call."""
        d = self.layers[l]
        if d.basis_error is None:
            th = (d.Z_host - d.origin_host[None, :]) @ d.Omega_host
            c, s = np.cos(th), np.sin(th)
            Khat = d.variance / d.L * (c @ c.T + s @ s.T)
            ls = np.broadcast_to(d.ls_host, (d.D,))
            diff = (d.Z_host[:, None, :] - d.Z_host[None, :, :]) / ls
            r2 = np.sum(diff * diff, axis=-1)
            if d.kind == "rbf":
                K = d.variance * np.exp(-0.5 * r2)
            else:
                r = np.sqrt(r2 + 1e-12)
                K = d.variance * (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r * r) * np.exp(-np.sqrt(5.0) * r)
            d.basis_error = float(np.max(np.abs(Khat - K)))
        return d.basis_error


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())
