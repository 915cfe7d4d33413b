"""Device engine: owns the flat unconstrained parameter vector theta, the workspace and the libdsdgp model handle for a
list of SVGP layers + likelihood, and keeps host `Parameter` objects coherent with it.

torch is used ONLY as the device allocator / stream provider (and, in distributed.py, for the RCCL process group);
no torch op runs on the hot path.
"""
import ctypes as C

import numpy as np

from . import _lib, settings
from .gpflow_compat import MultiClass, Parameter, likelihood_entry, positive_backward, positive_forward, split_kernel

_KIND = {"rbf": _lib.KERN_RBF, "matern52": _lib.KERN_MATERN52}
_MEAN = {"zero": _lib.MEAN_ZERO, "identity": _lib.MEAN_IDENTITY, "linear": _lib.MEAN_LINEAR}


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise _lib.DsdgpError("no MI355X visible (torch.cuda.is_available() is False): the DGP compute path has no CPU "
                              "fallback")
    return torch


class Context:
    """One libdsdgp context per process, bound to torch's current HIP stream on cuda:<device>."""
    _inst = None

    def __init__(self, device=None):
        torch = _torch()
        self.lib = _lib.load()
        self.device = torch.cuda.current_device() if device is None else device
        self.torch = torch
        # ONE stream for everything: torch's default stream has handle 0, which the C-ABI reads as "create a private
        # stream", and a private stream is not ordered with torch's copies nor with the RCCL all-reduce.  So create a
        # dedicated stream, make it torch's current stream for this process, and give its handle to libdsdgp: kernels,
        # H2D/D2H copies and collectives are then ordered by the stream itself.
        self.tstream = torch.cuda.Stream(device=self.device)
        torch.cuda.set_stream(self.tstream)
        h = C.c_void_p()
        _lib.check(self.lib.dsdgp_ctx_create(C.byref(h), self.device, C.c_void_p(self.tstream.cuda_stream)))
        self.handle = h

    @classmethod
    def get(cls):
        if cls._inst is None:
            cls._inst = Context()
        return cls._inst

    def sync(self):
        _lib.check(self.lib.dsdgp_sync(self.handle))

    def empty(self, *shape):
        return self.torch.empty(*shape, dtype=self.torch.float64, device=f"cuda:{self.device}")

    def to_device(self, arr):
        a = np.array(arr, dtype=np.float64, order="C", copy=True) if not getattr(arr, "flags", None) or not arr.flags.writeable \
            else np.ascontiguousarray(arr, dtype=np.float64)
        return self.torch.as_tensor(a).to(f"cuda:{self.device}")

    def as_device(self, a):
        """a as a contiguous float64 tensor on the device: a tensor is converted only where it has to be, anything else is uploaded"""
        return a.to(device=f"cuda:{self.device}", dtype=self.torch.float64).contiguous() if hasattr(a, "data_ptr") else self.to_device(a)

    # The dense primitives the collapsed layer composes, on tensors: every m, n, k comes from a .shape, every leading dimension from a
    # .stride(0), and an operand of the wrong dtype, device, layout or shape is a ValueError before the call, not an access out of bounds
    def _p(self, what, t, shape, packed=False):
        """(pointer, leading dimension) of the float64 tensor t on this device.  shape: what t's must be (None: any); its rows have unit
        stride; packed: no padding between them either (the library takes no leading dimension for this operand)"""
        ok = hasattr(t, "data_ptr") and t.dtype == self.torch.float64 and t.is_cuda and t.device.index == self.device
        ok = ok and t.dim() == len(shape) and t.numel() > 0 and all(w is None or w == h for w, h in zip(shape, t.shape))
        ok = ok and (t.is_contiguous() if packed or t.dim() == 1 else (t.stride(1) == 1 or t.shape[1] == 1) and t.stride(0) >= t.shape[1])
        if not ok:
            raise ValueError(f"{what}: expected a float64 tensor of shape {shape} on cuda:{self.device}, rows of unit stride"
                             f"{' and packed' if packed else ''}; got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        return C.c_void_p(t.data_ptr()), t.stride(0)

    def gram(self, spec, X, X2, jitter, out):                # out = K(X, X2); X2 None: K(X, X) + jitter I
        m, n2, D = X.shape[0], 0 if X2 is None else X2.shape[0], spec.input_dim
        x2 = None if X2 is None else self._p("gram: X2", X2, (n2, D), True)[0]
        _lib.check(self.lib.dsdgp_gram(self.handle, C.byref(spec), self._p("gram: X", X, (m, D), True)[0], m, x2, n2, jitter,
                                       *self._p("gram: out", out, (m, n2 or m))))

    def potrf(self, A):                                      # A <- its lower Cholesky factor; CholeskyError if A is not positive definite
        (a, lda), n = self._p("potrf: A", A, (A.shape[0], A.shape[0])), A.shape[0]
        _lib.check(self.lib.dsdgp_potrf(self.handle, 1, n, a, lda, lda * n, C.byref(C.c_int(0))))

    def trsm(self, L, B, trans=0):                           # B <- L^-1 B, with trans L^-T B; L lower triangular
        m, n = B.shape
        _lib.check(self.lib.dsdgp_trsm(self.handle, trans, m, n, *self._p("trsm: L", L, (m, m)), *self._p("trsm: B", B, (m, n))))

    def gemm(self, ta, tb, alpha, A, B, beta, out):          # out <- alpha op(A) op(B) + beta out, op the transpose with ta / tb
        (m, n), k = out.shape, A.shape[0 if ta else 1]
        _lib.check(self.lib.dsdgp_gemm(self.handle, ta, tb, m, n, k, alpha, *self._p("gemm: A", A, (k, m) if ta else (m, k)),
                                       *self._p("gemm: B", B, (n, k) if tb else (k, n)), beta, *self._p("gemm: out", out, (m, n))))

    def scale_copy(self, A, B, trans=0, div=1.0, diag_add=0.0):      # B <- op(A) / div + diag_add I
        m, n = B.shape
        _lib.check(self.lib.dsdgp_scale_copy(self.handle, trans, m, n, *self._p("scale_copy: A", A, (n, m) if trans else (m, n)), div,
                                             diag_add, *self._p("scale_copy: B", B, (m, n))))

    def collapsed_bound(self, LB, G, c, Y, psi0, s2, out):   # out (7): the bound and its six terms
        M, (n, DY), p = LB.shape[0], Y.shape, lambda k, t, shape: self._p("collapsed_bound: " + k, t, shape, True)[0]
        _lib.check(self.lib.dsdgp_collapsed_bound(self.handle, M, n, DY, *self._p("collapsed_bound: LB", LB, (M, M)),
                                                  *self._p("collapsed_bound: G", G, (M, M)), p("c", c, (M, DY)), p("Y", Y, (n, DY)),
                                                  p("psi0", psi0, (1,)), s2, p("out", out, (7,))))

    def collapsed_var(self, tmp1, tmp2, kdiag, var):         # var (ns, DY) from tmp1 = L^-1 K(Z, X*) and tmp2 = LB^-1 tmp1, both (M, ns)
        (M, ns), DY = tmp1.shape, var.shape[1]
        _lib.check(self.lib.dsdgp_collapsed_var(self.handle, M, ns, DY, *self._p("collapsed_var: tmp1", tmp1, (M, ns)),
                                                *self._p("collapsed_var: tmp2", tmp2, (M, ns)), kdiag,
                                                self._p("collapsed_var: var", var, (ns, DY), True)[0]))

    def collapsed_adjoints(self, Si, Ki, KpK, psi2, alpha, c, Y, psi0, s2, g_psi2, d_Kuu, out):      # g_psi2, d_Kuu (M, M), out (8)
        M, (n, DY), p = Si.shape[0], Y.shape, lambda k, t, shape: self._p("collapsed_adjoints: " + k, t, shape, True)[0]
        MM, MD = (M, M), (M, DY)
        _lib.check(self.lib.dsdgp_collapsed_adjoints(self.handle, M, n, DY, p("Si", Si, MM), p("Ki", Ki, MM), p("KpK", KpK, MM),
                                                     p("psi2", psi2, MM), p("alpha", alpha, MD), p("c", c, MD), p("Y", Y, (n, DY)),
                                                     p("psi0", psi0, (1,)), s2, p("g_psi2", g_psi2, MM), p("d_Kuu", d_Kuu, MM),
                                                     p("out", out, (8,))))

    def gram_grad(self, spec, X, X2, G, d_X=None, d_X2=None, d_kern=None):
        """the reverse pass of gram: G (n, n2) the adjoint of K(X, X2), or (n, n) of K(X, X) + diag with X2 None; each output may be None.
        d_kern (2 + lengthscale entries): variance, lengthscales, the diagonal add"""
        n, n2, D = X.shape[0], 0 if X2 is None else X2.shape[0], spec.input_dim
        x2 = None if X2 is None else self._p("gram_grad: X2", X2, (n2, D), True)[0]
        opt = lambda k, t, shape: None if t is None else self._p("gram_grad: " + k, t, shape, True)[0]
        nk = 2 + (D if spec.ard else 1)
        _lib.check(self.lib.dsdgp_gram_grad(self.handle, C.byref(spec), self._p("gram_grad: X", X, (n, D), True)[0], n, x2, n2,
                                            *self._p("gram_grad: G", G, (n, n2 or n)), opt("d_X", d_X, (n, D)),
                                            opt("d_X2", d_X2, (n2, D)), opt("d_kern", d_kern, (nk,))))

    def gpr_bound(self, L, V, out):                          # out (4): the bound and its three terms, from L = chol(K + s2 I), V = L^-1 (Y - m)
        n, DY = V.shape
        _lib.check(self.lib.dsdgp_gpr_bound(self.handle, n, DY, *self._p("gpr_bound: L", L, (n, n)), *self._p("gpr_bound: V", V, (n, DY)),
                                            self._p("gpr_bound: out", out, (4,), True)[0]))

    def gpr_var(self, A, kdiag, var):                        # var (ns, DY) = kdiag - colsum(A^2), A = L^-1 K(F, X*) (n, ns)
        (n, ns), DY = A.shape, var.shape[1]
        _lib.check(self.lib.dsdgp_gpr_var(self.handle, n, ns, DY, *self._p("gpr_var: A", A, (n, ns)), kdiag,
                                          self._p("gpr_var: var", var, (ns, DY), True)[0]))

    def _sparse_scratch(self, n, M, D, DO, reverse):
        """the block the sparse conditional keeps its intermediates in (the calls it composes use the context's own scratch)"""
        need = C.c_int64()
        _lib.check(self.lib.dsdgp_sparse_conditional_scratch_bytes(n, M, D, DO, int(reverse), C.byref(need)))
        return self.torch.empty(need.value // 8 + 32, dtype=self.torch.float64, device=f"cuda:{self.device}"), need.value

    def sparse_conditional(self, spec, Z, X, q_mu, white, jitter, mean=None, var=None):
        """the sparse conditional without q_sqrt (dsdgp_sparse_conditional): mean (n, DO) = A^T W, var (n,) = kdiag - colsum(A^2), A =
        Lu^-1 K(Z, X), W = q_mu (white) or Lu^-1 q_mu; each output may be None.  CholeskyError if K(Z, Z) + jitter I is not positive
        definite: nothing is written then."""
        (M, D), n, DO = Z.shape, X.shape[0], q_mu.shape[1]
        p = lambda k, t, shape: None if t is None else self._p("sparse_conditional: " + k, t, shape, True)[0]
        scr, nbytes = self._sparse_scratch(n, M, D, DO, False)
        _lib.check(self.lib.dsdgp_sparse_conditional(self.handle, C.byref(spec), p("Z", Z, (M, spec.input_dim)), M, p("X", X, (n, D)), n,
                                                     p("q_mu", q_mu, (M, DO)), DO, int(bool(white)), float(jitter), ptr(scr), nbytes,
                                                     p("mean", mean, (n, DO)), p("var", var, (n,)), C.byref(C.c_int(0))))

    def sparse_conditional_grad(self, spec, Z, X, q_mu, white, jitter, gm, gv, d_q_mu=None, d_Z=None, d_X=None, d_kern=None):
        """the reverse pass of sparse_conditional (dsdgp_sparse_conditional_grad): gm (n, DO) the adjoint of the mean, gv (n,) the adjoint
        of the variance summed over the outputs; each output may be None.  d_kern (2 + lengthscale entries): variance, lengthscales,
        the diagonal add (the White variance)"""
        (M, D), n, DO = Z.shape, X.shape[0], q_mu.shape[1]
        p = lambda k, t, shape: None if t is None else self._p("sparse_conditional_grad: " + k, t, shape, True)[0]
        nk = 2 + (D if spec.ard else 1)
        scr, nbytes = self._sparse_scratch(n, M, D, DO, True)
        _lib.check(self.lib.dsdgp_sparse_conditional_grad(
            self.handle, C.byref(spec), p("Z", Z, (M, spec.input_dim)), M, p("X", X, (n, D)), n, p("q_mu", q_mu, (M, DO)), DO,
            int(bool(white)), float(jitter), p("gm", gm, (n, DO)), p("gv", gv, (n,)), ptr(scr), nbytes, p("d_q_mu", d_q_mu, (M, DO)),
            p("d_Z", d_Z, (M, D)), p("d_X", d_X, (n, D)), p("d_kern", d_kern, (nk,)), C.byref(C.c_int(0))))

    def prof_enable(self, on=True):
        _lib.check(self.lib.dsdgp_prof_enable(self.handle, int(on)))

    def prof_read(self, name, reset=True):
        ms, cnt = C.c_double(), C.c_int64()
        _lib.check(self.lib.dsdgp_prof_read(self.handle, name.encode(), C.byref(ms), C.byref(cnt), int(reset)))
        return ms.value, cnt.value


def padded_M(M):
    """pad_M of csrc/common.hpp: the order of every device-side M x M operand"""
    if M <= 32:
        return 32
    q = 16 if M <= 128 else 32 if M <= 256 else 64 if M <= 512 else 128
    return -(-M // q) * q


def ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


class Engine:
    def __init__(self, layers, likelihood, white, n_max=1024, s_max=1):
        for layer in layers:
            if hasattr(layer, "q_sqrt") and layer.q_sqrt is None:
                raise NotImplementedError(f"Engine: {type(layer).__name__} has no q_sqrt, and the engine's KL tail reads one from every "
                                          "layer record (the logarithm of its diagonal); an SGPMC_Layer runs under a collapsed layer in "
                                          "a DGP_Collapsed, outside the engine")
        self.ctx = Context.get()
        self.lib = self.ctx.lib
        self.layers, self.likelihood, self.white = list(layers), likelihood, bool(white)
        self.jitter = float(settings.jitter)
        self.model = None
        self.n_max, self.s_max = 0, 0
        self._host_dirty = True        # host Parameter values newer than device theta
        self._dev_dirty = False        # device theta newer than host Parameter values
        self._structure_dirty = False
        self._needs_prepare = True
        self._sample_w = None
        self._build_layout()
        self._ensure(n_max, s_max)

    # ------------------------------------------------------------------ parameter layout
    def _params_of(self, layer):
        stat, white = split_kernel(layer.kern)
        return stat, white

    def _build_layout(self):
        off = 0
        self.entries = []      # (Parameter, offset, count, kind) ; kind in {'id','pos','qsqrt'}
        self.desc = _lib.ModelDesc()
        d = self.desc
        d.L = len(self.layers)
        if d.L > _lib.DSDGP_MAX_LAYERS:
            raise ValueError("too many layers")
        d.white = int(self.white)
        d.jitter = self.jitter
        self._mean_A = []
        for l, layer in enumerate(self.layers):
            stat, wk = self._params_of(layer)
            ld = d.layers[l]
            M, Din = layer.feature.Z.shape
            Dout = layer.num_outputs
            ld.M, ld.D_in, ld.D_out = M, Din, Dout
            ld.kern_kind = _KIND[stat.kind]
            ld.ard = int(stat.ARD)
            ld.has_white = int(wk is not None)
            ld.mean_kind = _MEAN[layer.mean_function.kind]
            ld.off_mean_A = ld.off_mean_b = -1
            mf_in_theta = False
            if layer.mean_function.kind == "linear":
                A = np.asarray(layer.mean_function.A._value, dtype=np.float64)
                if A.shape != (Din, Dout):
                    raise ValueError("Linear mean function has the wrong shape")
                mf_in_theta = layer.mean_function.in_theta()
                if not mf_in_theta:                       # fixed map, no bias: a constant device array
                    tA = self.ctx.to_device(A)
                    self._mean_A.append((layer.mean_function, tA))
                    ld.mean_A = tA.data_ptr()
                    # still owned: a later `mean_function.A = W`, a non-zero b or set_trainable(True) must reach the device
                    for p in (layer.mean_function.A, layer.mean_function.b):
                        if self not in p._owners:
                            p._owners.append(self)

            def add(p, kind, name):
                nonlocal off
                cnt = int(np.prod(p.shape)) if p.shape else 1
                self.entries.append((p, off, cnt, kind))
                setattr(ld, "off_" + name, off)
                if self not in p._owners:
                    p._owners.append(self)
                off += cnt
                return p.trainable

            ld.input_prop_dim = int(getattr(layer, "input_prop_dim", None) or 0)
            if ld.input_prop_dim and l == len(self.layers) - 1 and len(self.layers) > 1:
                raise NotImplementedError("the last layer of a DGP does not propagate inputs "
                                          "(layer_initializations.py:75-78)")
            ld.trainable_Z = int(add(layer.feature.Z, "id", "Z"))
            ld.trainable_q_mu = int(add(layer.q_mu, "id", "q_mu"))
            ld.trainable_q_sqrt = int(add(layer.q_sqrt, "qsqrt", "q_sqrt"))
            # a variance Parameter WITHOUT the positive transform (tests/test_dgp.py:79-85: NoTransformMatern52, variance 1e-24) is
            # its own free variable on the device too
            ld.kvar_identity = int(getattr(stat.variance, "transform", "positive") is None)
            ld.trainable_kvar = int(add(stat.variance, "id" if ld.kvar_identity else "pos", "kvar"))
            ld.trainable_kls = int(add(stat.lengthscales, "pos", "kls"))
            if wk is not None:
                ld.trainable_wvar = int(add(wk.variance, "pos", "wvar"))
            if mf_in_theta:
                ld.trainable_mean_A = int(add(layer.mean_function.A, "id", "mean_A"))
                ld.trainable_mean_b = int(add(layer.mean_function.b, "id", "mean_b"))
        d.lik_kind, p, const = likelihood_entry(self.likelihood)
        if d.lik_kind == _lib.LIK_MULTICLASS:
            d.num_classes = const
        elif const is not None:
            d.lik_aux = const
        d.off_lik_var = -1
        if p is not None:      # the likelihood's one positive parameter (Gaussian.variance, StudentT.scale, Gamma.shape, Beta.scale)
            self.entries.append((p, off, 1, "pos"))
            if self not in p._owners:
                p._owners.append(self)
            d.off_lik_var = off
            d.trainable_lik_var = int(p.trainable)
            off += 1
        d.n_theta = off
        self.n_theta = off

    def _pack_host(self):
        th = np.zeros(self.n_theta)
        for p, off, cnt, kind in self.entries:
            v = np.asarray(p._value, dtype=np.float64)
            if kind == "pos":
                v = positive_backward(v)
            elif kind == "qsqrt":
                v = np.tril(v)
            th[off:off + cnt] = np.ravel(v)
        return th

    def _unpack_host(self, th):
        for p, off, cnt, kind in self.entries:
            v = th[off:off + cnt].reshape(p.shape)
            if kind == "pos":
                v = positive_forward(v)
            p._value = np.array(v, dtype=np.float64)

    # ------------------------------------------------------------------ coherence
    def mark_host_dirty(self):
        self._host_dirty = True

    def mark_structure_dirty(self):
        self._structure_dirty = True

    def sync_to_host(self):
        if self._dev_dirty and self.model is not None:
            self.ctx.sync()
            self._unpack_host(self.theta.cpu().numpy())
            self._dev_dirty = False

    def _upload_if_needed(self):
        if self._host_dirty and any(mf.in_theta() for mf, _ in self._mean_A):
            self._structure_dirty = True       # a fixed Linear map gained a bias / became trainable: it moves into theta
        if settings.jitter != self.jitter or self._structure_dirty:
            self.sync_to_host()
            self.jitter = float(settings.jitter)
            self._structure_dirty = False
            for p, *_ in self.entries:
                if self in p._owners:
                    p._owners.remove(self)
            for mf, _ in self._mean_A:
                for p in (mf.A, mf.b):
                    if self in p._owners:
                        p._owners.remove(self)
            self._build_layout()
            n, s = self.n_max, self.s_max
            self._destroy()
            self._host_dirty = True
            self._ensure(n, s)
        if self._host_dirty:
            for mf, tA in self._mean_A:            # fixed maps: refresh the constant device copy in place (same pointer)
                tA.copy_(self.ctx.torch.as_tensor(np.ascontiguousarray(mf.A._value, dtype=np.float64)))
            th = self._pack_host()
            self.theta.copy_(self.ctx.torch.as_tensor(th))
            _lib.check(self.lib.dsdgp_model_theta_changed(self.model))     # our side of dsdgp_model_track_theta
            self._host_dirty = False
            self._dev_dirty = False
            self._needs_prepare = True

    def _prepare_checked(self):
        """build_cholesky_if_needed (layers.py:167-175) once per parameter change, surfacing tf.cholesky failures."""
        self._upload_if_needed()
        if self._needs_prepare:
            info = C.c_int(0)
            _lib.check(self.lib.dsdgp_model_prepare(self.model, C.byref(info)))
            self._needs_prepare = False

    # ------------------------------------------------------------------ model lifetime
    def _destroy(self):
        if self.model is not None:
            _lib.check(self.lib.dsdgp_model_destroy(self.model))
            self.model = None
        self.n_max = self.s_max = 0

    def _ensure(self, n, s):
        """(Re)create the device model for up to n rows x s samples.  Only the workspace depends on (n, s): theta, the
        gradient buffer and the Adam moments / step count are allocated once per parameter layout and SURVIVE a re-creation
        (a predict_* call with more rows or samples than the training shape must not reset the optimiser — TF keeps its
        Adam slots across predictions)."""
        if self.model is not None and n <= self.n_max and s <= self.s_max:
            return
        n_max, s_max = max(n, self.n_max), max(s, self.s_max)
        self._destroy()
        torch = self.ctx.torch
        nbytes = C.c_int64()
        _lib.check(self.lib.dsdgp_model_workspace_bytes(C.byref(self.desc), n_max, s_max, C.byref(nbytes)))
        dev = f"cuda:{self.ctx.device}"
        self.workspace = None                      # release the old workspace before allocating the larger one
        self.workspace = torch.empty(nbytes.value + 256, dtype=torch.uint8, device=dev)
        base = self.workspace.data_ptr()
        self._ws_ptr = (base + 255) // 256 * 256
        fresh = getattr(self, "theta", None) is None or self.theta.numel() != self.n_theta
        if fresh:
            self.theta = torch.zeros(self.n_theta, dtype=torch.float64, device=dev)
            # gradient and the 4 result scalars share one buffer so that data-parallel runs need ONE all-reduce per step
            self.gradbuf = torch.zeros(self.n_theta + 4, dtype=torch.float64, device=dev)
            self.grad = self.gradbuf[:self.n_theta]
            self.adam_m = torch.zeros(self.n_theta, dtype=torch.float64, device=dev)
            self.adam_v = torch.zeros(self.n_theta, dtype=torch.float64, device=dev)
            self.out4 = self.gradbuf[self.n_theta:]
            self.adam_t = 0
            self._host_dirty = True
        h = C.c_void_p()
        _lib.check(self.lib.dsdgp_model_create(self.ctx.handle, C.byref(self.desc), n_max, s_max, ptr(self.theta),
                                               ptr(self.grad), ptr(self.adam_m), ptr(self.adam_v),
                                               C.c_void_p(self._ws_ptr), nbytes.value, C.byref(h)))
        self.model = h
        self.generation = getattr(self, "generation", 0) + 1     # identifies THIS device model (a freed handle's address can come back)
        self._grad_first = 0
        self._grad_q_only = False
        # this engine is the only writer of theta besides the library's own optimiser steps and reports its uploads
        # (_upload_if_needed): an evaluation after a natural-gradient step alone keeps the factorisation of Ku
        _lib.check(self.lib.dsdgp_model_track_theta(self.model, 1))
        self.n_max, self.s_max = n_max, s_max
        if getattr(self, "_sample_w", None) is not None:       # DGP_Quad weights survive a model re-creation
            self.set_sample_weights(self._sample_w)
        for fn in getattr(self, "_post_create", ()):            # per-model settings owned by others (the data-parallel bucket callback)
            fn(self)
        self._needs_prepare = True

    # ------------------------------------------------------------------ compute
    def _zs_args(self, zs, S, n):
        """zs: list (per layer) of None or arrays broadcastable to (S, n, D_out) -> (ptr array, stride array, keepalive)"""
        L = len(self.layers)
        if zs is None:
            return None, None, []
        ptrs = (C.c_void_p * L)()
        strides = (C.c_int64 * (3 * L))()
        keep = []
        for l, z in enumerate(zs):
            if z is None:
                ptrs[l] = None
                continue
            D = self.layers[l].num_outputs
            if hasattr(z, "data_ptr"):
                t = z
                shape = tuple(t.shape)
            else:
                z = np.asarray(z, dtype=np.float64)
                if z.ndim != 3:
                    raise ValueError("z must be rank-3, broadcastable to (S, N, D_out)")
                shape = z.shape
                t = self.ctx.to_device(z)
            for want, got in zip((S, n, D), shape):
                if got not in (1, want):
                    raise ValueError(f"z of shape {shape} does not broadcast to {(S, n, D)}")
            keep.append(t)
            ptrs[l] = t.data_ptr()
            st = (shape[1] * shape[2], shape[2], 1)
            for k in range(3):
                strides[3 * l + k] = 0 if shape[k] == 1 else st[k]
        return ptrs, strides, keep

    def prepare(self):
        self._prepare_checked()

    def propagate(self, X, S, zs=None, seed=0, want=("F", "mean", "var")):
        """X: numpy (n, D) or device tensor. Returns lists of device tensors (S, n, D_out_l)."""
        Xd = X if hasattr(X, "data_ptr") else self.ctx.to_device(X)
        n = Xd.shape[0]
        self._ensure(n, S)
        self._prepare_checked()
        L = len(self.layers)
        outs = {}
        arrs = {}
        for key in ("F", "mean", "var"):
            if key in want:
                ts = [self.ctx.empty(S, n, layer.num_outputs) for layer in self.layers]
                a = (C.c_void_p * L)(*[t.data_ptr() for t in ts])
            else:
                ts, a = None, None
            outs[key], arrs[key] = ts, a
        zp, zst, keep = self._zs_args(zs, S, n)
        _lib.check(self.lib.dsdgp_model_propagate(self.model, ptr(Xd), n, S, zp, zst, C.c_uint64(seed), arrs["F"],
                                                  arrs["mean"], arrs["var"]))
        return outs["F"], outs["mean"], outs["var"]

    def elbo(self, X, Y, S, zs=None, seed=0, data_scale=1.0, kl_weight=1.0, with_grad=False, sync=True, grad_from_layer=0,
             grad_q_only=False):
        """grad_from_layer = l > 0: the reverse pass stops below layer l, as tf.gradients(loss, var_list) does for a var_list of
        upper-layer (q_mu, q_sqrt) pairs (NatGradOptimizer); the gradient entries of the lower layers are then NOT updated.
        grad_q_only: var_list holds nothing but (q_mu, q_sqrt) pairs — only those entries of the layers >= l are produced (the other
        entries of these layers are undefined afterwards; an Adam step is refused until a full gradient has been evaluated)."""
        Xd = X if hasattr(X, "data_ptr") else self.ctx.to_device(X)
        Yd = Y if hasattr(Y, "data_ptr") else self.ctx.to_device(Y)
        n = Xd.shape[0]
        self._check_targets_shape(Yd, n)
        self._ensure(n, S)
        self._upload_if_needed()
        zp, zst, keep = self._zs_args(zs, S, n)
        gfl = int(grad_from_layer) if with_grad else 0
        if gfl != getattr(self, "_grad_first", 0):
            _lib.check(self.lib.dsdgp_model_set_grad_first_layer(self.model, gfl))
            self._grad_first = gfl
        qo = bool(grad_q_only) and bool(with_grad)
        if qo != getattr(self, "_grad_q_only", False):
            _lib.check(self.lib.dsdgp_model_set_grad_q_only(self.model, int(qo)))
            self._grad_q_only = qo
        _lib.check(self.lib.dsdgp_model_elbo(self.model, ptr(Xd), ptr(Yd), n, S, zp, zst, C.c_uint64(seed),
                                             float(data_scale), float(kl_weight), int(with_grad), ptr(self.out4)))
        if not sync:
            return None
        self.ctx.sync()
        out = self.out4.cpu().numpy()
        if out[3] != 0.0:
            raise _lib.CholeskyError(f"Cholesky decomposition was not successful (Kuu pivot {int(out[3])})")
        return out

    def forward_saved(self, X, S, zs=None, seed=0):
        """dsdgp_model_forward_saved: the forward pass of a gradient evaluation without a likelihood -> (mean, var) of the last layer,
        device tensors (S, n, D_out).  The reverse pass it keeps its state for is `backward_adjoints`; any other call of this engine in
        between (an evaluation, an upload of changed parameters, an optimiser step) drops that state.  Asynchronous."""
        Xd = X if hasattr(X, "data_ptr") else self.ctx.to_device(X)
        n = Xd.shape[0]
        self._ensure(n, S)
        self._upload_if_needed()
        if getattr(self, "_grad_first", 0) != 0:           # a restriction left by NatGradOptimizer: lifted, as train_step does
            _lib.check(self.lib.dsdgp_model_set_grad_first_layer(self.model, 0))
            self._grad_first = 0
        if getattr(self, "_grad_q_only", False):
            _lib.check(self.lib.dsdgp_model_set_grad_q_only(self.model, 0))
            self._grad_q_only = False
        zp, zst, keep = self._zs_args(zs, S, n)
        D = self.layers[-1].num_outputs
        mean, var = self.ctx.empty(S, n, D), self.ctx.empty(S, n, D)
        _lib.check(self.lib.dsdgp_model_forward_saved(self.model, ptr(Xd), n, S, zp, zst, C.c_uint64(seed), ptr(mean), ptr(var)))
        self._saved_shape = (self.generation, S, n, D)
        self._saved_keep = (Xd, keep)       # the reverse pass reads X and the explicit draws again
        return mean, var

    def backward_adjoints(self, dmean, dvar, kl_weight=1.0, sync=True):
        """dsdgp_model_backward_adjoints: dmean, dvar (S, n, D_out) are dJ/dmean and dJ/dvar of a scalar J of `forward_saved`'s results.
        Leaves the gradient of loss = -(J - kl_weight * sum KL) where elbo(with_grad=True) leaves its own (`gradient_dict`, `adam_step`);
        the likelihood's entry is 0.  Returns out4 = [-kl_weight * sum KL, 0, kl_weight * sum KL, 0] (None with sync=False)."""
        shape = getattr(self, "_saved_shape", None)
        if shape is None or shape[0] != self.generation or self._host_dirty:
            raise _lib.DsdgpError("backward_adjoints: no saved forward pass (forward_saved) is this engine's last evaluation")
        dm, dv = self.ctx.as_device(dmean), self.ctx.as_device(dvar)
        for what, t in (("dmean", dm), ("dvar", dv)):       # the library copies S n D_out doubles from each
            if tuple(t.shape) != shape[1:]:
                raise ValueError(f"backward_adjoints: {what} has shape {tuple(t.shape)}, the saved forward pass {shape[1:]}")
        try:
            _lib.check(self.lib.dsdgp_model_backward_adjoints(self.model, ptr(dm), ptr(dv), float(kl_weight), ptr(self.out4)))
        finally:
            self._saved_shape = self._saved_keep = None
        if not sync:
            return None
        self.ctx.sync()
        out = self.out4.cpu().numpy()
        if out[3] != 0.0:
            raise _lib.CholeskyError(f"Cholesky decomposition was not successful (Kuu pivot {int(out[3])})")
        return out

    def _mixture_batch_args(self, Xd, S, zs, Yd=None):
        """What evaluate_batch, quantiles_batch, calibration_batch and classification_batch do ahead of their library call -> (n, zp, zst, keep)"""
        n = Xd.shape[0]
        if Yd is not None:
            self._check_targets_shape(Yd, n)
        self._ensure(n, S)
        self._prepare_checked()
        return (n, *self._zs_args(zs, S, n))

    def evaluate_batch(self, Xd, Yd, S, acc, accumulate, zs=None, seed=0, rows=None):
        """dsdgp_model_evaluate on one batch of device rows: forward pass + mixture reduction into the device accumulator `acc`
        (3 x D_out of the last layer; added to when `accumulate`), per-row values into `rows` (n, D_out, 3) if given.  Asynchronous."""
        n, zp, zst, keep = self._mixture_batch_args(Xd, S, zs, Yd)
        _lib.check(self.lib.dsdgp_model_evaluate(self.model, ptr(Xd), ptr(Yd), n, S, zp, zst, C.c_uint64(seed), ptr(rows), ptr(acc),
                                                 int(bool(accumulate))))
        return keep

    def quantiles_batch(self, Xd, S, probs, q, level=1, zs=None, seed=0):
        """dsdgp_model_quantiles on one batch of device rows: forward pass + the mixture's quantiles at the host array `probs` into the
        device tensor `q` (n, D_out, P).  level 1: the predictive y (Gaussian likelihood), 0: the latent f.  Asynchronous."""
        probs = np.ascontiguousarray(probs, dtype=np.float64)
        n, zp, zst, keep = self._mixture_batch_args(Xd, S, zs)
        _lib.check(self.lib.dsdgp_model_quantiles(self.model, ptr(Xd), n, S, zp, zst, C.c_uint64(seed), int(level),
                                                  probs.ctypes.data_as(_lib.c_double_p), probs.size, ptr(q)))
        return keep

    def calibration_batch(self, Xd, Yd, S, probs, acc, accumulate, zs=None, seed=0, rows=None):
        """dsdgp_model_calibration on one batch of device rows: forward pass + PIT / CRPS reduction into the device accumulator `acc`
        ((2 + P) x D_out; added to when `accumulate`), per-row [u, CRPS] into `rows` (n, D_out, 2) if given.  Asynchronous."""
        probs = np.ascontiguousarray(probs, dtype=np.float64)
        n, zp, zst, keep = self._mixture_batch_args(Xd, S, zs, Yd)
        _lib.check(self.lib.dsdgp_model_calibration(self.model, ptr(Xd), ptr(Yd), n, S, zp, zst, C.c_uint64(seed),
                                                    probs.ctypes.data_as(_lib.c_double_p), probs.size, ptr(rows), ptr(acc),
                                                    int(bool(accumulate))))
        return keep

    def classification_batch(self, Xd, Yd, S, bins, acc, accumulate, zs=None, seed=0, probs=None, rows=None):
        """dsdgp_model_classification on one batch of device rows (MultiClass / Bernoulli): forward pass + class probabilities + report
        reduction into the device accumulator `acc` ((4 + 3 bins + C + C^2) x ND; added to when `accumulate`), the mixture class
        probabilities into `probs` (n, D_out) and per-row [predicted class, conf, l, brier] into `rows` (n, ND, 4) if given.
        Asynchronous."""
        n, zp, zst, keep = self._mixture_batch_args(Xd, S, zs, Yd)
        _lib.check(self.lib.dsdgp_model_classification(self.model, ptr(Xd), ptr(Yd), n, S, zp, zst, C.c_uint64(seed), int(bins),
                                                       ptr(probs), ptr(rows), ptr(acc), int(bool(accumulate))))
        return keep

    def adam_step(self, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8):
        # the library refuses a pruned gradient: count the step only once it has been taken
        _lib.check(self.lib.dsdgp_model_adam_step(self.model, lr, beta1, beta2, eps, self.adam_t + 1))
        self.adam_t += 1
        self._dev_dirty = True
        self._needs_prepare = True

    def train_step(self, X, Y, S, zs=None, seed=0, data_scale=1.0, kl_weight=1.0, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8):
        """ELBO + gradient + Adam update in one library call (single-process training); asynchronous, result scalars in out4."""
        Xd = X if hasattr(X, "data_ptr") else self.ctx.to_device(X)
        Yd = Y if hasattr(Y, "data_ptr") else self.ctx.to_device(Y)
        n = Xd.shape[0]
        self._check_targets_shape(Yd, n)
        self._ensure(n, S)
        self._upload_if_needed()
        zp, zst, keep = self._zs_args(zs, S, n)
        if getattr(self, "_grad_first", 0) != 0:
            _lib.check(self.lib.dsdgp_model_set_grad_first_layer(self.model, 0))
            self._grad_first = 0
        if getattr(self, "_grad_q_only", False):
            _lib.check(self.lib.dsdgp_model_set_grad_q_only(self.model, 0))
            self._grad_q_only = False
        _lib.check(self.lib.dsdgp_model_train_step(self.model, ptr(Xd), ptr(Yd), n, S, zp, zst, C.c_uint64(seed), float(data_scale),
                                                   float(kl_weight), lr, beta1, beta2, eps, self.adam_t + 1, ptr(self.out4)))
        self.adam_t += 1
        self._dev_dirty = True
        self._needs_prepare = True

    def train_step_minibatch(self, Xall, Yall, idx, idx_offset, n, S, seed=0, data_scale=1.0, kl_weight=1.0, lr=0.01, beta1=0.9,
                             beta2=0.999, eps=1e-8):
        """train_step on rows idx[idx_offset : idx_offset + n] of the device-resident data (gather inside the step's first launch)."""
        self._check_targets_shape(Yall, Yall.shape[0])
        if Xall.shape[0] != Yall.shape[0]:
            raise ValueError(f"X has {Xall.shape[0]} rows, Y {Yall.shape[0]}")
        if idx_offset < 0 or idx_offset + n > idx.numel():
            raise ValueError(f"index span [{idx_offset}, {idx_offset + n}) outside the index buffer of {idx.numel()} entries")
        self._ensure(n, S)
        self._upload_if_needed()
        if getattr(self, "_grad_first", 0) != 0:
            _lib.check(self.lib.dsdgp_model_set_grad_first_layer(self.model, 0))
            self._grad_first = 0
        if getattr(self, "_grad_q_only", False):
            _lib.check(self.lib.dsdgp_model_set_grad_q_only(self.model, 0))
            self._grad_q_only = False
        _lib.check(self.lib.dsdgp_model_train_step_minibatch(self.model, ptr(Xall), ptr(Yall), ptr(idx), int(idx_offset), int(n), S,
                                                             C.c_uint64(seed), float(data_scale), float(kl_weight), lr, beta1, beta2,
                                                             eps, self.adam_t + 1, ptr(self.out4)))
        self.adam_t += 1
        self._dev_dirty = True
        self._needs_prepare = True

    def _check_targets_shape(self, Yd, n):
        """Y must be (n, D_out of the last layer) for the element-wise likelihoods, (n, 1) labels for MultiClass: the likelihood
        kernels index Y[(row % n) * DY + d] and would read out of bounds otherwise."""
        want = 1 if isinstance(self.likelihood, MultiClass) else self.layers[-1].num_outputs
        if tuple(Yd.shape) != (n, want):
            raise ValueError(f"Y has shape {tuple(Yd.shape)}, expected {(n, want)} (rows of X x outputs of the last layer)")

    def natgrad_step(self, l, gamma, check=True):
        """[UPSTREAM] NatGradOptimizer(gamma) step on layer l's (q_mu, q_sqrt) from the gradient of the last
        elbo(with_grad=True).  A step whose A = S^-1 + 2 gamma Sbar is not positive definite for some output is refused: the library
        leaves theta as it was (CholeskyError with check=True; silently with check=False, as every unchecked call)."""
        info = C.c_int(0)
        try:
            _lib.check(self.lib.dsdgp_model_natgrad_step(self.model, l, float(gamma), C.byref(info) if check else None))
        finally:
            # also on the error path: the launches were issued and the library has dropped its prepared state
            self._dev_dirty = True
            self._needs_prepare = True

    def set_sample_weights(self, w_dev):
        """DGP_Quad (dgp.py:160-166): weight the S propagated samples by w (device tensor, kept alive here) instead of 1/S;
        None restores the Monte-Carlo mean."""
        self._sample_w = w_dev
        _lib.check(self.lib.dsdgp_model_set_sample_weights(self.model, ptr(w_dev) if w_dev is not None else None,
                                                           int(w_dev.numel()) if w_dev is not None else 0))

    def layer_kl(self, l):
        self._prepare_checked()
        out = self.ctx.empty(1)
        _lib.check(self.lib.dsdgp_model_layer_kl(self.model, l, ptr(out)))
        self.ctx.sync()
        return float(out.cpu().numpy()[0])

    def layer_matrix(self, l, which):
        """One of layer l's factorisation buffers as the kernels left it: the whole padded (Mp, Mp) array, nothing cleaned up.
        which: "Lu" (white = True models only: DsdgpError otherwise), "Linv" = Lu^-1, "LinvT" = Lu^-T, "Kinv" = Ku^-1."""
        code = {"Lu": _lib.MAT_LU, "Linv": _lib.MAT_LUINV, "LinvT": _lib.MAT_LUINVT, "Kinv": _lib.MAT_KUINV}[which]
        self._prepare_checked()
        Mp = padded_M(self.layers[l].feature.Z.shape[0])
        out = np.empty((Mp, Mp), dtype=np.float64)
        _lib.check(self.lib.dsdgp_model_layer_matrix(self.model, l, code, out.ctypes.data_as(C.c_void_p), Mp))
        return out

    def layer_conditional(self, l, X):
        Xd = X if hasattr(X, "data_ptr") else self.ctx.to_device(X)
        n = Xd.shape[0]
        self._ensure(max(n, 1), 1)
        self._prepare_checked()
        D = self.layers[l].num_outputs
        mean, var = self.ctx.empty(n, D), self.ctx.empty(n, D)
        _lib.check(self.lib.dsdgp_model_layer_conditional(self.model, l, ptr(Xd), n, ptr(mean), ptr(var)))
        return mean, var

    def randn(self, shape, seed=None):
        """N(0,1) draws from the device Philox generator (tf.random_normal, layers.py:101-102) as a numpy array."""
        n = int(np.prod(shape))
        out = self.ctx.empty(n)
        self._rng_calls = getattr(self, "_rng_calls", 0) + 1
        _lib.check(self.lib.dsdgp_randn(self.ctx.handle, C.c_uint64(0x5eed if seed is None else seed),
                                        C.c_uint64(1 << 32 | self._rng_calls), n, ptr(out)))
        self.ctx.sync()
        return out.cpu().numpy().reshape(shape)

    def layer_conditional_full(self, l, X):
        """conditional_ND(X, full_cov=True): mean (n, D), var (n, n, D) (layers.py:206-209)."""
        Xd = X if hasattr(X, "data_ptr") else self.ctx.to_device(X)
        n = Xd.shape[0]
        self._ensure(max(n, 1), 1)
        self._prepare_checked()
        D = self.layers[l].num_outputs
        mean, var = self.ctx.empty(n, D), self.ctx.empty(n, n, D)
        _lib.check(self.lib.dsdgp_model_layer_conditional_full(self.model, l, ptr(Xd), n, ptr(mean), ptr(var)))
        return mean, var

    def gradient_dict(self):
        """d loss / d (unconstrained) parameters of the last elbo(with_grad=True), keyed like oracle/model.py."""
        self.ctx.sync()
        g = self.grad.cpu().numpy()
        out = {}
        names = {}
        for l, layer in enumerate(self.layers):
            stat, wk = self._params_of(layer)
            names[id(layer.feature.Z)] = f"l{l}.Z"
            names[id(layer.q_mu)] = f"l{l}.q_mu"
            names[id(layer.q_sqrt)] = f"l{l}.q_sqrt"
            names[id(stat.variance)] = f"l{l}.kern_variance_raw"
            names[id(stat.lengthscales)] = f"l{l}.kern_lengthscales_raw"
            if wk is not None:
                names[id(wk.variance)] = f"l{l}.white_variance_raw"
            if layer.mean_function.kind == "linear":
                names[id(layer.mean_function.A)] = f"l{l}.mean_A"
                names[id(layer.mean_function.b)] = f"l{l}.mean_b"
        p = likelihood_entry(self.likelihood)[1]
        if p is not None:
            names[id(p)] = "lik_variance_raw"
        for p, off, cnt, kind in self.entries:
            out[names[id(p)]] = g[off:off + cnt].reshape(p.shape).copy()
        return out
