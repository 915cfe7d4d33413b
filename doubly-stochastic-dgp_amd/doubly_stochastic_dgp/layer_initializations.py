"""Layer construction for DGP (host-side, one-off).  Same two entry points and argument meaning as the reference's
layer_initializations.py:16-52 / :55-79, organised differently: the inter-layer width maps are PLANNED first (one
`_width_map` per boundary) and the layers are then built from the plan."""
import ctypes as C

import numpy as np

from . import settings
from .gpflow_compat import Identity, Linear, Stationary, Zero, split_kernel
from .layers import SVGP_Layer

KMEANS_MAX_M, KMEANS_MAX_D = 2048, 1024          # KM_MAX_M, KM_MAX_D of csrc/kmeans.hip
GREEDY_MAX_M, GREEDY_MAX_D = 2048, 1024          # GR_MAX_M, GR_MAX_D of csrc/greedy.hip
_GREEDY_KIND = {"rbf": 0, "matern52": 1}         # DSDGP_KERN_*
PCA_MAX_D, PCA_MAX_SWEEPS = 1024, 64             # PCA_MAX_D, PCA_MAX_SWEEPS of csrc/pca.hip


def _kmeans_args(X, M, iter, init):
    """Everything kmeans_inducing can refuse without a device -> (n, D, M, iters, index array or None, centre array or None); called
    before the engine's context is touched, so a machine without a GPU reports the bad argument and not the missing device."""
    on_device = hasattr(X, "data_ptr")
    if not on_device:
        X = np.asarray(X)
    if len(X.shape) != 2:
        raise ValueError(f"X must be a 2-D (n, D) array, not one of shape {tuple(X.shape)}")
    n, D = int(X.shape[0]), int(X.shape[1])
    if isinstance(M, bool) or not isinstance(M, (int, np.integer)):
        raise ValueError(f"M must be an integer, not {M!r}")
    M, iters = int(M), int(iter)
    if not 2 <= M <= KMEANS_MAX_M:
        raise ValueError(f"M = {M} outside 2 .. {KMEANS_MAX_M}")
    if not 1 <= D <= KMEANS_MAX_D:
        raise ValueError(f"D = {D} outside 1 .. {KMEANS_MAX_D}")
    if iters < 1:
        raise ValueError(f"iter = {iters}: at least one iteration")
    if M > n:
        raise ValueError(f"M = {M} centres from n = {n} rows")
    if not on_device and not np.all(np.isfinite(np.asarray(X, dtype=np.float64))):
        raise ValueError("X holds a non-finite value")
    idx = centres = None
    if init is not None:
        if hasattr(init, "data_ptr"):
            init = init.cpu().numpy()
        init = np.asarray(init)
        if init.ndim == 1:
            if init.shape != (M,) or not np.issubdtype(init.dtype, np.integer):
                raise ValueError(f"init as row indices must be an integer array of shape ({M},)")
            if init.min() < 0 or init.max() >= n:
                raise ValueError(f"init holds a row index outside 0 .. {n - 1}")
            idx = init.astype(np.int64)
        elif init.shape == (M, D):
            centres = np.ascontiguousarray(init, dtype=np.float64)
            if not np.all(np.isfinite(centres)):
                raise ValueError("init holds a non-finite value")
        else:
            raise ValueError(f"init must be ({M},) row indices or ({M}, {D}) centres, not shape {init.shape}")
    return n, D, M, iters, idx, centres


def kmeans_inducing(X, M, iter=10, seed=0, init=None, return_info=False):
    """Inducing inputs by k-means on the device: what demos/run_regression.py:57 does with scipy's kmeans2(X, M, minit='points')[0].
    X: numpy array or device tensor (n, D).  init None: the start centres are the rows np.random.default_rng(seed).choice(n, M,
    replace=False) — the minit='points' rule, M distinct rows, but numpy's Generator stream and not the RandomState draw scipy makes,
    so the same seed does not reproduce scipy's Z.  init may instead be M row indices, shape (M,), or the centres themselves, (M, D).
    `iter` Lloyd iterations (kmeans2's default 10): ties go to the lowest centre, a centre without rows keeps its value; the same
    X, M, iter and start give the same bits on every call and every rank.  Returns Z (M, D) as numpy; with return_info also a dict:
    `labels` (n,) int32 and `counts` (M,) int64 of the assignment Z was averaged from (kmeans2's second result), `inertia` = that
    assignment's sum of squared distances to its centres.
    ValueError, before any device is looked for: X not 2-D, M outside 2 .. 2048, D outside 1 .. 1024, iter < 1, M > n, an init of the
    wrong shape or with an index out of range, a non-finite value in a numpy X or init."""
    n, D, M, iters, idx, centres = _kmeans_args(X, M, iter, init)
    if idx is None and centres is None:
        idx = np.random.default_rng(seed).choice(n, M, replace=False).astype(np.int64)
    from . import _lib
    from .engine import Context
    ctx = Context.get()
    torch = ctx.torch
    dev = f"cuda:{ctx.device}"
    with torch.cuda.stream(ctx.tstream):
        if hasattr(X, "data_ptr"):
            Xd = X.to(device=dev, dtype=torch.float64).contiguous()
            Z0 = Xd[torch.as_tensor(idx).to(dev)].contiguous() if centres is None else ctx.to_device(centres)
        else:
            Xh = np.ascontiguousarray(X, dtype=np.float64)
            Xd = ctx.to_device(Xh)
            Z0 = ctx.to_device(Xh[idx] if centres is None else centres)
        Z = ctx.empty(M, D)
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        counts = torch.empty(M, dtype=torch.int64, device=dev)
        inertia = ctx.empty(1)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(ctx.lib.dsdgp_kmeans(ctx.handle, p(Xd), n, D, M, p(Z0), iters, p(Z), p(labels), p(counts), p(inertia)))
    ctx.sync()
    Zh = Z.cpu().numpy()
    if not return_info:
        return Zh
    return Zh, {"labels": labels.cpu().numpy(), "counts": counts.cpu().numpy(), "inertia": float(inertia.cpu().numpy()[0])}


def _greedy_args(X, M, kernel, first, threshold):
    """Everything greedy_inducing can refuse without a device -> (n, D, M, first or -1, threshold, kind, ard, variance, white variance
    or None, lengthscales); called before the engine's context is touched, as _kmeans_args is."""
    on_device = hasattr(X, "data_ptr")
    if not on_device:
        X = np.asarray(X)
    if len(X.shape) != 2:
        raise ValueError(f"X must be a 2-D (n, D) array, not one of shape {tuple(X.shape)}")
    n, D = int(X.shape[0]), int(X.shape[1])
    if isinstance(M, bool) or not isinstance(M, (int, np.integer)):
        raise ValueError(f"M must be an integer, not {M!r}")
    M = int(M)
    if not 2 <= M <= GREEDY_MAX_M:
        raise ValueError(f"M = {M} outside 2 .. {GREEDY_MAX_M}")
    if not 1 <= D <= GREEDY_MAX_D:
        raise ValueError(f"D = {D} outside 1 .. {GREEDY_MAX_D}")
    if M > n:
        raise ValueError(f"M = {M} points from n = {n} rows")
    if n >= 2 ** 31:
        raise ValueError(f"n = {n}: at most 2^31 - 1 rows")
    if first is None:
        first = -1
    else:
        if isinstance(first, bool) or not isinstance(first, (int, np.integer)):
            raise ValueError(f"first must be a row index, not {first!r}")
        first = int(first)
        if not 0 <= first < n:
            raise ValueError(f"first = {first} outside 0 .. {n - 1}")
    threshold = float(settings.jitter if threshold is None else threshold)
    if not threshold >= 0.0:
        raise ValueError(f"threshold = {threshold}: a non-negative number")
    try:
        stat, white = split_kernel(kernel)
    except NotImplementedError as e:
        raise ValueError(str(e))
    if not isinstance(stat, Stationary) or stat.kind not in _GREEDY_KIND:
        raise ValueError(f"kernel {type(stat).__name__} is neither RBF nor Matern52")
    if int(stat.input_dim) != D:
        raise ValueError(f"the kernel's input_dim = {stat.input_dim} is not D = {D}")
    if not on_device and not np.all(np.isfinite(np.asarray(X, dtype=np.float64))):
        raise ValueError("X holds a non-finite value")
    ls = np.ascontiguousarray(np.asarray(stat.lengthscales.value, dtype=np.float64).reshape(-1))
    return (n, D, M, first, threshold, _GREEDY_KIND[stat.kind], int(stat.ARD), float(stat.variance.value),
            None if white is None else float(white.variance.value), ls)


def greedy_inducing(X, M, kernel, first=None, threshold=None, return_info=False):
    """Inducing inputs by the greedy conditional-variance rule on the device (the pivoted Cholesky factorisation of K(X, X);
    "ConditionalVariance" of Burt, Rasmussen and van der Wilk 2020): each step takes the row of X whose variance under `kernel`,
    conditioned on the rows already chosen, is largest (ties: the lowest row).  X: numpy array or device tensor (n, D).  kernel: a
    gpflow_compat RBF or Matern52 (scalar or ARD lengthscales), alone or in a sum with White, mapped as the engine maps a layer's kernel.
    first: the row to start from (default: row 0, every row having the same prior variance).  The selection stops early at the first
    row whose conditional variance is <= threshold; None means settings.jitter — a pivot below what Ku gets added to its diagonal is
    one the jitter dominates.  Returns Z (m, D) as numpy, m <= M, its rows bit copies of rows of X; with return_info also a dict:
    `indices` (m,) int32, `m`, `residual` (m,): the conditional variance of each row when it was chosen, `trace` (m,): tr(Kff - Qff)
    after 1 .. m points — the quantity that bounds the gap of the sparse approximation, so the answer to "is M large enough?" — and
    `L` (m, m): the lower Cholesky factor of k(Z, Z) (+ White) in pivot order.  The same arguments give the same bits on every call.
    ValueError, before any device is looked for: X not 2-D, M outside 2 .. 2048, D outside 1 .. 1024, M > n, first outside 0 .. n-1, a
    negative or NaN threshold, a non-finite value in a numpy X, a kernel whose input_dim is not D or that is not RBF / Matern52 (+ White)."""
    n, D, M, first, threshold, kind, ard, variance, wvar, ls = _greedy_args(X, M, kernel, first, threshold)
    from . import _lib
    from .engine import Context
    ctx = Context.get()
    torch = ctx.torch
    dev = f"cuda:{ctx.device}"
    spec = _lib.KernelSpec(kind=kind, input_dim=D, ard=ard, has_white=int(wvar is not None), variance=variance,
                           white_variance=0.0 if wvar is None else wvar, lengthscales=ls.ctypes.data_as(_lib.c_double_p))
    with torch.cuda.stream(ctx.tstream):
        Xd = X.to(device=dev, dtype=torch.float64).contiguous() if hasattr(X, "data_ptr") else ctx.to_device(X)
        idx = torch.empty(M, dtype=torch.int32, device=dev)
        m_out = torch.empty(1, dtype=torch.int32, device=dev)
        Z, res, tr, L = ctx.empty(M, D), ctx.empty(M), ctx.empty(M), ctx.empty(M, M)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(ctx.lib.dsdgp_greedy_inducing(ctx.handle, C.byref(spec), p(Xd), n, M, first, threshold, p(idx), p(m_out), p(Z), p(res),
                                             p(tr), p(L), M))
    ctx.sync()
    m = int(m_out.cpu().numpy()[0])
    Zh = Z.cpu().numpy()[:m].copy()
    if not return_info:
        return Zh
    return Zh, {"indices": idx.cpu().numpy()[:m].copy(), "m": m, "residual": res.cpu().numpy()[:m].copy(),
                "trace": tr.cpu().numpy()[:m].copy(), "L": L.cpu().numpy()[:m, :m].copy()}


def _pca_args(X, k, max_sweeps):
    """Everything pca_map can refuse without a device -> (n, D, k, max_sweeps); called before the engine's context is touched, as
    _kmeans_args is."""
    on_device = hasattr(X, "data_ptr")
    if not on_device:
        X = np.asarray(X)
    if len(X.shape) != 2:
        raise ValueError(f"X must be a 2-D (n, D) array, not one of shape {tuple(X.shape)}")
    n, D = int(X.shape[0]), int(X.shape[1])
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"k must be an integer, not {k!r}")
    if isinstance(max_sweeps, bool) or not isinstance(max_sweeps, (int, np.integer)):
        raise ValueError(f"max_sweeps must be an integer, not {max_sweeps!r}")
    k, max_sweeps = int(k), int(max_sweeps)
    if not 1 <= D <= PCA_MAX_D:
        raise ValueError(f"D = {D} outside 1 .. {PCA_MAX_D}")
    if not 1 <= k <= D:
        raise ValueError(f"k = {k} outside 1 .. D = {D}")
    if n < 1:
        raise ValueError("X has no rows")
    if n >= 2 ** 31:
        raise ValueError(f"n = {n}: at most 2^31 - 1 rows")
    if not 1 <= max_sweeps <= PCA_MAX_SWEEPS:
        raise ValueError(f"max_sweeps = {max_sweeps} outside 1 .. {PCA_MAX_SWEEPS}")
    if not on_device and not np.all(np.isfinite(np.asarray(X, dtype=np.float64))):
        raise ValueError("X holds a non-finite value")
    return n, D, k, max_sweeps


def pca_map(X, k, center=False, max_sweeps=30, return_info=False):
    """The step-down map of init_layers_linear on the device: the top k right singular vectors of X, which the reference takes from
    np.linalg.svd(X, full_matrices=False) (layer_initializations.py:35), as the top k eigenvectors of C = X^T X (center=False, what
    svd(X) diagonalises) or of the centred (X - mean)^T (X - mean) (center=True).  X: numpy array or device tensor (n, D).  C is formed
    on the fp64 MFMA pipe and diagonalised by a round-robin two-sided Jacobi iteration, at most max_sweeps sweeps, all on the device.
    Returns T (D, k) as numpy: column j is the unit eigenvector of the j-th largest eigenvalue, its entry of largest magnitude positive
    (ties: the lowest row) — np.linalg.svd's rows up to that sign.  The same arguments give the same bits on every call and every rank.
    With return_info also a dict: `eigenvalues` (D,), non-increasing; `singular_values` (D,) = sqrt(max(eigenvalues, 0)); `explained`
    (D,) = cumsum(max(eigenvalues, 0)) / sum(max(eigenvalues, 0)) (zeros if the sum is zero): the share of tr(C) the first 1 .. D
    directions carry, so explained[k - 1] answers "is the narrower width wide enough?"; `mean` (D,): the column means (zeros when
    center=False); `gram` (D, D): C as the device formed it; `sweeps`; `converged`.
    RuntimeError if the iteration has not converged after max_sweeps sweeps — unless return_info is set: then the caller reads the flag.
    ValueError, before any device is looked for: X not 2-D, k not an integer or outside 1 .. D, D outside 1 .. 1024, no rows,
    max_sweeps outside 1 .. 64, a non-finite value in a numpy X."""
    n, D, k, max_sweeps = _pca_args(X, k, max_sweeps)
    from . import _lib
    from .engine import Context
    ctx = Context.get()
    torch = ctx.torch
    dev = f"cuda:{ctx.device}"
    with torch.cuda.stream(ctx.tstream):
        Xd = X.to(device=dev, dtype=torch.float64).contiguous() if hasattr(X, "data_ptr") else ctx.to_device(X)
        W, evals, mean, gram = ctx.empty(D, k), ctx.empty(D), ctx.empty(D), ctx.empty(D, D)
        info = torch.empty(4, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(ctx.lib.dsdgp_pca(ctx.handle, p(Xd), n, D, k, int(bool(center)), max_sweeps, p(W), k, p(evals), p(mean), p(gram), p(info)))
    ctx.sync()
    T = W.cpu().numpy()
    flags = info.cpu().numpy()
    converged, sweeps = bool(flags[0]), int(flags[1])
    if not return_info:
        if not converged:
            raise RuntimeError(f"pca_map: the Jacobi iteration has not converged after {sweeps} sweeps ({int(flags[2])} rotations in "
                               "the last one); raise max_sweeps")
        return T
    lam = evals.cpu().numpy()
    pos = np.maximum(lam, 0.0)
    total = pos.sum()
    return T, {"eigenvalues": lam, "singular_values": np.sqrt(pos), "explained": np.cumsum(pos) / total if total > 0 else np.zeros(D),
               "mean": mean.cpu().numpy(), "gram": gram.cpu().numpy(), "sweeps": sweeps, "converged": converged}


def _check_pca(pca):
    if pca not in ("host", "device"):
        raise ValueError(f"pca = {pca!r}: 'host' or 'device'")


def _width_map(d_from, d_to, cloud, pca="host"):
    """The fixed linear map between two layer widths, or None when they agree (identity mean function).
    narrower: the top `d_to` right singular vectors of `cloud` (the data as seen at this depth) — a PCA projection; pca="host":
              numpy's SVD of the whole cloud, pca="device": pca_map(cloud, d_to);
    wider:    [I | 0], the extra coordinates start at zero."""
    _check_pca(pca)
    if d_from == d_to:
        return None
    if d_from > d_to:
        if pca == "device":
            return pca_map(cloud, d_to)
        right = np.linalg.svd(cloud, full_matrices=False)[2]
        return right[:d_to].T.copy()
    out = np.zeros((d_from, d_to))
    out[np.arange(d_from), np.arange(d_from)] = 1.0
    return out


def _plan_widths(X, Z, widths, pca="host"):
    """[(inducing inputs, output width, map-or-None)] for every inner boundary, plus the inducing inputs of the last layer.
    Data and inducing inputs are carried through the maps together so that each layer's Z lives in that layer's input space."""
    cloud, ind = np.array(X, dtype=np.float64), np.array(Z, dtype=np.float64)
    plan = []
    for d_from, d_to in zip(widths[:-1], widths[1:]):
        T = _width_map(d_from, d_to, cloud, pca)
        plan.append((ind, d_to, T))
        if T is not None:
            cloud, ind = cloud @ T, ind @ T
    return plan, ind


def _frozen_linear(T):
    mf = Linear(T)
    mf.set_trainable(False)          # the PCA / padding maps are constants of the model (layer_initializations.py:41-42)
    return mf


def init_layers_linear(X, Y, Z, kernels, num_outputs=None, mean_function=None, Layer=SVGP_Layer, white=False, pca="host"):
    """Inner layers get an identity mean where consecutive kernels share their input width and a fixed linear map where they do
    not (see `_width_map`); the last layer gets `mean_function` (default Zero) and `num_outputs` (default: columns of Y).
    pca: where the step-down maps are computed, "host" (np.linalg.svd, as the reference) or "device" (pca_map)."""
    _check_pca(pca)
    final_mean = Zero() if mean_function is None else mean_function
    n_out = num_outputs or Y.shape[1]
    plan, Z_last = _plan_widths(X, Z, [k.input_dim for k in kernels], pca)
    layers = [Layer(k, Zl, width, Identity() if T is None else _frozen_linear(T), white=white)
              for k, (Zl, width, T) in zip(kernels[:-1], plan)]
    layers.append(Layer(kernels[-1], Z_last, n_out, final_mean, white=white))
    return layers


def _padded_inducing(Z, extra, scale):
    """Z with `extra` further columns drawn N(0, (2 scale)^2) from numpy's GLOBAL generator, as the reference's np.random.randn
    does (layer_initializations.py:67,76) — seed it for reproducibility."""
    return np.concatenate([Z, np.random.randn(Z.shape[0], extra) * (2.0 * scale)], 1)


def init_layers_input_prop(X, Y, Z, kernels, num_outputs=None, mean_function=None, Layer=SVGP_Layer, white=False):
    """layer_initializations.py:55-79: every inner layer forwards the D data inputs beside its own outputs
    (Layer(input_prop_dim=D), zero mean), so kernel l sees D + (its layer's own width) inputs; the inducing inputs of the
    additional coordinates are random, scaled by the standard deviation of the kernel that produces them."""
    final_mean = Zero() if mean_function is None else mean_function
    n_out = num_outputs or Y.shape[1]
    D = X.shape[1]
    sd = [float(np.asarray(k.variance.value)) ** 0.5 for k in kernels]
    layers = []
    for l in range(len(kernels) - 1):
        k = kernels[l]
        layers.append(Layer(k, _padded_inducing(Z, k.input_dim - D, sd[l]), kernels[l + 1].input_dim - D, Zero(), white=white,
                            input_prop_dim=D))
    k = kernels[-1]
    layers.append(Layer(k, _padded_inducing(Z, k.input_dim - D, sd[-2] if k.input_dim > D else 1.0), n_out, final_mean, white=white))
    return layers
