"""The greedy conditional-variance selection of inducing points (pivoted Cholesky of K(X, X)) in numpy, the yardstick of
tests/test_gpu_greedy.py.  greedy(..., dtype=np.longdouble) is the reference; greedy(..., dtype=np.float64) is the same program in
plain float64, the yardstick for rounding: a device result is allowed a small multiple of the float64 version's own distance from the
long-double one.

    d_i = v (+ white)
    for j = 0 .. M-1:
        p_j = first if j == 0 and a first row was given, else argmax_i d_i over the rows not yet chosen (np.argmax: the lowest i on ties)
        stop if d_p <= threshold                                     (m = j)
        c_j[i] = (k(x_i, x_p) - sum_{t<j} c_t[i] c_t[p]) / sqrt(d_p)
        d_i = max(d_i - c_j[i]^2, 0), d_p = 0;  trace_j = sum_i d_i
    L[j][t] = c_t[p_j] (t < j), L[j][j] = sqrt(d_p at step j)

r^2 = sum_d ((x_i - x_p)_d / l_d)^2 from differences of rows (exact in either precision for the test data), Matern52 with
r = sqrt(r^2 + 1e-12) as the library's kern_val.

Margin.  Step j's margin is (largest - second largest d among the rows not yet chosen) / v, where rows bit-identical to the winner
count as the winner (they carry its d bit for bit on the device and lose the tie to it by index), and never more than
|largest - threshold| / v, which pins the stop decision the same way (at a stop it is that alone: which row held the largest d no
longer matters).  Step 0 has no gap (inf): every row starts from the same d, or
`first` names the row.  While every margin stays above a few thousand roundings (tests/greedy_cases.MARGIN), any evaluation that sums
in a different but fixed order picks the same rows."""
import numpy as np

LD = np.longdouble


def kernel_column(X, p, kind, v, ls):
    """k(x_i, x_p) for every row i, in X's dtype (no White part: it lives on the diagonal only)"""
    dt = X.dtype.type
    e = (X - X[p]) / ls
    r2 = (e * e).sum(1)
    if kind == "rbf":
        return dt(v) * np.exp(dt(-0.5) * r2)
    s5 = np.sqrt(dt(5))
    r = np.sqrt(r2 + dt(1e-12))
    return dt(v) * (dt(1) + s5 * r + dt(5) / dt(3) * (r * r)) * np.exp(-s5 * r)


def kernel_matrix(Z, kind, v, ls, white=0.0):
    """k(Z, Z) + white I in Z's dtype, the diagonal being what kern.Kdiag gives: v + white exactly (the Matern52 formula at r^2 = 0
    sits 8e-13 v below it, its r = sqrt(r^2 + 1e-12) being 1e-6 there)"""
    K = np.stack([kernel_column(Z, p, kind, v, ls) for p in range(Z.shape[0])], 1)
    np.fill_diagonal(K, Z.dtype.type(v) + Z.dtype.type(white))
    return K


def greedy(X, M, kind, v, ls, white=0.0, first=None, threshold=0.0, dtype=LD):
    """-> dict(indices (m,), m, residual (m,), trace (m,), L (m, m), margin: the smallest step margin, margins: per step incl. a stop)"""
    X64 = np.asarray(X, dtype=np.float64)
    Xw = X64.astype(dtype)
    ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (X64.shape[1],)).astype(dtype)
    n = X64.shape[0]
    dt = Xw.dtype.type
    d = np.full(n, dt(v) + dt(white), dtype=dtype)
    free = np.ones(n, dtype=bool)
    C = np.zeros((M, n), dtype=dtype)
    idx, res, trace, margins = [], [], [], []
    for j in range(M):
        cand = np.where(free, d, dt(-np.inf))
        if j == 0 and first is not None:
            p = int(first)
        else:
            p = int(np.argmax(cand))
        if j == 0 or not d[p] > dt(threshold):      # a stop: which row held the largest d no longer matters
            margin = np.inf
        else:
            same = (X64 == X64[p]).all(1)
            rest = cand[~same]
            margin = float((cand[p] - rest.max()) / dt(v)) if rest.size else np.inf
        margin = min(margin, float(abs(d[p] - dt(threshold)) / dt(v)))
        margins.append(margin)
        if not d[p] > dt(threshold):
            break
        r = d[p]
        sq = np.sqrt(r)
        k = kernel_column(Xw, p, kind, v, ls)
        c = (k - (C[:j, p] @ C[:j] if j else dt(0))) / sq
        C[j] = c
        d = np.maximum(d - c * c, dt(0))
        d[p] = dt(0)
        free[p] = False
        idx.append(p)
        res.append(r)
        trace.append(d.sum())
    m = len(idx)
    L = np.zeros((m, m), dtype=dtype)
    for j in range(m):
        L[j, :j] = C[:j, idx[j]]
        L[j, j] = np.sqrt(res[j])
    return dict(indices=np.array(idx, dtype=np.int32), m=m, residual=np.array(res, dtype=dtype), trace=np.array(trace, dtype=dtype), L=L,
                margin=min(margins), margins=margins)
