"""-m gpu: the reverse pass of the kernel expectations on the device (csrc/psi_grad.hip; dsdgp_rbf_expectations_grad,
layers.kernel_expectations_grad) against tests/psi_grad_reference.py on the cases of tests/psi_grad_cases.py.

Bars, by the project's rule (tests/test_gpu_psi.py): the truth is the direct form in long double; e64 is the distance of the same
operation sequence in float64 from it, entry by entry; mag is the sum of the magnitudes of the terms added into the entry.  Every entry of
every output of the device is within 8 max(e64, 2^-50 mag) of the truth.  A second call and a call through
layers.kernel_expectations_grad on device tensors give the same bits, nothing outside the outputs is written, and the padding columns
of g_psi1 / g_psi2 are not read into the result.  DSDGP_PSI_GRAD_PROFILE=<file> writes the measured ratio of every case, 1 = at the bar
(profiles/psi_grad_errors.md)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import psi_grad_cases as GC

pytestmark = pytest.mark.gpu

BAD_ARG, UNSUPPORTED = -1, -4
CANARY = -12345.25
GUARD = 16
KEYS = ("X_mean", "X_var", "Z", "variance", "lengthscales")
_ROWS = []


@pytest.fixture(scope="module")
def ctx():
    from doubly_stochastic_dgp.engine import Context
    return Context.get()


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("DSDGP_PSI_GRAD_PROFILE")
    if not path or not _ROWS:
        return
    with open(path, "w") as f:
        f.write("# Reverse pass of the device kernel expectations: measured errors (tests/test_gpu_psi_grad.py)\n\n"
                "Every figure is a ratio to its bar, 1 = at the bar: the worst over the entries of an output of |device - truth| over\n"
                "8 max(e64, 2^-50 mag), e64 the distance of the float64 numpy sequence from the long-double truth at that entry, mag the sum\n"
                "of the magnitudes of the terms added into it.  NaN entries of the truth (negvar) are compared as a pattern, not here.\n\n"
                "| case | n | M | D | d_mu | d_s | d_Z | d_variance | d_lengthscales |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in _ROWS:
            f.write("| %s | %d | %d | %d | %.3g | %.3g | %.3g | %.3g | %.3g |\n" % r)


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _spec(c):
    from doubly_stochastic_dgp import _lib
    ls = np.ascontiguousarray(c["ls"], dtype=np.float64)
    spec = _lib.KernelSpec(kind=0, input_dim=c["mu"].shape[1], ard=int(c["ard"]), has_white=0, variance=c["variance"],
                           white_variance=0.1, lengthscales=ls.ctypes.data_as(_lib.c_double_p))
    return spec, ls


def _padded(ctx, a, pad):
    """`a` in a device buffer with `pad` extra columns holding the canary -> (the view of the buffer, its leading dimension)"""
    rows, cols = a.shape
    buf = ctx.empty(rows, cols + pad).fill_(CANARY)
    buf[:, :cols] = ctx.to_device(a)
    return buf, cols + pad


def _raw(ctx, c, pad1=3, pad2=5, use=("g1", "g2"), want=KEYS, s_zero=False):
    """dsdgp_rbf_expectations_grad into guarded buffers -> (rc, dict of the outputs asked for (numpy), dict of the whole buffers)"""
    n, D = c["mu"].shape
    M = c["Z"].shape[0]
    nls = D if c["ard"] else 1
    spec, ls = _spec(c)
    mu, Z = ctx.to_device(c["mu"]), ctx.to_device(c["Z"])
    s = None if c["s"] is None else ctx.to_device(c["s"])
    if s_zero:
        s = ctx.to_device(np.zeros((n, D)))
    g1, ld1 = _padded(ctx, c["g1"], pad1) if "g1" in use else (None, 0)
    g2, ld2 = _padded(ctx, c["g2"], pad2) if "g2" in use else (None, 0)
    sizes = dict(X_mean=n * D, X_var=n * D, Z=M * D, kern=1 + nls)
    need = dict(X_mean="X_mean" in want, X_var="X_var" in want, Z="Z" in want, kern="variance" in want or "lengthscales" in want)
    bufs = {k: ctx.empty(2 * GUARD + sizes[k]).fill_(CANARY) for k in sizes if need[k]}
    o = {k: (bufs[k][GUARD:-GUARD] if k in bufs else None) for k in sizes}
    rc = ctx.lib.dsdgp_rbf_expectations_grad(ctx.handle, C.byref(spec), _p(Z), M, _p(mu), _p(s), n, c["g0"], _p(g1), ld1, _p(g2), ld2,
                                             _p(o["X_mean"]), _p(o["X_var"]), _p(o["Z"]), _p(o["kern"]))
    ctx.sync()
    out = {}
    if need["X_mean"]:
        out["X_mean"] = o["X_mean"].cpu().numpy().reshape(n, D)
    if need["X_var"]:
        out["X_var"] = o["X_var"].cpu().numpy().reshape(n, D)
    if need["Z"]:
        out["Z"] = o["Z"].cpu().numpy().reshape(M, D)
    if need["kern"]:
        k = o["kern"].cpu().numpy()
        out["variance"], out["lengthscales"] = k[:1].copy(), k[1:].copy()
    return rc, out, {k: b.cpu().numpy() for k, b in bufs.items()}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _ratio(dev, tr, f64, mag, mask=None):
    """worst |device - truth| / (8 max(e64, 2^-50 mag)) over the entries (of `mask`)"""
    dev, tr, f64, mag = (np.atleast_1d(np.asarray(a)) for a in (dev, tr, f64, mag))
    mask = np.ones(tr.shape, dtype=bool) if mask is None else mask
    if not mask.any():
        return 0.0
    err = np.abs(dev - tr).astype(np.float64)[mask]
    e64 = np.abs(f64 - tr).astype(np.float64)[mask]
    bar = 8.0 * np.maximum(e64, 2.0 ** -50 * mag.astype(np.float64)[mask])
    if np.any((bar == 0.0) & (err != 0.0)) or np.any(np.isnan(err)):
        return float("inf")
    return float(np.max(err / np.where(bar == 0.0, 1.0, bar)))


@pytest.mark.parametrize("name", GC.NAMES)
def test_cases_match_the_truth(ctx, name):
    from doubly_stochastic_dgp.gpflow_compat import RBF
    from doubly_stochastic_dgp.layers import kernel_expectations_grad
    c, (tr, mag), f = GC.inputs(name), GC.truth(name), GC.float64(name)
    n, D = c["mu"].shape
    M = c["Z"].shape[0]
    rc, got, bufs = _raw(ctx, c)
    assert rc == 0, ctx.lib.dsdgp_last_error()
    for b in bufs.values():                                            # nothing outside the outputs
        assert np.all(b[:GUARD] == CANARY) and np.all(b[-GUARD:] == CANARY)
    assert got["lengthscales"].shape == ((D,) if c["ard"] else (1,))
    # the NaN pattern is the reference's: a row with l^2 + 2 s < 0 reaches its own rows of d_mu / d_s and every sum over rows
    for k in KEYS:
        assert np.array_equal(np.isnan(got[k]), np.isnan(np.atleast_1d(np.asarray(tr[k], dtype=np.float64)))), k
    if name in GC.NEGVAR:
        bad = GC.NEGVAR_ROW[name]
        nan_rows = np.zeros(n, dtype=bool)
        nan_rows[bad] = True
        assert np.array_equal(np.isnan(got["X_mean"]).all(axis=1), nan_rows) and np.array_equal(np.isnan(got["X_var"]).any(axis=1), nan_rows)
        assert np.isnan(got["Z"]).all() and np.isnan(got["variance"]).all() and np.isnan(got["lengthscales"]).all()
    if name == "far":                                                  # the far centre: +0 or finite, never NaN
        assert np.all(np.isfinite(got["Z"][0])) and all(np.all(np.isfinite(got[k])) for k in KEYS)
    # a second call (other paddings), and the host mirror on device tensors: the same bits
    rc, again, _ = _raw(ctx, c, pad1=0, pad2=1)
    assert rc == 0
    kern = RBF(D, variance=c["variance"], lengthscales=c["ls"] if c["ard"] else float(c["ls"][0]), ARD=c["ard"])
    host = kernel_expectations_grad(kern, ctx.to_device(c["Z"]), ctx.to_device(c["mu"]), None if c["s"] is None else ctx.to_device(c["s"]),
                                    c["g0"], ctx.to_device(c["g1"]), ctx.to_device(c["g2"]))
    for k in KEYS:
        assert _same_bits(again[k], got[k]), k
        assert _same_bits(np.atleast_1d(host[k]), got[k]), k
    # the bars
    figs = []
    for k in KEYS:
        ok = ~np.isnan(np.atleast_1d(np.asarray(tr[k], dtype=np.float64)))
        figs.append(_ratio(got[k], tr[k], f[k], mag[k], ok))
    row = (name, n, M, D) + tuple(figs)
    print("%s (n = %d, M = %d, D = %d): d_mu %.3g, d_s %.3g, d_Z %.3g, d_variance %.3g, d_lengthscales %.3g (x bar)" % row)
    _ROWS.append(row)
    for k, fig in zip(KEYS, figs):
        assert fig <= 1.0, (k, fig)


def test_null_variance_is_zero_variance(ctx):
    """s == NULL and s = 0: the same bits for every output; d_s at s == NULL is the derivative at s = 0"""
    rc0, zero, _ = _raw(ctx, GC.inputs("zero"))
    rc1, null, _ = _raw(ctx, GC.inputs("null"))
    assert rc0 == 0 and rc1 == 0
    for k in KEYS:
        assert _same_bits(zero[k], null[k]), k
    assert np.all(np.isfinite(null["X_var"])) and np.any(null["X_var"] != 0.0)


def test_adjoints_and_outputs_are_optional(ctx):
    c = GC.inputs("split")
    n, M = c["mu"].shape[0], c["Z"].shape[0]
    rc, full, _ = _raw(ctx, c)
    assert rc == 0
    # each output NULL alone: what remains has the same bits
    for drop in ("X_mean", "X_var", "Z", "variance"):
        want = tuple(k for k in KEYS if k != drop and not (drop == "variance" and k == "lengthscales"))
        rc, part, bufs = _raw(ctx, c, want=want)
        assert rc == 0 and set(part) == set(want)
        for k in want:
            assert _same_bits(part[k], full[k]), (drop, k)
    # each adjoint NULL alone: the bits of the same call given zeros in its place, and the truth of the part that remains
    from tests import psi_grad_reference as R
    for use, zeroed in ((("g2",), "g1"), (("g1",), "g2")):
        rc, part, _ = _raw(ctx, c, use=use)
        cz = dict(c)
        cz[zeroed] = np.zeros_like(c[zeroed])
        rcz, withzero, _ = _raw(ctx, cz)
        assert rc == 0 and rcz == 0
        a = list(GC.args(c))
        a[7 if zeroed == "g1" else 8] = None
        tr, mag = R.psi_grad(*a, dtype=R.LD)
        f = R.psi_grad(*a, dtype=np.float64)[0]
        for k in KEYS:
            assert _same_bits(part[k], withzero[k]), (zeroed, k)
            assert _ratio(part[k], tr[k], f[k], mag[k]) <= 1.0, (zeroed, k)


def test_unsupported_width_and_error_codes(ctx):
    from doubly_stochastic_dgp import _lib
    c = GC.inputs(GC.UNSUPPORTED)
    rc, out, bufs = _raw(ctx, c)
    assert rc == UNSUPPORTED and b"input_dim" in ctx.lib.dsdgp_last_error()
    for b in bufs.values():                                            # a refused call launches nothing
        assert np.all(b == CANARY)
    c = GC.inputs("n15")
    n, M = c["mu"].shape[0], c["Z"].shape[0]
    mu, Z, s, g1, g2 = (ctx.to_device(c[k]) for k in ("mu", "Z", "s", "g1", "g2"))
    o = ctx.empty(n * 4).fill_(CANARY)

    def call(spec, M_=M, n_=n, ld1=M, ld2=M, Zp=Z, mup=mu):
        rc = ctx.lib.dsdgp_rbf_expectations_grad(ctx.handle, C.byref(spec), _p(Zp), M_, _p(mup), _p(s), n_, 0.5, _p(g1), ld1, _p(g2), ld2,
                                                 _p(o), None, None, None)
        ctx.sync()
        return rc

    good, keep = _spec(c)
    for kind, white in ((1, 0), (0, 1)):                               # Matern52; RBF + White
        bad, keep2 = _spec(c)
        bad.kind, bad.has_white = kind, white
        assert call(bad) == UNSUPPORTED
    assert call(good, M_=0) == BAD_ARG and call(good, M_=2049) == BAD_ARG and call(good, n_=0) == BAD_ARG
    assert call(good, ld1=M - 1) == BAD_ARG and call(good, ld2=M - 1) == BAD_ARG
    assert call(good, Zp=None) == BAD_ARG and call(good, mup=None) == BAD_ARG
    assert np.all(o.cpu().numpy() == CANARY)
    assert call(good) == 0
