"""-m gpu: the reverse pass of the Gram matrix on the device (csrc/gram_grad.hip; dsdgp_gram_grad, layers.kernel_gram_grad) against
tests/gram_grad_reference.py on the cases of tests/gram_grad_cases.py.

Bars, by the project's rule (tests/test_gpu_psi.py): the truth is the direct form in long double; e64 is the distance of the same
operation sequence in float64 from it, entry by entry; mag is the sum of the magnitudes of the terms added into the entry.  Every entry of
every output of the device is within 8 max(e64, 2^-50 mag) of the truth.  A second call and a call through layers.kernel_gram_grad on
device tensors give the same bits, each output requested alone has the bits it has when all are requested, nothing outside the outputs
is written, and the padding columns of G are not read into the result.  DSDGP_GRAM_GRAD_PROFILE=<file> writes the measured ratio of
every case, 1 = at the bar (profiles/gram_grad_errors.md)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import gram_grad_cases as GC

pytestmark = pytest.mark.gpu

BAD_ARG, UNSUPPORTED = -1, -4
CANARY = -12345.25
GUARD = 16
KEYS = GC.KEYS
_ROWS = []


@pytest.fixture(scope="module")
def ctx():
    from doubly_stochastic_dgp.engine import Context
    return Context.get()


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("DSDGP_GRAM_GRAD_PROFILE")
    if not path or not _ROWS:
        return
    with open(path, "w") as f:
        f.write("# Reverse pass of the device Gram matrix: measured errors (tests/test_gpu_gram_grad.py)\n\n"
                "Every figure is a ratio to its bar, 1 = at the bar: the worst over the entries of an output of |device - truth| over\n"
                "8 max(e64, 2^-50 mag), e64 the distance of the float64 numpy sequence from the long-double truth at that entry, mag the sum\n"
                "of the magnitudes of the terms added into it.  `-`: the form has no such output.\n\n"
                "| case | kernel | form | n | n2 | D | d_X | d_X2 | d_variance | d_lengthscales | d_diag |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in _ROWS:
            f.write("| %s | %s | %s | %d | %d | %d | %s |\n" % (r[:6] + (" | ".join("-" if x is None else "%.3g" % x for x in r[6:]),)))


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _spec(c):
    from doubly_stochastic_dgp import _lib
    ls = np.ascontiguousarray(c["ls"], dtype=np.float64)
    spec = _lib.KernelSpec(kind=c["kind"], input_dim=c["X"].shape[1], ard=int(c["ard"]), has_white=int(c["white"] is not None),
                           variance=c["variance"], white_variance=c["white"] or 0.0, lengthscales=ls.ctypes.data_as(_lib.c_double_p))
    return spec, ls


def _raw(ctx, c, pad=3, want=KEYS):
    """dsdgp_gram_grad into guarded buffers, G with `pad` canary columns -> (rc, dict of the outputs asked for (numpy), the whole buffers)"""
    n, D = c["X"].shape
    n2 = n if c["sym"] else c["X2"].shape[0]
    nls = D if c["ard"] else 1
    spec, ls = _spec(c)
    X = ctx.to_device(c["X"])
    X2 = None if c["sym"] else ctx.to_device(c["X2"])
    G = ctx.empty(n, n2 + pad).fill_(CANARY)
    G[:, :n2] = ctx.to_device(c["G"])
    sizes = dict(X=n * D, X2=n2 * D, kern=2 + nls)
    need = dict(X="X" in want, X2="X2" in want and not c["sym"], kern=any(k in want for k in ("variance", "lengthscales", "diag")))
    bufs = {k: ctx.empty(2 * GUARD + sizes[k]).fill_(CANARY) for k in sizes if need[k]}
    o = {k: (bufs[k][GUARD:-GUARD] if k in bufs else None) for k in sizes}
    rc = ctx.lib.dsdgp_gram_grad(ctx.handle, C.byref(spec), _p(X), n, _p(X2), 0 if c["sym"] else n2, _p(G), n2 + pad, _p(o["X"]),
                                 _p(o["X2"]), _p(o["kern"]))
    ctx.sync()
    out = {}
    if need["X"]:
        out["X"] = o["X"].cpu().numpy().reshape(n, D)
    if need["X2"]:
        out["X2"] = o["X2"].cpu().numpy().reshape(n2, D)
    if need["kern"]:
        k = o["kern"].cpu().numpy()
        out["variance"], out["lengthscales"], out["diag"] = k[:1].copy(), k[1:1 + nls].copy(), k[1 + nls:].copy()
    return rc, out, {k: b.cpu().numpy() for k, b in bufs.items()}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _ratio(dev, tr, f64, mag):
    """worst |device - truth| / (8 max(e64, 2^-50 mag)) over the entries"""
    dev, tr, f64, mag = (np.atleast_1d(np.asarray(a)) for a in (dev, tr, f64, mag))
    err = np.abs(dev - tr).astype(np.float64)
    e64 = np.abs(f64 - tr).astype(np.float64)
    bar = 8.0 * np.maximum(e64, 2.0 ** -50 * mag.astype(np.float64))
    if np.any((bar == 0.0) & (err != 0.0)) or np.any(np.isnan(err)):
        return float("inf")
    return float(np.max(err / np.where(bar == 0.0, 1.0, bar)))


def _kernel(c):
    from doubly_stochastic_dgp.gpflow_compat import RBF, Matern52, White
    D = c["X"].shape[1]
    kern = (RBF if c["kind"] == GC.RBF else Matern52)(D, variance=c["variance"], lengthscales=c["ls"] if c["ard"] else float(c["ls"][0]),
                                                     ARD=c["ard"])
    return kern if c["white"] is None else kern + White(D, variance=c["white"])


@pytest.mark.parametrize("name", GC.NAMES)
def test_cases_match_the_truth(ctx, name):
    from doubly_stochastic_dgp.layers import kernel_gram_grad
    c, (tr, mag), f = GC.inputs(name), GC.truth(name), GC.float64(name)
    n, D = c["X"].shape
    n2 = n if c["sym"] else c["X2"].shape[0]
    keys = tuple(k for k in KEYS if tr[k] is not None)
    rc, got, bufs = _raw(ctx, c)
    assert rc == 0, ctx.lib.dsdgp_last_error()
    for b in bufs.values():                                            # nothing outside the outputs
        assert np.all(b[:GUARD] == CANARY) and np.all(b[-GUARD:] == CANARY)
    assert set(got) == set(keys) and got["lengthscales"].shape == ((D,) if c["ard"] else (1,))
    assert all(np.all(np.isfinite(got[k])) for k in keys)
    if not c["sym"]:
        assert got["diag"][0] == 0.0
    if name == "far_c":                                                # the far row: every pair underflows, +0 exactly
        assert np.all(got["X2"][4] == 0.0)
    if name == "far_s":
        assert np.all(got["X"][9] == 0.0)
    # a second call (another padding of G), and the host mirror on device tensors: the same bits
    rc, again, _ = _raw(ctx, c, pad=0)
    assert rc == 0
    host = kernel_gram_grad(_kernel(c), ctx.to_device(c["X"]), None if c["sym"] else ctx.to_device(c["X2"]), ctx.to_device(c["G"]))
    assert (host["X2"] is None) == c["sym"]
    for k in keys:
        assert _same_bits(again[k], got[k]), k
        assert _same_bits(np.atleast_1d(host[k]), got[k]), k
    # the bars
    figs = [_ratio(got[k], tr[k], f[k], mag[k]) if tr[k] is not None else None for k in KEYS]
    row = (name, "rbf" if c["kind"] == GC.RBF else "matern52", "symmetric" if c["sym"] else "cross", n, n2, D) + tuple(figs)
    print("%s (%s, %s, n = %d, n2 = %d, D = %d): " % row[:6] + ", ".join("%s %s" % (k, "-" if x is None else "%.3g" % x)
                                                                         for k, x in zip(KEYS, figs)) + " (x bar)")
    _ROWS.append(row)
    for k, fig in zip(KEYS, figs):
        assert fig is None or fig <= 1.0, (k, fig)


@pytest.mark.parametrize("name", ("x129", "rb129", "d32"))
def test_each_output_alone_has_the_bits_of_the_full_call(ctx, name):
    c = GC.inputs(name)
    rc, full, _ = _raw(ctx, c)
    assert rc == 0
    for want in (("X",), ("X2",), ("variance", "lengthscales", "diag")):
        if want == ("X2",) and c["sym"]:
            continue
        rc, part, bufs = _raw(ctx, c, want=want)
        assert rc == 0 and set(part) == set(want)
        for b in bufs.values():
            assert np.all(b[:GUARD] == CANARY) and np.all(b[-GUARD:] == CANARY)
        for k in want:
            assert _same_bits(part[k], full[k]), (want, k)


def test_symmetric_form_takes_the_two_halves_of_g_together(ctx):
    """a non-symmetric G and its transpose give the same gradients in the symmetric form (the sum G_ij + G_ji is commutative, so the
    same bits)"""
    c = GC.inputs("s33")
    assert not np.array_equal(c["G"], c["G"].T)
    base = _raw(ctx, c)[1]
    rc, got, _ = _raw(ctx, dict(c, G=c["G"].T.copy()))
    assert rc == 0
    for k in ("X", "variance", "lengthscales", "diag"):
        assert _same_bits(got[k], base[k]), k


def test_unsupported_width_and_error_codes(ctx):
    c = GC.inputs(GC.UNSUPPORTED)
    rc, out, bufs = _raw(ctx, c)
    assert rc == UNSUPPORTED and b"input_dim" in ctx.lib.dsdgp_last_error()
    for b in bufs.values():                                            # a refused call launches nothing
        assert np.all(b == CANARY)
    c = GC.inputs("c15")
    n, n2 = c["X"].shape[0], c["X2"].shape[0]
    X, X2, G = (ctx.to_device(c[k]) for k in ("X", "X2", "G"))
    o = ctx.empty(64 * 4).fill_(CANARY)

    def call(spec, n_=n, n2_=n2, ldg=n2, Xp=X, X2p=X2, Gp=G, dX2=None):
        rc = ctx.lib.dsdgp_gram_grad(ctx.handle, C.byref(spec), _p(Xp), n_, _p(X2p), n2_, _p(Gp), ldg, _p(o), _p(dX2), None)
        ctx.sync()
        return rc

    good, keep = _spec(c)
    bad, keep2 = _spec(c)
    bad.kind = 2
    assert call(bad) == BAD_ARG
    assert call(good, n_=0) == BAD_ARG and call(good, n2_=0) == BAD_ARG and call(good, n_=2 ** 31) == BAD_ARG
    assert call(good, ldg=n2 - 1) == BAD_ARG
    assert call(good, Xp=None) == BAD_ARG and call(good, Gp=None) == BAD_ARG
    Gs = ctx.to_device(np.zeros((n, n)))
    assert call(good, X2p=None, Gp=Gs, ldg=n, dX2=o) == BAD_ARG     # the symmetric form has no d_X2
    assert call(good, X2p=None, Gp=Gs, ldg=n - 1) == BAD_ARG
    assert np.all(o.cpu().numpy() == CANARY)
    assert call(good) == 0
