"""-m gpu: the sparse conditional without q_sqrt and its reverse pass on the device (csrc/sparse_cond.hip; dsdgp_sparse_conditional,
dsdgp_sparse_conditional_grad) against tests/sparse_cond_reference.py on the cases of tests/sparse_cond_cases.py.

Bars, by the project's rule (tests/test_gpu_psi.py): the truth is long double; e64 is the distance of the same operation sequence in
float64 numpy from it, entry by entry; mag is the sum of the magnitudes of the terms added into the entry.  Every entry of every output of
the device is within 8 max(e64, 2^-50 mag) of the truth.  A second call gives the same bits, any subset of the outputs has the bits it
has when all are asked for, nothing outside the outputs is written, a refused call launches nothing, and a Ku that is not positive
definite gives dsdgp_potrf's status and writes nothing.  DSDGP_SPARSE_COND_PROFILE=<file> writes the measured ratio of every case, 1 = at
the bar (profiles/sparse_cond_errors.md)."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from tests import sparse_cond_cases as SC
from tests import sparse_cond_reference as SR

pytestmark = pytest.mark.gpu

BAD_ARG, NOT_SPD, UNSUPPORTED = -1, -2, -4
CANARY = -12345.25
GUARD = 16
_ROWS = []


@pytest.fixture(scope="module")
def ctx():
    from doubly_stochastic_dgp.engine import Context
    return Context.get()


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("DSDGP_SPARSE_COND_PROFILE")
    if not path or not _ROWS:
        return
    keys = SR.KEYS_FWD + SR.KEYS_REV
    with open(path, "w") as f:
        f.write("# Sparse conditional without q_sqrt and its reverse pass: measured errors (tests/test_gpu_sparse_cond.py)\n\n"
                "Every figure is a ratio to its bar, 1 = at the bar: the worst over the entries of an output of |device - truth| over\n"
                "8 max(e64, 2^-50 mag), e64 the distance of the float64 numpy sequence from the long-double truth at that entry, mag the sum\n"
                "of the magnitudes of the terms added into it.  `-`: the kernel has no White part (the entry is the jitter's gradient).\n\n"
                "| case | kernel | white | n | M | D | DO | " + " | ".join(keys) + " |\n|" + "---|" * (7 + len(keys)) + "\n")
        for r in _ROWS:
            f.write("| %s | %s | %s | %d | %d | %d | %d | %s |\n" % (r[:7] + (" | ".join("-" if x is None else "%.3g" % x for x in r[7:]),)))


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _spec(c):
    from doubly_stochastic_dgp import _lib
    ls = np.ascontiguousarray(c["ls"], dtype=np.float64)
    spec = _lib.KernelSpec(kind=c["kind"], input_dim=c["D"], ard=int(c["ard"]), has_white=int(c["white_var"] is not None),
                           variance=c["variance"], white_variance=c["white_var"] or 0.0, lengthscales=ls.ctypes.data_as(_lib.c_double_p))
    return spec, ls


def _scratch(ctx, c, reverse):
    need = C.c_int64()
    assert ctx.lib.dsdgp_sparse_conditional_scratch_bytes(c["n"], c["M"], c["D"], c["DO"], int(reverse), C.byref(need)) == 0
    return ctx.empty(need.value // 8 + 32), need.value


def _guarded(ctx, sizes, want):
    bufs = {k: ctx.empty(2 * GUARD + sizes[k]).fill_(CANARY) for k in sizes if k in want}
    return bufs, {k: (bufs[k][GUARD:-GUARD] if k in bufs else None) for k in sizes}


def _forward(ctx, c, want=("mean", "var"), jitter=None):
    n, M, DO = c["n"], c["M"], c["DO"]
    spec, ls = _spec(c)
    Z, X, q = (ctx.to_device(c[k]) for k in ("Z", "X", "q_mu"))
    scr, nbytes = _scratch(ctx, c, False)
    bufs, o = _guarded(ctx, dict(mean=n * DO, var=n), want)
    info = C.c_int(-7)
    rc = ctx.lib.dsdgp_sparse_conditional(ctx.handle, C.byref(spec), _p(Z), M, _p(X), n, _p(q), DO, int(c["white"]),
                                          c["jitter"] if jitter is None else jitter, _p(scr), nbytes, _p(o["mean"]), _p(o["var"]), C.byref(info))
    ctx.sync()
    out = {k: o[k].cpu().numpy().reshape((n, DO) if k == "mean" else (n,)) for k in want}
    return rc, out, {k: b.cpu().numpy() for k, b in bufs.items()}, info.value


def _reverse(ctx, c, want=("q_mu", "Z", "X", "kern"), jitter=None, scratch_bytes=None):
    n, M, D, DO = c["n"], c["M"], c["D"], c["DO"]
    nls = D if c["ard"] else 1
    spec, ls = _spec(c)
    Z, X, q, gm, gv = (ctx.to_device(c[k]) for k in ("Z", "X", "q_mu", "gm", "gv"))
    if D <= 32:
        scr, nbytes = _scratch(ctx, c, True)
    else:
        scr, nbytes = ctx.empty(64), 512            # a refused call reads no scratch
    bufs, o = _guarded(ctx, dict(q_mu=M * DO, Z=M * D, X=n * D, kern=2 + nls), want)
    info = C.c_int(-7)
    rc = ctx.lib.dsdgp_sparse_conditional_grad(ctx.handle, C.byref(spec), _p(Z), M, _p(X), n, _p(q), DO, int(c["white"]),
                                               c["jitter"] if jitter is None else jitter, _p(gm), _p(gv), _p(scr),
                                               nbytes if scratch_bytes is None else scratch_bytes, _p(o["q_mu"]), _p(o["Z"]), _p(o["X"]),
                                               _p(o["kern"]), C.byref(info))
    ctx.sync()
    out = {}
    for k, shape in (("q_mu", (M, DO)), ("Z", (M, D)), ("X", (n, D))):
        if k in want:
            out[k] = o[k].cpu().numpy().reshape(shape)
    if "kern" in want:
        k = o["kern"].cpu().numpy()
        out["variance"], out["lengthscales"], out["diag"] = k[:1].copy(), k[1:1 + nls].copy(), k[1 + nls:].copy()
    return rc, out, {k: b.cpu().numpy() for k, b in bufs.items()}, info.value


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


def _guards_intact(bufs):
    return all(np.all(b[:GUARD] == CANARY) and np.all(b[-GUARD:] == CANARY) for b in bufs.values())


@pytest.mark.parametrize("name", SC.NAMES)
def test_cases_match_the_truth(ctx, name):
    c = SC.inputs(name)
    (ftr, fmag), (f64, _) = SC.forward(name), SC.forward(name, np.float64)
    (rtr, rmag), (r64, _) = SC.reverse(name), SC.reverse(name, np.float64)
    rc, fwd, bufs, info = _forward(ctx, c)
    assert rc == 0 and info == 0, ctx.lib.dsdgp_last_error()
    assert _guards_intact(bufs)
    rc, rev, bufs, info = _reverse(ctx, c)
    assert rc == 0 and info == 0, ctx.lib.dsdgp_last_error()
    assert _guards_intact(bufs)
    got = dict(fwd, **rev)
    assert all(np.all(np.isfinite(v)) for v in got.values())
    assert got["lengthscales"].shape == ((c["D"],) if c["ard"] else (1,))
    if "far" in c["flags"]:                    # every exponential of the far row underflows: its mean and its input gradient are +0
        assert np.all(got["mean"][SC.FAR_ROW] == 0.0) and np.all(got["X"][SC.FAR_ROW] == 0.0)
        assert got["var"][SC.FAR_ROW] == c["variance"]
    # a second call: the same bits
    again = dict(_forward(ctx, c)[1], **_reverse(ctx, c)[1])
    for k in got:
        assert _same_bits(again[k], got[k]), k
    tr, mag, f = dict(ftr, **rtr), dict(fmag, **rmag), dict(f64, **r64)
    keys = SR.KEYS_FWD + SR.KEYS_REV
    figs = [_ratio(got[k], tr[k], f[k], mag[k]) for k in keys]
    row = (name, "rbf" if c["kind"] == SC.RBF else "matern52", str(c["white"]), c["n"], c["M"], c["D"], c["DO"]) + tuple(figs)
    print("%s (%s, white = %s, n = %d, M = %d, D = %d, DO = %d): " % row[:7] + ", ".join("%s %.3g" % kv for kv in zip(keys, figs))
          + " (x bar)")
    _ROWS.append(row)
    for k, fig in zip(keys, figs):
        assert fig <= 1.0, (k, fig)


@pytest.mark.parametrize("name", ("n129", "m65", "do65"))
def test_any_subset_of_the_outputs_has_the_bits_of_the_full_call(ctx, name):
    c = SC.inputs(name)
    full = dict(_forward(ctx, c)[1], **_reverse(ctx, c)[1])
    for want in (("mean",), ("var",)):
        rc, part, bufs, _ = _forward(ctx, c, want=want)
        assert rc == 0 and set(part) == set(want) and _guards_intact(bufs)
        assert all(_same_bits(part[k], full[k]) for k in part), want
    outs = ("q_mu", "Z", "X", "kern")
    for r in (1, 2, 3):
        for want in itertools.combinations(outs, r):
            rc, part, bufs, _ = _reverse(ctx, c, want=want)
            assert rc == 0 and _guards_intact(bufs)
            assert all(_same_bits(part[k], full[k]) for k in part), want


def test_the_forward_takes_a_wide_input_and_the_reverse_refuses_it(ctx):
    c = SC.inputs(SC.FORWARD_ONLY)
    args = (c["kind"], c["Z"], c["X"], c["q_mu"], c["variance"], c["ls"], c["white_var"], c["jitter"], c["white"])
    (tr, mag), (f64, _) = SR.forward(*args), SR.forward(*args, dtype=np.float64)
    rc, fwd, bufs, info = _forward(ctx, c)
    assert rc == 0 and info == 0 and _guards_intact(bufs)
    for k in SR.KEYS_FWD:
        fig = _ratio(fwd[k], tr[k], f64[k], mag[k])
        print("%s %s: %.3g (x bar)" % (SC.FORWARD_ONLY, k, fig))
        assert fig <= 1.0, (k, fig)
    launches = ctx.lib.dsdgp_launch_count()
    rc, out, bufs, _ = _reverse(ctx, c)
    assert rc == UNSUPPORTED and b"input_dim" in ctx.lib.dsdgp_last_error()
    assert ctx.lib.dsdgp_launch_count() == launches                    # a refused call launches nothing
    assert all(np.all(b == CANARY) for b in bufs.values())


def test_bad_arguments_launch_nothing(ctx):
    c = SC.inputs("n65")
    launches = ctx.lib.dsdgp_launch_count()
    rc, _, bufs, _ = _reverse(ctx, c, scratch_bytes=1024)               # a scratch block that is too small
    assert rc == BAD_ARG and all(np.all(b == CANARY) for b in bufs.values())
    need = C.c_int64()
    assert ctx.lib.dsdgp_sparse_conditional_scratch_bytes(0, 5, 2, 1, 0, C.byref(need)) == BAD_ARG
    assert ctx.lib.dsdgp_sparse_conditional_scratch_bytes(10, 2049, 2, 1, 0, C.byref(need)) == BAD_ARG
    assert ctx.lib.dsdgp_launch_count() == launches
    # more than 8 GB of scratch: unsupported, as the sibling calls
    spec, ls = _spec(c)
    t = ctx.empty(64)
    rc = ctx.lib.dsdgp_sparse_conditional(ctx.handle, C.byref(spec), _p(t), 2048, _p(t), 2 ** 20, _p(t), 1, 1, 0.1, _p(t), 512, _p(t), _p(t),
                                          None)
    assert rc == UNSUPPORTED and ctx.lib.dsdgp_launch_count() == launches


def test_a_ku_that_is_not_positive_definite_gives_the_potrf_status_and_writes_nothing(ctx):
    c = SC.inputs("n65")
    rc, _, bufs, info = _forward(ctx, c, jitter=-10.0)                  # K(Z, Z) - 10 I
    assert rc == NOT_SPD and info > 0 and all(np.all(b == CANARY) for b in bufs.values())
    rc, _, bufs, info2 = _reverse(ctx, c, jitter=-10.0)
    assert rc == NOT_SPD and info2 == info and all(np.all(b == CANARY) for b in bufs.values())
    rc, _, _, info = _forward(ctx, c)
    assert rc == 0 and info == 0


def test_the_context_methods_give_the_raw_calls_bits(ctx):
    c = SC.inputs("n129")
    raw = dict(_forward(ctx, c)[1], **_reverse(ctx, c)[1])
    spec, ls = _spec(c)
    Z, X, q, gm, gv = (ctx.to_device(c[k]) for k in ("Z", "X", "q_mu", "gm", "gv"))
    n, M, D, DO = c["n"], c["M"], c["D"], c["DO"]
    mean, var = ctx.empty(n, DO), ctx.empty(n)
    ctx.sparse_conditional(spec, Z, X, q, c["white"], c["jitter"], mean, var)
    dq, dZ, dX, dk = ctx.empty(M, DO), ctx.empty(M, D), ctx.empty(n, D), ctx.empty(2 + (D if c["ard"] else 1))
    ctx.sparse_conditional_grad(spec, Z, X, q, c["white"], c["jitter"], gm, gv, dq, dZ, dX, dk)
    ctx.sync()
    for k, t in (("mean", mean), ("var", var), ("q_mu", dq), ("Z", dZ), ("X", dX)):
        assert _same_bits(t.cpu().numpy(), raw[k]), k
    assert _same_bits(dk.cpu().numpy(), np.concatenate([raw["variance"], raw["lengthscales"], raw["diag"]]))
