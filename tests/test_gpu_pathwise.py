"""-m gpu: the two C-ABI calls of the pathwise function draws (csrc/pathwise.hip; dsdgp_pathwise_eval, dsdgp_pathwise_weights) against
tests/pathwise_reference.py on the cases of tests/pathwise_cases.py.

Bars, by the project's rule (tests/test_gpu_psi.py): the truth is long double; e64 is the distance of the same operation sequence in
float64 numpy from it, entry by entry; mag is the sum of the magnitudes of the terms added into the entry, each sine / cosine term
weighted by 1 + sum_d |x_d - c_d| |Omega_dj|.  Every entry of the device is within 8 max(e64, 2^-50 mag) of the truth.  The switch of the
argument reduction is at |theta| = 4096: `theta_lo` lies below it, `theta_hi` on both sides.  A second call gives the same bits, a row
sub-range and a single draw give the full call's bits, nothing outside out[:, :DO] is written, a refused call launches nothing, and a Ku
that is not positive definite gives dsdgp_potrf's status and writes nothing.  DSDGP_PATHWISE_PROFILE=<file> writes the measured ratio of
every case, 1 = at the bar (profiles/pathwise_errors.md)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import pathwise_cases as PC
from tests import pathwise_reference as PR

pytestmark = pytest.mark.gpu

BAD_ARG, NOT_SPD, UNSUPPORTED = -1, -2, -4
CANARY = -12345.25
GUARD = 16
PAD = 3                                      # ld_out = DO + PAD: canaries between the rows too
_ROWS = []
_KIND = {"rbf": 0, "matern52": 1, "unknown": 7}      # 7: a kernel kind without a spectral density here


@pytest.fixture(scope="module")
def ctx():
    from doubly_stochastic_dgp.engine import Context
    return Context.get()


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("DSDGP_PATHWISE_PROFILE")
    if not path or not _ROWS:
        return
    with open(path, "w") as f:
        f.write("# Pathwise function draws: measured errors of the two C-ABI calls (tests/test_gpu_pathwise.py)\n\n"
                "Every figure is a ratio to its bar, 1 = at the bar: the worst over the entries of |device - truth| over\n"
                "8 max(e64, 2^-50 mag), e64 the distance of the float64 numpy sequence from the long-double truth at that entry, mag the sum\n"
                "of the magnitudes of the terms added into it (sine / cosine terms weighted by 1 + sum_d |x_d - c_d| |Omega_dj|).\n"
                "`-`: the case has no inducing rows, so no weights call.\n\n"
                "| case | kernel | n | L | D | M | DO | S | eval | weights |\n|" + "---|" * 10 + "\n")
        for r in _ROWS:
            f.write("| %s | %s | %d | %d | %d | %d | %d | %d | %s |\n" % (r[:8] + (" | ".join("-" if x is None else "%.3g" % x for x in r[8:]),)))


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _spec(c):
    from doubly_stochastic_dgp import _lib
    ls = np.ascontiguousarray(c["ls"], dtype=np.float64)
    spec = _lib.KernelSpec(kind=_KIND[c["kind"]], input_dim=c["D"], ard=int(c["ard"]), has_white=int(c["white_var"] is not None),
                           variance=c["variance"], white_variance=c["white_var"] or 0.0, lengthscales=ls.ctypes.data_as(_lib.c_double_p))
    return spec, ls


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _eval(ctx, c, V, rows=None, draw=None, n_arg=None, L_arg=None, ld_out=None):
    """dsdgp_pathwise_eval on the case: (rc, out (S', n', DO), the whole guarded buffer).  rows = (i0, i1): that sub-range of the rows of
    draw `draw`; n_arg, L_arg, ld_out: overrides for the refusal tests"""
    n, L, D, M, DO, S = (c[k] for k in ("n", "L", "D", "M", "DO", "S"))
    spec, ls = _spec(c)
    X = np.asarray(c["X"])
    addv = None if c["addv"] is None else np.asarray(c["addv"])
    Wc, Ws = c["Wc"], c["Ws"]
    if rows is not None:
        i0, i1 = rows
        X = X[draw, i0:i1] if X.ndim == 3 else X[i0:i1]
        if addv is not None:
            addv = addv[draw, i0:i1] if addv.ndim == 3 else addv[i0:i1]
        Wc, Ws, V = Wc[draw:draw + 1], Ws[draw:draw + 1], None if V is None else V[draw:draw + 1]
        n, S = i1 - i0, 1
    per_draw = X.ndim == 3
    Xd = ctx.to_device(X)
    if c["add"] == "identity":
        add, ld_add, add_stride = Xd, D, n * D if per_draw else 0
    elif c["add"] == "linear":
        add = ctx.to_device(addv)
        ld_add, add_stride = DO, n * DO if per_draw else 0
    else:
        add, ld_add, add_stride = None, 0, 0
    Om, org, Wcd, Wsd = (ctx.to_device(a) for a in (c["Omega"], c["origin"], Wc, Ws))
    Zd, Vd = (ctx.to_device(c["Z"]), ctx.to_device(V)) if M > 0 else (None, None)
    ld = DO + PAD if ld_out is None else ld_out
    buf = ctx.empty(2 * GUARD + S * n * max(ld, DO)).fill_(CANARY)
    rc = ctx.lib.dsdgp_pathwise_eval(ctx.handle, C.byref(spec), _p(Xd), n if n_arg is None else n_arg, n * D if per_draw else 0, S, _p(Om),
                                     _p(org), L if L_arg is None else L_arg, _p(Wcd), _p(Wsd), _p(Zd), M, _p(Vd), DO, _p(add), ld_add,
                                     add_stride, _p(buf[GUARD:]), ld)
    ctx.sync()
    host = buf.cpu().numpy()
    out = host[GUARD:GUARD + S * n * ld].reshape(S, n, ld)[:, :, :DO].copy() if ld >= DO else None
    return rc, out, host


def _canaries_intact(host, S, n, DO, ld):
    body = host[GUARD:GUARD + S * n * ld].reshape(S * n, ld)
    return np.all(host[:GUARD] == CANARY) and np.all(host[GUARD + S * n * ld:] == CANARY) and np.all(body[:, DO:] == CANARY)


def _weights(ctx, c, jitter=None, scratch_bytes=None):
    L, D, M, DO, S = (c[k] for k in ("L", "D", "M", "DO", "S"))
    spec, ls = _spec(c)
    Zd, Om, org, Wc, Ws, q_mu, eps = (ctx.to_device(c[k]) for k in ("Z", "Omega", "origin", "Wc", "Ws", "q_mu", "eps"))
    q_sqrt = None if c["q_sqrt"] is None else ctx.to_device(c["q_sqrt"])
    need = C.c_int64()
    assert ctx.lib.dsdgp_pathwise_scratch_bytes(M, D, DO, S, C.byref(need)) == 0
    scr = ctx.empty(need.value // 8 + 32)
    buf = ctx.empty(2 * GUARD + S * M * DO).fill_(CANARY)
    info = C.c_int(-7)
    rc = ctx.lib.dsdgp_pathwise_weights(ctx.handle, C.byref(spec), _p(Zd), M, _p(Om), _p(org), L, _p(Wc), _p(Ws), S, _p(q_mu), _p(q_sqrt),
                                        _p(None if q_sqrt is None else eps), DO, int(c["white"]), c["jitter"] if jitter is None else jitter,
                                        _p(scr), need.value if scratch_bytes is None else scratch_bytes, _p(buf[GUARD:]), C.byref(info))
    ctx.sync()
    host = buf.cpu().numpy()
    return rc, host[GUARD:-GUARD].reshape(S, M, DO).copy(), host, info.value


@pytest.mark.parametrize("name", PC.NAMES)
def test_cases_match_the_truth(ctx, name):
    c = PC.inputs(name)
    n, DO, S = c["n"], c["DO"], c["S"]
    V = PC.eval_weights(name)
    (tr, mag), (tw, _) = PC.evaluate(name), PC.evaluate(name, np.float64)
    rc, out, host = _eval(ctx, c, V)
    assert rc == 0, ctx.lib.dsdgp_last_error()
    assert _canaries_intact(host, S, n, DO, DO + PAD)
    keep = np.ones(n, dtype=bool)
    if "nan" in c["flags"]:                  # a NaN row gives NaN in that row's outputs only
        assert np.all(np.isnan(out[:, PC.NAN_ROW]))
        keep[PC.NAN_ROW] = False
    assert np.all(np.isfinite(out[:, keep]))
    if "far" in c["flags"]:                  # every exponential of the far row underflows: the row is its prior part
        f0, _ = PR.evaluate(c["kind"], c["X"], c["Omega"], c["origin"], c["Wc"], c["Ws"], c["Z"], None, c["variance"], c["ls"], c["addv"])
        assert np.all(tr[:, PC.FAR_ROW] == f0[:, PC.FAR_ROW])
    fig = PR.ratio(out[:, keep], tr[:, keep], tw[:, keep], mag[:, keep])
    rc2, again, _ = _eval(ctx, c, V)
    assert rc2 == 0 and _same_bits(again[:, keep], out[:, keep])
    wfig = None
    if c["M"] > 0:
        (vtr, vmag), (vtw, _) = PC.weights(name), PC.weights(name, np.float64)
        rc, v, vhost, info = _weights(ctx, c)
        assert rc == 0 and info == 0, ctx.lib.dsdgp_last_error()
        assert np.all(vhost[:GUARD] == CANARY) and np.all(vhost[-GUARD:] == CANARY) and np.all(np.isfinite(v))
        wfig = PR.ratio(v, vtr, vtw, vmag)
        assert _same_bits(_weights(ctx, c)[1], v)
    print("%s (%s, n = %d, L = %d, D = %d, M = %d, DO = %d, S = %d): eval %.3g, weights %s (x bar)"
          % (name, c["kind"], n, c["L"], c["D"], c["M"], DO, S, fig, "-" if wfig is None else "%.3g" % wfig))
    _ROWS.append((name, c["kind"], n, c["L"], c["D"], c["M"], DO, S, fig, wfig))
    assert fig <= 1.0, fig
    assert wfig is None or wfig <= 1.0, wfig


@pytest.mark.parametrize("name", ("n65", "d33", "n17", "theta_hi"))
def test_a_row_sub_range_of_one_draw_has_the_bits_of_the_full_call(ctx, name):
    c = PC.inputs(name)
    V = PC.eval_weights(name)
    rc, full, _ = _eval(ctx, c, V)
    assert rc == 0
    n = c["n"]
    for draw in range(c["S"]):
        for i0, i1 in ((0, n), (1, n), (n - 1, n), (n // 3, n // 3 + 5)):
            rc, part, host = _eval(ctx, c, V, rows=(i0, i1), draw=draw)
            assert rc == 0 and _canaries_intact(host, 1, i1 - i0, c["DO"], c["DO"] + PAD)
            assert _same_bits(part[0], full[draw, i0:i1]), (draw, i0, i1)


def test_refused_calls_launch_nothing_and_write_nothing(ctx):
    c = PC.inputs("n17")
    V = PC.eval_weights("n17")
    launches = ctx.lib.dsdgp_launch_count()
    for kw, want in ((dict(n_arg=0), BAD_ARG), (dict(L_arg=0), BAD_ARG), (dict(ld_out=c["DO"] - 1), BAD_ARG), (dict(L_arg=65537), UNSUPPORTED),
                     (dict(n_arg=c["n"] + 1), BAD_ARG)):            # n + 1: x_stride is neither 0 nor n D
        rc, _, host = _eval(ctx, c, V, **kw)
        assert rc == want, (kw, rc)
        assert np.all(host == CANARY), kw
    rc, _, host = _eval(ctx, dict(c, kind="unknown"), V)
    assert rc == UNSUPPORTED and np.all(host == CANARY)
    rc, _, vhost, _ = _weights(ctx, c, scratch_bytes=1024)          # a scratch block that is too small
    assert rc == BAD_ARG and np.all(vhost == CANARY)
    need = C.c_int64()
    assert ctx.lib.dsdgp_pathwise_scratch_bytes(0, 2, 1, 1, C.byref(need)) == BAD_ARG
    assert ctx.lib.dsdgp_pathwise_scratch_bytes(2049, 2, 1, 1, C.byref(need)) == BAD_ARG
    assert ctx.lib.dsdgp_launch_count() == launches


def test_a_ku_that_is_not_positive_definite_gives_the_potrf_status_and_writes_nothing(ctx):
    c = PC.inputs("n16")
    rc, _, vhost, info = _weights(ctx, c, jitter=-10.0)             # K(Z, Z) - 10 I
    assert rc == NOT_SPD and info > 0 and np.all(vhost == CANARY)
    rc, _, _, info = _weights(ctx, c)
    assert rc == 0 and info == 0
