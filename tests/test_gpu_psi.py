"""-m gpu: the expectations of the RBF kernel under a Gaussian input on the device (csrc/psi.hip; dsdgp_rbf_expectations,
layers.kernel_expectations) against tests/psi_reference.py on the cases of tests/psi_cases.py.

Bars, by the project's rule (tests/test_gpu_greedy.py, tests/test_gpu_natgrad_direct.py): the truth is the direct form in long double;
e64 is the distance of the same operation sequence in float64 from it.  The device is within 8 max(e64, 2^-50) of the truth, in units
of v for psi1 and of N v^2 for psi2 (v = the kernel variance).  An entry of psi2 above 1e-3 of the largest one also meets a relative
bar: 8 max(the float64 sequence's relative error of that entry, (D + 8) 2^-52 (1 + absE)), absE = max_n of the sum of the magnitudes of
the terms of the entry's exponent — the exponent's rounding, amplified by exp.  psi0 is exact, psi2 bit-symmetric, a second call and a
call through layers.kernel_expectations on device tensors give the same bits, and nothing outside the M columns of the outputs is written.
DSDGP_PSI_PROFILE=<file> writes the measured ratio of every case, 1 = at the bar (profiles/psi_errors.md)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import psi_cases as PC

pytestmark = pytest.mark.gpu

BAD_ARG, UNSUPPORTED = -1, -4
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
    path = os.environ.get("DSDGP_PSI_PROFILE")
    if not path or not _ROWS:
        return
    with open(path, "w") as f:
        f.write("# Device kernel expectations: measured errors (tests/test_gpu_psi.py)\n\n"
                "Every figure is a ratio to its bar, 1 = at the bar.  `psi1`, `psi2`: the worst |device - truth| over 8 max(e64, 2^-50) in\n"
                "units of v and N v^2, e64 the distance of the float64 numpy sequence from the long-double truth.  `rel`: over the entries of\n"
                "psi2 above 1e-3 of the largest, the worst relative error over 8 max(the float64 sequence's, (D + 8) 2^-52 (1 + absE)).\n\n"
                "| case | n | M | D | psi1 | psi2 | rel |\n|---|---|---|---|---|---|---|\n")
        for r in _ROWS:
            f.write("| %s | %d | %d | %d | %.3g | %.3g | %.3g |\n" % r)


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _spec(c, kind=0, has_white=0):
    from doubly_stochastic_dgp import _lib
    ls = np.ascontiguousarray(c["ls"], dtype=np.float64)
    spec = _lib.KernelSpec(kind=kind, input_dim=c["mu"].shape[1], ard=int(c["ard"]), has_white=has_white, variance=c["variance"],
                           white_variance=0.1, lengthscales=ls.ctypes.data_as(_lib.c_double_p))
    return spec, ls


def _raw(ctx, c, pad1=3, pad2=5):
    """dsdgp_rbf_expectations into guarded buffers with padded leading dimensions -> (rc, psi0, psi1, psi2, the three whole buffers)"""
    n, M = c["mu"].shape[0], c["Z"].shape[0]
    ld1, ld2 = M + pad1, M + pad2
    spec, ls = _spec(c)
    mu, Z = ctx.to_device(c["mu"]), ctx.to_device(c["Z"])
    s = None if c["s"] is None else ctx.to_device(c["s"])
    b0 = ctx.empty(2 * GUARD + 1).fill_(CANARY)
    b1 = ctx.empty(2 * GUARD + n * ld1).fill_(CANARY)
    b2 = ctx.empty(2 * GUARD + M * ld2).fill_(CANARY)
    p0, p1, p2 = b0[GUARD:GUARD + 1], b1[GUARD:GUARD + n * ld1].view(n, ld1), b2[GUARD:GUARD + M * ld2].view(M, ld2)
    rc = ctx.lib.dsdgp_rbf_expectations(ctx.handle, C.byref(spec), _p(Z), M, _p(mu), _p(s), n, _p(p0), _p(p1), ld1, _p(p2), ld2)
    ctx.sync()
    return rc, p0.cpu().numpy(), p1.cpu().numpy(), p2.cpu().numpy(), (b0.cpu().numpy(), b1.cpu().numpy(), b2.cpu().numpy())


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("name", PC.NAMES)
def test_cases_match_the_truth(ctx, name):
    from doubly_stochastic_dgp.gpflow_compat import RBF
    from doubly_stochastic_dgp.layers import kernel_expectations
    c, tr, f = PC.inputs(name), PC.truth(name), PC.float64(name)
    n, D = c["mu"].shape
    M, v = c["Z"].shape[0], c["variance"]
    rc, p0, p1w, p2w, bufs = _raw(ctx, c)
    assert rc == 0, ctx.lib.dsdgp_last_error()
    p1, p2 = p1w[:, :M], p2w[:M, :M]
    # nothing outside the outputs: the guards around every buffer and the padding columns
    for b in bufs:
        assert np.all(b[:GUARD] == CANARY) and np.all(b[-GUARD:] == CANARY)
    assert np.all(p1w[:, M:] == CANARY) and np.all(p2w[:, M:] == CANARY)
    assert p0[0] == n * v
    assert _same_bits(p2, p2.T)
    nan1, nan2 = np.isnan(tr["psi1"]), np.isnan(tr["psi2"])
    assert np.array_equal(np.isnan(p1), nan1) and np.array_equal(np.isnan(p2), nan2)
    if name in PC.NEGVAR:
        assert nan2.all() and not nan1.any()
    if name == "far":
        assert np.all(p1[:, 0] == 0.0) and np.all(p2[0] == 0.0) and not np.any(np.signbit(p2[0])) and not np.any(np.signbit(p1[:, 0]))
    # a second call, and the host mirror on device tensors: the same bits
    rc, q0, q1w, q2w, _ = _raw(ctx, c, pad1=0, pad2=1)
    assert rc == 0 and _same_bits(q1w[:, :M], p1) and _same_bits(q2w[:M, :M], p2) and q0[0] == p0[0]
    kern = RBF(D, variance=v, lengthscales=c["ls"] if c["ard"] else float(c["ls"][0]), ARD=c["ard"])
    h0, h1, h2 = kernel_expectations(kern, ctx.to_device(c["Z"]), ctx.to_device(c["mu"]),
                                     None if c["s"] is None else ctx.to_device(c["s"]))
    assert h0 == p0[0] and _same_bits(h1, p1) and _same_bits(h2, p2)
    # the bars
    ok1, ok2 = ~nan1, ~nan2
    e1 = float(np.max(np.abs(f["psi1"] - tr["psi1"])[ok1], initial=0.0)) / v
    e2 = float(np.max(np.abs(f["psi2"] - tr["psi2"])[ok2], initial=0.0)) / (n * v * v)
    d1 = float(np.max(np.abs(p1 - tr["psi1"])[ok1], initial=0.0)) / v
    d2 = float(np.max(np.abs(p2 - tr["psi2"])[ok2], initial=0.0)) / (n * v * v)
    bar1, bar2 = 8.0 * max(e1, 2.0 ** -50), 8.0 * max(e2, 2.0 ** -50)
    t2 = tr["psi2"].astype(np.float64)
    big = ok2 & (t2 > 1e-3 * np.max(t2[ok2], initial=0.0))
    r_fig = 0.0
    if big.any():
        rel_dev = np.abs((p2 - tr["psi2"]) / tr["psi2"]).astype(np.float64)[big]
        rel_64 = np.abs((f["psi2"] - tr["psi2"]) / tr["psi2"]).astype(np.float64)[big]
        rbar = 8.0 * np.maximum(rel_64, (D + 8) * 2.0 ** -52 * (1.0 + tr["absE"][big]))
        r_fig = float(np.max(rel_dev / rbar))
    row = (name, n, M, D, d1 / bar1, d2 / bar2, r_fig)
    print("%s (n = %d, M = %d, D = %d): psi1 %.3g, psi2 %.3g, rel %.3g (x bar); e64 %.3g / %.3g" % (row + (e1, e2)))
    _ROWS.append(row)
    assert d1 <= bar1
    assert d2 <= bar2
    assert r_fig <= 1.0


def test_outputs_are_optional(ctx):
    c = PC.inputs("split")
    n, M = c["mu"].shape[0], c["Z"].shape[0]
    _, p0, p1w, p2w, _ = _raw(ctx, c, pad1=0, pad2=0)
    spec, ls = _spec(c)
    mu, Z, s = ctx.to_device(c["mu"]), ctx.to_device(c["Z"]), ctx.to_device(c["s"])
    a1, a2 = ctx.empty(n, M).fill_(CANARY), ctx.empty(M, M).fill_(CANARY)
    assert ctx.lib.dsdgp_rbf_expectations(ctx.handle, C.byref(spec), _p(Z), M, _p(mu), _p(s), n, None, _p(a1), M, None, 0) == 0
    assert ctx.lib.dsdgp_rbf_expectations(ctx.handle, C.byref(spec), _p(Z), M, _p(mu), _p(s), n, None, None, 0, _p(a2), M) == 0
    ctx.sync()
    assert _same_bits(a1.cpu().numpy(), p1w) and _same_bits(a2.cpu().numpy(), p2w)


def test_float32_and_strided_tensors_are_converted_not_reinterpreted(ctx):
    """n = 17, M = 5, D = 3: a float32 device tensor for X_mean and a transposed (non-contiguous) view for Z give the bits of the
    float64 contiguous copies of the same values, in the expectations and in their reverse pass."""
    import torch
    from doubly_stochastic_dgp.gpflow_compat import RBF
    from doubly_stochastic_dgp.layers import kernel_expectations, kernel_expectations_grad
    rng = np.random.default_rng(7)
    n, M, D = 17, 5, 3
    mu32 = ctx.to_device(rng.standard_normal((n, D))).to(torch.float32)
    Zt = ctx.to_device(rng.standard_normal((D, M))).t()
    s, g1, g2 = rng.uniform(0.0, 0.8, (n, D)), rng.standard_normal((n, M)), rng.standard_normal((M, M))
    assert mu32.dtype == torch.float32 and not Zt.is_contiguous() and tuple(Zt.shape) == (M, D)
    mu64, Zc = mu32.to(torch.float64), Zt.contiguous()
    kern = RBF(D, variance=1.7, lengthscales=np.array([0.9, 1.4, 2.0]), ARD=True)
    got, want = kernel_expectations(kern, Zt, mu32, s), kernel_expectations(kern, Zc, mu64, s)
    assert got[0] == want[0] and _same_bits(got[1], want[1]) and _same_bits(got[2], want[2])
    assert np.all(np.isfinite(want[1])) and np.all(want[2] > 0.0)
    got = kernel_expectations_grad(kern, Zt, mu32, s, -0.7, g1, g2)
    want = kernel_expectations_grad(kern, Zc, mu64, s, -0.7, g1, g2)
    for k in ("X_mean", "X_var", "Z", "lengthscales"):
        assert _same_bits(got[k], want[k]) and np.all(np.isfinite(want[k])) and np.any(want[k] != 0.0), k
    assert got["variance"] == want["variance"]


def test_error_codes(ctx):
    c = PC.inputs("n15")
    n, M = c["mu"].shape[0], c["Z"].shape[0]
    mu, Z, s = ctx.to_device(c["mu"]), ctx.to_device(c["Z"]), ctx.to_device(c["s"])
    o0, o1, o2 = ctx.empty(1).fill_(CANARY), ctx.empty(n, M).fill_(CANARY), ctx.empty(M, M).fill_(CANARY)

    def call(spec, M_=M, n_=n, ld1=M, ld2=M, Zp=Z, mup=mu):
        rc = ctx.lib.dsdgp_rbf_expectations(ctx.handle, C.byref(spec), _p(Zp), M_, _p(mup), _p(s), n_, _p(o0), _p(o1), ld1, _p(o2), ld2)
        ctx.sync()
        return rc

    good, keep = _spec(c)
    for spec, keep2 in (_spec(c, kind=1), _spec(c, has_white=1)):      # Matern52; RBF + White
        assert call(spec) == UNSUPPORTED
    assert call(good, M_=0) == BAD_ARG and call(good, M_=2049) == BAD_ARG
    assert call(good, n_=0) == BAD_ARG
    assert call(good, ld1=M - 1) == BAD_ARG and call(good, ld2=M - 1) == BAD_ARG
    assert call(good, Zp=None) == BAD_ARG and call(good, mup=None) == BAD_ARG
    for D in (0, 1025):
        bad, keep3 = _spec(c)
        bad.input_dim = D
        assert call(bad) == BAD_ARG
    for o in (o0, o1, o2):                                              # a refused call launches nothing
        assert np.all(o.cpu().numpy() == CANARY)
    assert call(good) == 0
