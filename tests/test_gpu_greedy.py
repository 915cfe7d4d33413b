"""-m gpu: greedy conditional-variance selection of the inducing points on the device (csrc/greedy.hip; dsdgp_greedy_inducing,
layer_initializations.greedy_inducing, DGP(..., inducing="greedy")) against tests/greedy_reference.py on the cases of
tests/greedy_cases.py.

Bounds.  indices and m: exactly the long-double reference's — every case keeps a margin of at least 1e-9 v between the two largest
conditional variances at every step (tests/test_greedy_reference_cpu.py asserts it), against a drift of about 2 j^2 2^-53 v under a
different summation order.  Z: the bits of X[indices].
residual, trace and the entries of L L^T: within 8 max(e64, 2^-50) of the reference's, in units of v (residual, L L^T) and of n v
(trace), e64 being the distance of the plain float64 numpy version from the same reference for that case and quantity; the factor 8
covers a different but fixed summation order (the rule of tests/test_gpu_natgrad_direct.py).  The products L L^T are formed in long
double from each L, so they measure the factors and not the product's own rounding.
L L^T against dsdgp_gram(Z) at jitter 0: (m + 4) 2^-52 (v + white) for the factorisation (tests/test_greedy_reference_cpu.py) plus
what the Gram build may lose forming r^2 from |x|^2 + |z|^2 - 2 x.z, (D + 4) 2^-52 times the largest scaled squared norm of a pair,
times |dk / dr^2| <= v; on a Matern52 diagonal the Gram build evaluates the formula at r = 1e-6 where Kdiag is v: 1e-12 v more.
DSDGP_GREEDY_PROFILE=<file> writes the measured ratios and the margins per case (profiles/greedy_errors.md)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import greedy_cases as GC
from tests import greedy_reference as R

pytestmark = pytest.mark.gpu

OK, BAD_ARG, UNSUPPORTED = 0, -1, -4
CANARY = -12345.25
ICANARY = -77
_ROWS = []


@pytest.fixture(scope="module")
def ctx():
    from doubly_stochastic_dgp.engine import Context
    return Context.get()


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("DSDGP_GREEDY_PROFILE")
    if not path or not _ROWS:
        return
    with open(path, "w") as f:
        f.write("# Greedy inducing points on the device: measured errors (tests/test_gpu_greedy.py)\n\n"
                "`indices`: entries that differ from the long-double reference of tests/greedy_reference.py (held to 0; `m` is exact).\n"
                "`residual`, `trace`, `L L^T`: the device's distance from the reference over the bar 8 max(e64, 2^-50) (1 = at the bar;\n"
                "units of v, n v, v), and in brackets e64, the float64 numpy version's own distance in the same units.  `margin`: the\n"
                "reference's smallest gap between the two largest conditional variances at a step, over v.\n\n"
                "| case | n | D | M | m | indices | residual (e64) | trace (e64) | L L^T (e64) | margin |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for r in _ROWS:
            f.write("| %s | %d | %d | %d | %d | %d | %.3g (%.2g) | %.3g (%.2g) | %.3g (%.2g) | %.3g |\n" % r)


def _greedy(name, X=None):
    from doubly_stochastic_dgp.layer_initializations import greedy_inducing
    c = GC.inputs(name)
    return greedy_inducing(c["X"] if X is None else X, c["M"], GC.kernel_of(name), first=c["first"], threshold=c["threshold"],
                           return_info=True)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _llt(L):
    Lw = np.asarray(L).astype(R.LD)
    return Lw @ Lw.T


@pytest.mark.parametrize("name", GC.NAMES)
def test_cases_match_the_reference(name):
    c = GC.inputs(name)
    ref, f64 = GC.reference(name), GC.float64(name)
    assert ref["margin"] >= GC.MARGIN, "the reference's margin does not pin the rows"
    Z, info = _greedy(name)
    X, v = c["X"], c["v"]
    n, D = X.shape
    m = ref["m"]
    assert info["m"] == m and info["indices"].dtype == np.int32 and info["indices"].shape == (info["m"],)
    assert Z.shape == (m, D) and info["residual"].shape == (m,) and info["trace"].shape == (m,) and info["L"].shape == (m, m)
    differ = int(np.sum(info["indices"] != ref["indices"]))
    ref_llt = _llt(ref["L"])
    figs = []
    for key, unit in (("residual", v), ("trace", n * v), ("L", v)):
        if key == "L":
            dev, e64 = float(np.abs(_llt(info["L"]) - ref_llt).max()) / unit, float(np.abs(_llt(f64["L"]) - ref_llt).max()) / unit
        else:
            dev = float(np.abs(info[key].astype(R.LD) - ref[key]).max()) / unit
            e64 = float(np.abs(f64[key].astype(R.LD) - ref[key]).max()) / unit
        figs.append((dev / (8.0 * max(e64, 2.0 ** -50)), e64))
    row = (name, n, D, c["M"], info["m"], differ) + tuple(x for f in figs for x in f) + (ref["margin"],)
    print("%s (%d x %d, M = %d): m = %d, %d indices differ; residual %.3g (e64 %.2g), trace %.3g (e64 %.2g), L L^T %.3g (e64 %.2g) "
          "of the bar; margin %.3g" % row)
    _ROWS.append(row)
    assert differ == 0
    assert _same_bits(Z, X[ref["indices"]])
    assert np.all(np.triu(info["L"], 1) == 0)
    for ratio, _ in figs:
        assert ratio <= 1.0


@pytest.mark.parametrize("name", ["a", "b", "white"])
def test_l_factorises_the_gram_matrix_of_z(ctx, name):
    from doubly_stochastic_dgp import _lib
    c = GC.inputs(name)
    Z, info = _greedy(name)
    m, D = Z.shape
    ls = np.ascontiguousarray(c["ls"], dtype=np.float64)
    spec = _lib.KernelSpec(kind={"rbf": 0, "matern52": 1}[c["kind"]], input_dim=D, ard=int(c["ard"]), has_white=int(c["white"] > 0),
                           variance=c["v"], white_variance=c["white"], lengthscales=ls.ctypes.data_as(_lib.c_double_p))
    dZ, out = ctx.to_device(Z), ctx.empty(m, m)
    _lib.check(ctx.lib.dsdgp_gram(ctx.handle, C.byref(spec), C.c_void_p(dZ.data_ptr()), m, None, 0, 0.0, C.c_void_p(out.data_ptr()), m))
    ctx.sync()
    Ku = out.cpu().numpy()
    norm = float(((Z / ls) ** 2).sum(1).max())
    bound = (m + 4) * 2.0 ** -52 * (c["v"] + c["white"]) + (D + 4) * 2.0 ** -52 * 4.0 * norm * c["v"]
    if c["kind"] == "matern52":
        bound += 1e-12 * c["v"]
    err = float(np.abs(_llt(info["L"]) - Ku.astype(R.LD)).max())
    print("%s: |L L^T - dsdgp_gram(Z)| = %.3g (bound %.3g)" % (name, err, bound))
    assert err <= bound


@pytest.mark.parametrize("name", ["d", "dup"])
def test_a_second_call_and_a_device_tensor_give_the_same_bits(ctx, name):
    Z1, i1 = _greedy(name)
    Z2, i2 = _greedy(name)
    Z3, i3 = _greedy(name, ctx.to_device(GC.inputs(name)["X"]))
    for Z, i in ((Z2, i2), (Z3, i3)):
        assert _same_bits(Z, Z1) and i["m"] == i1["m"]
        for key in ("indices", "residual", "trace", "L"):
            assert _same_bits(i[key], i1[key]), key


# ------------------------------------------------------------------------------------------------ the C entry point itself
def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


class _Raw:
    """device buffers of one case, each with a canary one element past its end (L: one column past every row, and one row)"""

    def __init__(self, ctx, name):
        from doubly_stochastic_dgp import _lib
        torch = ctx.torch
        c = GC.inputs(name)
        self.ctx, self.c = ctx, c
        self.n, self.D = c["X"].shape
        self.M = M = c["M"]
        self.ls = np.ascontiguousarray(c["ls"], dtype=np.float64)
        self.spec = _lib.KernelSpec(kind={"rbf": 0, "matern52": 1}[c["kind"]], input_dim=self.D, ard=int(c["ard"]),
                                    has_white=int(c["white"] > 0), variance=c["v"], white_variance=c["white"],
                                    lengthscales=self.ls.ctypes.data_as(_lib.c_double_p))
        self.X = ctx.to_device(c["X"])
        dev = self.X.device
        self.idx = torch.full((M + 1,), ICANARY, dtype=torch.int32, device=dev)
        self.m = torch.full((2,), ICANARY, dtype=torch.int32, device=dev)
        self.Z = ctx.empty(M + 1, self.D).fill_(CANARY)
        self.res = ctx.empty(M + 1).fill_(CANARY)
        self.tr = ctx.empty(M + 1).fill_(CANARY)
        self.ldl = M + 1
        self.L = ctx.empty(M + 1, self.ldl).fill_(CANARY)

    def call(self, **kw):
        a = dict(spec=self.spec, X=self.X, n=self.n, M=self.M, first=-1 if self.c["first"] is None else self.c["first"],
                 threshold=self.c["threshold"], idx=self.idx, m=self.m, Z=self.Z, res=self.res, tr=self.tr, L=self.L, ldl=self.ldl)
        a.update(kw)
        rc = self.ctx.lib.dsdgp_greedy_inducing(self.ctx.handle, C.byref(a["spec"]) if a["spec"] is not None else None, _p(a["X"]), a["n"],
                                                a["M"], a["first"], a["threshold"], _p(a["idx"]), _p(a["m"]), _p(a["Z"]), _p(a["res"]),
                                                _p(a["tr"]), _p(a["L"]), a["ldl"])
        self.ctx.sync()
        return rc

    def canaries_intact(self):
        M = self.M
        return (int(self.idx[M]) == ICANARY and int(self.m[1]) == ICANARY and bool((self.Z[M] == CANARY).all())
                and float(self.res[M]) == CANARY and float(self.tr[M]) == CANARY and bool((self.L[M] == CANARY).all())
                and bool((self.L[:, M] == CANARY).all()))

    def untouched(self):
        return (self.canaries_intact() and bool((self.idx == ICANARY).all()) and bool((self.m == ICANARY).all())
                and all(bool((t == CANARY).all()) for t in (self.Z, self.res, self.tr, self.L)))


def test_an_early_stop_leaves_the_documented_fill(ctx):
    raw = _Raw(ctx, "dup")
    ref = GC.reference("dup")
    assert raw.call() == OK, ctx.lib.dsdgp_last_error()
    M, m = raw.M, ref["m"]
    assert m == 20 < M and int(raw.m[0]) == m and raw.canaries_intact()
    idx = raw.idx[:M].cpu().numpy()
    assert np.array_equal(idx[:m], ref["indices"]) and np.all(idx[m:] == -1)
    res, tr = raw.res[:M].cpu().numpy(), raw.tr[:M].cpu().numpy()
    assert np.all(res[:m] > raw.c["threshold"]) and np.all(res[m:] == 0.0)
    assert np.all(tr[m:].view(np.uint64) == tr[m - 1:m].view(np.uint64))
    Z, L = raw.Z[:M].cpu().numpy(), raw.L[:M, :M].cpu().numpy()
    assert _same_bits(Z[:m], raw.c["X"][idx[:m]]) and np.all(Z[m:] == 0.0) and np.all(L[m:] == 0.0) and np.all(L[:m, m:] == 0.0)
    Zh, info = _greedy("dup")
    assert _same_bits(Zh, Z[:m]) and _same_bits(info["L"], L[:m, :m]) and _same_bits(info["trace"], tr[:m])


@pytest.mark.parametrize("name", ["edge", "first"])
def test_every_optional_output_may_be_null(ctx, name):
    raw = _Raw(ctx, name)
    assert raw.call() == OK, ctx.lib.dsdgp_last_error()
    assert raw.canaries_intact()
    M = raw.M
    full = {k: getattr(raw, k).cpu().numpy().copy() for k in ("idx", "m", "Z", "res", "tr", "L")}
    assert np.array_equal(full["idx"][:M], GC.reference(name)["indices"])
    for null in (("Z",), ("res",), ("tr",), ("L",), ("Z", "res", "tr", "L")):
        fresh = _Raw(ctx, name)
        assert fresh.call(**{k: None for k in null}) == OK, ctx.lib.dsdgp_last_error()
        assert fresh.canaries_intact()
        for k in ("idx", "m", "Z", "res", "tr", "L"):
            got = getattr(fresh, k).cpu().numpy()
            if k in null:
                assert np.all(got == CANARY), (null, k)
            else:
                assert _same_bits(got, full[k]), (null, k)


def test_bad_arguments_return_an_error_and_touch_nothing(ctx):
    from doubly_stochastic_dgp import _lib
    raw = _Raw(ctx, "edge")
    n, M, D = raw.n, raw.M, raw.D
    err = ctx.lib.dsdgp_last_error

    def spec(**kw):
        a = dict(kind=0, input_dim=D, ard=1, has_white=0, variance=1.0, white_variance=0.0, lengthscales=raw.ls.ctypes.data_as(_lib.c_double_p))
        a.update(kw)
        return _lib.KernelSpec(**a)

    for kw in (dict(n=M - 1), dict(n=2 ** 31), dict(M=1), dict(M=2049), dict(spec=spec(input_dim=0)), dict(spec=spec(input_dim=1025)),
               dict(spec=spec(kind=2)), dict(spec=spec(kind=-1)), dict(first=-2), dict(first=n), dict(threshold=-1e-300),
               dict(threshold=float("nan")), dict(X=None), dict(idx=None), dict(m=None), dict(ldl=M - 1), dict(spec=None)):
        assert raw.call(**kw) == BAD_ARG, kw
        assert b"bad argument" in err(), kw
        assert raw.untouched(), kw
    assert raw.call() == OK and int(raw.m[0]) == M


def test_the_workspace_cap_is_reported_not_allocated(ctx):
    from doubly_stochastic_dgp import _lib
    raw = _Raw(ctx, "edge")
    # 2048 columns of 2^19 + 1 rows: one row past 2^30 doubles; the X buffer holds 257 rows and is never read
    assert 2048 * (2 ** 19 + 1) > 2 ** 30 >= 2048 * 2 ** 19
    big = _Raw(ctx, "edge")
    big.idx = ctx.torch.full((2049,), ICANARY, dtype=ctx.torch.int32, device=raw.X.device)
    assert big.call(n=2 ** 19 + 1, M=2048, Z=None, res=None, tr=None, L=None) == UNSUPPORTED
    assert b"subset of the rows" in ctx.lib.dsdgp_last_error()
    assert bool((big.idx == ICANARY).all()) and bool((big.m == ICANARY).all())
    # the transposed copy of X has the same cap: 1024 columns of 2^20 + 1 rows
    ls = np.ones(1)
    wide = _lib.KernelSpec(kind=0, input_dim=1024, ard=0, has_white=0, variance=1.0, white_variance=0.0, lengthscales=ls.ctypes.data_as(_lib.c_double_p))
    assert raw.call(spec=wide, n=2 ** 20 + 1, M=2, Z=None, res=None, tr=None, L=None) == UNSUPPORTED
    assert raw.untouched()
    # at the cap itself the call is accepted as far as its arguments go: not run here, it would need the 8 GB


def test_dgp_takes_the_greedy_rule_for_an_integer_z():
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian
    from doubly_stochastic_dgp.layer_initializations import greedy_inducing, kmeans_inducing
    X = np.array(GC.inputs("b")["X"])
    Y = np.random.default_rng(11).standard_normal((X.shape[0], 1))
    model = DGP(X, Y, 37, [RBF(8), RBF(8)], Gaussian(), inducing="greedy")
    Z = greedy_inducing(X, 37, RBF(8))
    assert Z.shape == (37, 8) and _same_bits(np.ascontiguousarray(model.layers[0].feature.Z.value), Z)
    assert np.isfinite(model.train_step(0.01, sync=True))
    plain = DGP(X, Y, 37, [RBF(8), RBF(8)], Gaussian())
    assert _same_bits(np.ascontiguousarray(plain.layers[0].feature.Z.value), kmeans_inducing(X, 37, seed=0))
    with pytest.raises(ValueError, match="only 20 of"):
        dup = np.array(GC.inputs("dup")["X"])
        DGP(dup, np.zeros((dup.shape[0], 1)), 32, [RBF(4, lengthscales=1.5), RBF(4)], Gaussian(), inducing="greedy")
