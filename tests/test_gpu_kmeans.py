"""-m gpu: k-means for the inducing points on the device (csrc/kmeans.hip; dsdgp_kmeans, layer_initializations.kmeans_inducing,
DGP(X, Y, M, ...)) against tests/kmeans_reference.py on the cases of tests/kmeans_cases.py, for 1, 2 and 10 iterations.

Bounds.  Labels and counts: exactly the reference's — every case keeps a margin of at least 1e-9 between a row's two nearest centres
in units of |x_i - xbar|^2 + max_m |z_m - xbar|^2 (tests/test_kmeans_reference_cpu.py asserts it), several orders above what a
correctly rounded |z|^2 - 2 x.z on centred data loses (about (D + 8) 2^-53 of those units).
Centres: |Z - Z_ref| <= max_count 2^-52 max|X| elementwise, the bound of summing max_count terms of size max|X| one after another; the
labels agree at every iteration, so nothing compounds.
Inertia: within 4 (D + 8) 2^-53 sum_i (|x_i - xbar|^2 + max_m |z_m - xbar|^2) of the reference's.
DSDGP_KMEANS_PROFILE=<file> writes the measured error of every case (profiles/kmeans_errors.md)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import kmeans_cases as KC

pytestmark = pytest.mark.gpu

BAD_ARG = -1
CANARY = -12345.25
_ROWS = []


@pytest.fixture(scope="module")
def ctx():
    from doubly_stochastic_dgp.engine import Context
    return Context.get()


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("DSDGP_KMEANS_PROFILE")
    if not path or not _ROWS:
        return
    with open(path, "w") as f:
        f.write("# Device k-means: measured errors (tests/test_gpu_kmeans.py)\n\n"
                "`labels`, `counts`: entries that differ from tests/kmeans_reference.py (held to 0).  `Z`: the worst |Z - Z_ref| over\n"
                "max_count 2^-52 max|X| (1 = at the bound).  `inertia`: |inertia - reference| over\n"
                "4 (D + 8) 2^-53 sum_i (|x_i - xbar|^2 + max_m |z_m - xbar|^2) (1 = at the bound).  `margin`: the reference's smallest\n"
                "relative margin between a row's two nearest centres up to that iteration.\n\n"
                "| case | n | D | M | iters | labels | counts | Z | inertia | margin |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for r in _ROWS:
            f.write("| %s | %d | %d | %d | %d | %d | %d | %.3g | %.3g | %.3g |\n" % r)


def _kmeans(X, idx, iters):
    from doubly_stochastic_dgp.layer_initializations import kmeans_inducing
    return kmeans_inducing(X, len(idx), iter=iters, init=idx, return_info=True)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("name,iters", [(n, it) for n in KC.NAMES for it in KC.iters_of(n)])
def test_cases_match_the_reference(name, iters):
    X, idx, _, _ = KC.inputs(name)
    ref = KC.reference(name)[iters - 1]
    assert ref["margin"] >= KC.MARGIN, "the reference's margin does not pin the labels"
    Z, info = _kmeans(X, idx, iters)
    n, D = X.shape
    M = len(idx)
    zb = float(ref["counts"].max()) * 2.0 ** -52 * float(np.abs(X).max())
    ib = 4.0 * (D + 8) * 2.0 ** -53 * ref["scale"]
    fig = (name, n, D, M, iters, int(np.sum(info["labels"] != ref["labels"])), int(np.sum(info["counts"] != ref["counts"])),
           float(np.abs(Z - ref["Z"]).max()) / zb, abs(info["inertia"] - ref["inertia"]) / ib, ref["margin"])
    print("%s (%d x %d, M = %d), %d iterations: %d labels, %d counts differ; Z %.3g, inertia %.3g (x bound); margin %.3g" % fig)
    _ROWS.append(fig)
    assert Z.shape == (M, D) and info["labels"].shape == (n,) and info["counts"].shape == (M,)
    assert info["labels"].dtype == np.int32 and info["counts"].dtype == np.int64
    assert info["labels"].min() >= 0 and info["labels"].max() < M
    assert np.array_equal(info["labels"], ref["labels"])
    assert np.array_equal(info["counts"], ref["counts"])
    assert np.all(np.abs(Z - ref["Z"]) <= zb)
    assert abs(info["inertia"] - ref["inertia"]) <= ib
    if name == "dup":
        assert not np.any(info["labels"] == KC.DUP) and info["counts"][KC.DUP] == 0
        assert _same_bits(Z[KC.DUP], X[idx[KC.DUP]])          # an empty cluster keeps its centre bit for bit


@pytest.mark.parametrize("name", ["e", "f"])
def test_a_second_call_and_a_device_tensor_give_the_same_bits(ctx, name):
    X, idx, _, _ = KC.inputs(name)
    Z1, i1 = _kmeans(X, idx, 10)
    Z2, i2 = _kmeans(X, idx, 10)
    Z3, i3 = _kmeans(ctx.to_device(X), idx, 10)
    for Z, i in ((Z2, i2), (Z3, i3)):
        assert _same_bits(Z, Z1) and np.array_equal(i["labels"], i1["labels"]) and np.array_equal(i["counts"], i1["counts"])
        assert np.float64(i["inertia"]).view(np.uint64) == np.float64(i1["inertia"]).view(np.uint64)


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _raw(ctx, Xd, Z0d, Zd, n, D, M, iters, labels=None, counts=None, inertia=None, X_null=False):
    rc = ctx.lib.dsdgp_kmeans(ctx.handle, None if X_null else _p(Xd), n, D, M, _p(Z0d), iters, _p(Zd), _p(labels), _p(counts), _p(inertia))
    ctx.sync()
    return rc


@pytest.mark.parametrize("name", ["b", "dup"])
def test_z_may_alias_z0_and_the_outputs_are_optional(ctx, name):
    torch = ctx.torch
    X, idx, _, _ = KC.inputs(name)
    iters = 2 if name == "b" else 1
    n, D = X.shape
    M = len(idx)
    Xd = ctx.to_device(X)
    Z0 = ctx.to_device(X[idx])
    Zsep = ctx.empty(M + 1, D).fill_(CANARY)
    lab = torch.full((n + 1,), -7, dtype=torch.int32, device=Xd.device)
    cnt = torch.full((M + 1,), -7, dtype=torch.int64, device=Xd.device)
    ine = ctx.empty(2).fill_(CANARY)
    assert _raw(ctx, Xd, Z0, Zsep, n, D, M, iters, lab, cnt, ine) == 0, ctx.lib.dsdgp_last_error()
    assert np.array_equal(Z0.cpu().numpy(), X[idx]), "Z0 was written"
    assert np.all(Zsep[M].cpu().numpy() == CANARY) and int(lab[n]) == -7 and int(cnt[M]) == -7 and float(ine[1]) == CANARY
    Zal = Z0.clone()
    assert _raw(ctx, Xd, Zal, Zal, n, D, M, iters) == 0, ctx.lib.dsdgp_last_error()
    assert _same_bits(Zal.cpu().numpy(), Zsep[:M].cpu().numpy())
    Zh, info = _kmeans(X, idx, iters)
    assert _same_bits(Zh, Zsep[:M].cpu().numpy()) and np.array_equal(info["labels"], lab[:n].cpu().numpy())
    assert np.array_equal(info["counts"], cnt[:M].cpu().numpy()) and info["inertia"] == float(ine[0])


def test_dgp_takes_an_integer_for_z():
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian
    from doubly_stochastic_dgp.layer_initializations import kmeans_inducing
    X = KC.inputs("a")[0]
    Y = np.random.default_rng(11).standard_normal((X.shape[0], 1))
    model = DGP(X, Y, 37, [RBF(8), RBF(8)], Gaussian())
    Z = kmeans_inducing(X, 37, seed=0)
    assert _same_bits(np.ascontiguousarray(model.layers[0].feature.Z.value), Z)
    also = DGP(X, Y, np.int64(37), [RBF(8), RBF(8)], Gaussian())
    assert _same_bits(np.ascontiguousarray(also.layers[0].feature.Z.value), Z)
    assert np.isfinite(model.train_step(0.01, sync=True))


def test_seeded_start_rows_are_the_documented_draw():
    from doubly_stochastic_dgp.layer_initializations import kmeans_inducing
    X = KC.inputs("b")[0]
    idx = np.random.default_rng(3).choice(X.shape[0], 16, replace=False)
    assert _same_bits(kmeans_inducing(X, 16, iter=2, seed=3), kmeans_inducing(X, 16, iter=2, init=idx))
    assert _same_bits(kmeans_inducing(X, 16, iter=2, seed=3), kmeans_inducing(X, 16, iter=2, init=X[idx]))


def test_bad_arguments_return_an_error_and_leave_z_alone(ctx):
    X, idx, _, _ = KC.inputs("h")
    n, D = X.shape
    M = len(idx)
    Xd, Z0 = ctx.to_device(X), ctx.to_device(X[idx])
    Z = ctx.empty(M, D).fill_(CANARY)
    err = ctx.lib.dsdgp_last_error
    for kw in (dict(n=M - 1), dict(M=1), dict(M=2049), dict(D=0), dict(D=1025), dict(iters=0), dict(iters=-1)):
        a = dict(n=n, D=D, M=M, iters=1)
        a.update(kw)
        assert _raw(ctx, Xd, Z0, Z, a["n"], a["D"], a["M"], a["iters"]) == BAD_ARG, kw
        assert b"bad argument" in err()
    assert _raw(ctx, Xd, Z0, Z, n, D, M, 1, X_null=True) == BAD_ARG
    assert _raw(ctx, Xd, None, Z, n, D, M, 1) == BAD_ARG
    assert _raw(ctx, Xd, Z0, None, n, D, M, 1) == BAD_ARG
    assert np.all(Z.cpu().numpy() == CANARY)
    assert _raw(ctx, Xd, Z0, Z, n, D, M, 1) == 0
    assert np.all(np.isfinite(Z.cpu().numpy()))
