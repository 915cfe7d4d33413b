"""The CPU reference of tests/test_gpu_pca.py (tests/pca_reference.py) and its case table (tests/pca_cases.py) pinned on their own,
without a GPU — and the host side of pca_map that needs no device.

Above the "host side" rule the tests guard the yardstick: the numpy Jacobi (the device's iteration in float64 numpy) converges within 30
sweeps on every case it runs on and reproduces the long-double truth to within 2 D 2^-52 (|C|_F) in orthonormality, residual and
eigenvalues; on the cases with a gap behind the k-th eigenvalue its k-dimensional subspace is the truth's and np.linalg.svd's; the case
`offset` is one where the one-pass X^T X - n m m^T fails.  They import nothing of the package and pass with or without the feature.
Below the rule the tests call the package and fail without it."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import pca_cases as PC
from tests import pca_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAPPED = [n for n in PC.NAMES if PC.gapped(n)]


@pytest.mark.parametrize("name", PC.JACOBI_NAMES)
def test_numpy_jacobi_converges_and_matches_the_truth(name):
    tr, j = PC.truth(name), PC.jacobi(name)
    r_orth, r_res, r_lam = R.figures(tr, j["lam"], j["V"])
    print("%s: %d sweeps, %d rotations in the last; r_orth %.3g, r_res %.3g, r_lam %.3g" % (name, j["sweeps"], j["rotations"], r_orth,
                                                                                             r_res, r_lam))
    assert j["converged"] and j["sweeps"] <= 30
    assert np.all(np.diff(j["lam"]) <= 0.0)
    assert r_orth <= 2.0 and r_res <= 2.0 and r_lam <= 2.0


def test_worst_ratios_are_exposed():
    print("R_ORTH %.3g, R_RES %.3g, R_LAM %.3g, R_PROJ %.3g" % (R.R_ORTH, R.R_RES, R.R_LAM, R.R_PROJ))
    for r in (R.R_ORTH, R.R_RES, R.R_LAM, R.R_PROJ):
        assert 0.0 < r <= 2.0


def test_at_least_ten_cases_have_a_gap():
    print({n: round(PC.gap(n), 4) for n in PC.NAMES})
    assert len(GAPPED) >= 10
    assert all(PC.CASES[n][2] < PC.CASES[n][1] for n in GAPPED)


@pytest.mark.parametrize("name", [n for n in GAPPED if n in PC.JACOBI_NAMES])
def test_subspace_of_a_gapped_case_is_the_truths_and_the_svds(name):
    """A perturbation E of C moves the projector on an eigenvalue cluster with gap g by at most about 2 |E|_2 / g (Davis-Kahan); the
    numpy Jacobi's backward error is its residual, below D 2^-52 |C|_F, hence R_PROJ <= 2.  LAPACK's SVD of X has a backward error of
    the same order in X, i.e. a few D 2^-52 |C| in C: both projectors within 2 bars of the truth, 4 of each other."""
    X, k, center = PC.inputs(name)
    tr, V = PC.truth(name), PC.jacobi(name)["V"]
    fig = R.projector_figure(tr, V, k)
    Vs = np.linalg.svd(tr["Xc"] if center else X, full_matrices=False)[2][:k].T
    P, Ps = V[:, :k] @ V[:, :k].T, Vs @ Vs.T
    svd = float(np.linalg.norm(P - Ps, 2)) / PC.projector_bar(name)
    print("%s: gap %.3g, |P - P_truth| %.3g, |P - P_svd| %.3g (x bar)" % (name, PC.gap(name), fig, svd))
    assert fig <= R.R_PROJ <= 2.0
    assert svd <= 4.0


def test_reference_rules():
    """the skip rule, the 45 degree rotation, the order of equal eigenvalues and the sign rule, on matrices small enough to read"""
    rot, t, c, s = R.rotations(np.array([5.0, 1.0, 0.0]), np.array([5.0, 2.0, 0.0]), np.array([4.0, 0.0, 0.0]))
    assert list(rot) == [True, False, False] and t[0] == 1.0 and c[0] == s[0] and np.all(np.isfinite(t))
    j = R.jacobi(np.array([[5.0, 4.0], [4.0, 5.0]]))
    assert j["sweeps"] == 1 and j["converged"] and np.array_equal(j["lam"], [9.0, 1.0])
    assert j["V"][0, 0] == j["V"][1, 0] > 0 and j["V"][0, 1] > 0 > j["V"][1, 1]          # ties: the lowest row is made positive
    j = R.jacobi(np.diag([2.0, 7.0, 2.0, 7.0]))
    assert j["sweeps"] == 1 and j["rotations"] == 0 and np.array_equal(j["lam"], [7.0, 7.0, 2.0, 2.0])
    assert np.array_equal(j["V"], np.eye(4)[:, [1, 3, 0, 2]])                                # equal eigenvalues keep their index order
    for Dp in (2, 4, 6, 18):
        seen = set()
        for step in range(Dp - 1):
            p, q = R.pairs(step, Dp)
            assert np.all(p < q) and sorted(np.concatenate([p, q])) == list(range(Dp))
            seen |= set(zip(p.tolist(), q.tolist()))
        assert len(seen) == Dp * (Dp - 1) // 2          # a sweep meets every pair once


def test_offset_defeats_the_one_pass_formula():
    """what gives the case `offset` its teeth: float64 X^T X - n m m^T misses the long-double centred Gram by more than 1e4 times what
    Xc^T Xc does"""
    X, _, center = PC.inputs("offset")
    assert center
    tr = PC.truth("offset")
    m = X.mean(axis=0)
    one_pass = X.T @ X - X.shape[0] * np.outer(m, m)
    two_pass = tr["Xc"].T @ tr["Xc"]
    e1, e2 = float(np.max(np.abs(one_pass - tr["C"]))), float(np.max(np.abs(two_pass - tr["C"])))
    print("offset: one pass off by %.3g, two passes by %.3g" % (e1, e2))
    assert e1 > 1e4 * e2


# ------------------------------------------------------------------------------------------------ host side of the feature
def test_c_abi_is_declared_on_both_sides():
    from doubly_stochastic_dgp import _lib
    with open(os.path.join(ROOT, "include", "dsdgp.h")) as f:
        h = f.read()
    m = re.search(r"int dsdgp_pca\(([^;]*)\);", h)
    assert m, "include/dsdgp.h does not declare dsdgp_pca"
    assert len(m.group(1).split(",")) == 13
    res, args = _lib._PROTOS["dsdgp_pca"]
    assert res is ctypes.c_int and len(args) == 13
    assert args[2] is ctypes.c_int64 and all(args[i] is ctypes.c_int32 for i in (3, 4, 5, 6)) and args[8] is ctypes.c_int64
    assert "dsdgp_pca" in _lib.EXPORTED_SYMBOLS
    assert "layer_initializations.py:35" in h[h.index("dsdgp_pca: "):m.start()]


def test_every_refusal_comes_before_the_device():
    """no GPU is needed (or, where there is one, touched) to be told about a bad argument"""
    from doubly_stochastic_dgp.layer_initializations import _pca_args, pca_map
    X = np.random.default_rng(0).standard_normal((50, 3))
    bad = [
        dict(X=X[:, 0], k=1),                                     # not 2-D
        dict(X=X[None], k=1),
        dict(X=X, k=1.0),                                         # k not an integer
        dict(X=X, k=True),
        dict(X=X, k=0),                                           # k outside 1 .. D
        dict(X=X, k=4),
        dict(X=np.zeros((50, 0)), k=1),                           # D outside 1 .. 1024
        dict(X=np.zeros((5, 1025)), k=1),
        dict(X=np.zeros((0, 3)), k=1),                            # n < 1
        dict(X=X, k=2, max_sweeps=0),                             # max_sweeps outside 1 .. 64
        dict(X=X, k=2, max_sweeps=65),
        dict(X=np.where(np.arange(150).reshape(50, 3) == 7, np.nan, X), k=2),          # non-finite values
        dict(X=np.where(np.arange(150).reshape(50, 3) == 9, np.inf, X), k=2),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            pca_map(**kw)
        with pytest.raises(ValueError):
            _pca_args(kw["X"], kw["k"], kw.get("max_sweeps", 30))
    assert _pca_args(X, np.int64(3), 64) == (50, 3, 3, 64)


def _layers(**kw):
    from doubly_stochastic_dgp.gpflow_compat import RBF
    from doubly_stochastic_dgp.layer_initializations import init_layers_linear
    rng = np.random.default_rng(2)
    X, Y = rng.standard_normal((40, 5)), rng.standard_normal((40, 1))
    return init_layers_linear(X, Y, X[:7].copy(), [RBF(5), RBF(2), RBF(2)], white=True, **kw)


def test_pca_host_is_the_default_bit_for_bit():
    for a, b in zip(_layers(), _layers(pca="host")):
        assert np.array_equal(a.feature.Z.value, b.feature.Z.value)
        assert type(a.mean_function) is type(b.mean_function)
        if hasattr(a.mean_function, "A"):
            assert np.array_equal(a.mean_function.A.value, b.mean_function.A.value)
    A = _layers()[0].mean_function.A.value
    rng = np.random.default_rng(2)
    assert np.array_equal(A, np.linalg.svd(rng.standard_normal((40, 5)), full_matrices=False)[2][:2].T)


def test_an_unknown_pca_is_refused_before_the_device():
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian
    from doubly_stochastic_dgp.layer_initializations import _width_map
    with pytest.raises(ValueError):
        _layers(pca="nonsense")
    with pytest.raises(ValueError):
        _width_map(3, 2, np.zeros((4, 3)), pca="gpu")
    X = np.random.default_rng(1).standard_normal((20, 3))
    with pytest.raises(ValueError):
        DGP(X, np.zeros((20, 1)), X[:5].copy(), [RBF(3), RBF(2)], Gaussian(), pca="nonsense")


def test_valid_arguments_reach_the_device_or_its_absence():
    """with valid arguments the call goes on to the context: without a GPU that is the library's "no CPU fallback" error"""
    import torch
    from doubly_stochastic_dgp import _lib
    from doubly_stochastic_dgp.layer_initializations import pca_map
    X = np.random.default_rng(0).standard_normal((50, 3))
    if torch.cuda.is_available():
        assert pca_map(X, 2).shape == (3, 2)
    else:
        with pytest.raises(_lib.DsdgpError, match="no CPU fallback"):
            pca_map(X, 2)
