"""The CPU reference of tests/test_gpu_kmeans.py (tests/kmeans_reference.py) and its case table (tests/kmeans_cases.py) pinned on their
own, without a GPU — and the host side of kmeans_inducing that needs no device.

Above the "host side" rule the tests guard the yardstick: the reference is scipy's kmeans2 (labels equal, centres to 1e-12) wherever
scipy's own route is well conditioned, i.e. everywhere but case g (X = N(0, 1) + 1e6: scipy forms |x|^2 + |z|^2 - 2 x.z on the
uncentred data and mislabels rows there — asserted below as well, it is why the device path centres); every case keeps the margin under
which a correctly rounded device result must give the reference's labels; no case a - i ever has an empty cluster.  They import nothing
of the package and pass with or without the feature.  Below the rule the tests call the package and fail without it."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

from tests import kmeans_cases as KC
from tests import kmeans_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scipy(name):
    from scipy.cluster.vq import kmeans2
    X, idx, iters, _ = KC.inputs(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # `dup` has an empty cluster: missing='warn'
        return kmeans2(X, X[idx].copy(), iter=iters, minit="matrix")


@pytest.mark.parametrize("name", [n for n in KC.NAMES if n != "g"])
def test_reference_equals_scipy(name):
    Zs, ls = _scipy(name)
    ref = KC.reference(name)[-1]
    err = float(np.max(np.abs(Zs - ref["Z"])))
    print(name, "labels that differ:", int(np.sum(ls != ref["labels"])), "max |Z - Z_scipy|:", err)
    assert np.array_equal(ls, ref["labels"])
    assert err <= 1e-12


def test_scipy_is_badly_conditioned_far_from_the_origin():
    """case g: the reason for centring.  kmeans2 from the same start mislabels rows against direct differences."""
    Zs, ls = _scipy("g")
    ref = KC.reference("g")[-1]
    wrong = int(np.sum(ls != ref["labels"]))
    print("g: kmeans2 mislabels", wrong, "of", ls.size, "rows; centres off by", float(np.max(np.abs(Zs - ref["Z"]))))
    assert wrong > 0


@pytest.mark.parametrize("name", KC.NAMES)
def test_every_case_keeps_its_margin(name):
    ref = KC.reference(name)
    print(name, "margin per iteration:", [r["margin"] for r in ref])
    assert ref[-1]["margin"] >= KC.MARGIN
    assert all(a["margin"] >= b["margin"] for a, b in zip(ref, ref[1:]))          # the running minimum


@pytest.mark.parametrize("name", list(KC.CASES))
def test_no_empty_clusters(name):
    for it, r in enumerate(KC.reference(name)):
        assert r["counts"].min() >= 1, (name, it)
        assert r["counts"].sum() == KC.CASES[name][0]


def test_dup_leaves_the_copy_empty():
    X, idx, _, _ = KC.inputs("dup")
    r = KC.reference("dup")[0]
    assert np.array_equal(X[idx[KC.DUP]], X[idx[3]])
    assert r["counts"][KC.DUP] == 0 and not np.any(r["labels"] == KC.DUP)
    assert np.array_equal(r["Z"][KC.DUP], X[idx[KC.DUP]])          # an empty cluster keeps its centre
    assert r["counts"][3] >= 1


def test_reference_carries_its_centres_in_extended_precision():
    """what keeps the reference's own inertia error on case g below the bound the device is held to (tests/kmeans_reference.py)"""
    assert np.finfo(R.LD).eps <= 2.0 ** -63


def test_reference_ties_and_inertia():
    X = np.array([[0.0], [1.0], [2.0], [10.0]])
    Z0 = np.array([[1.0], [1.0], [10.0]])          # centres 0 and 1 tie everywhere: the lowest index wins, centre 1 stays
    r = R.lloyd(X, Z0, 2)
    assert np.array_equal(r[0]["labels"], [0, 0, 0, 2]) and np.array_equal(r[0]["counts"], [3, 0, 1])
    assert r[0]["inertia"] == 2.0 and np.array_equal(r[0]["Z"], [[1.0], [1.0], [10.0]])
    assert r[1]["inertia"] == 2.0


# ------------------------------------------------------------------------------------------------ host side of the feature
def test_c_abi_is_declared_on_both_sides():
    from doubly_stochastic_dgp import _lib
    with open(os.path.join(ROOT, "include", "dsdgp.h")) as f:
        h = f.read()
    m = re.search(r"int dsdgp_kmeans\(([^;]*)\);", h)
    assert m, "include/dsdgp.h does not declare dsdgp_kmeans"
    assert len(m.group(1).split(",")) == 11
    res, args = _lib._PROTOS["dsdgp_kmeans"]
    assert res is ctypes.c_int and len(args) == 11
    assert args[2] is ctypes.c_int64 and args[3] is ctypes.c_int32 and args[4] is ctypes.c_int32 and args[6] is ctypes.c_int32
    assert "run_regression.py:57" in h[h.index("dsdgp_kmeans: "):m.start()]


def test_every_refusal_comes_before_the_device():
    """no GPU is needed (or, where there is one, touched) to be told about a bad argument"""
    from doubly_stochastic_dgp.layer_initializations import kmeans_inducing
    X = np.random.default_rng(0).standard_normal((50, 3))
    bad = [
        dict(X=X[:, 0], M=5),                                     # not 2-D
        dict(X=X[None], M=5),
        dict(X=X, M=1),                                           # M outside 2 .. 2048
        dict(X=X, M=0),
        dict(X=np.zeros((3000, 2)), M=2049),
        dict(X=X, M=2.5),
        dict(X=np.zeros((50, 0)), M=5),                           # D outside 1 .. 1024
        dict(X=np.zeros((50, 1025)), M=5),
        dict(X=X, M=5, iter=0),                                   # iter < 1
        dict(X=X, M=5, iter=-3),
        dict(X=X, M=51),                                          # M > n
        dict(X=X, M=5, init=np.arange(4)),                        # init: wrong shapes
        dict(X=X, M=5, init=np.zeros((5, 2))),
        dict(X=X, M=5, init=np.zeros((4, 3))),
        dict(X=X, M=5, init=np.zeros((5, 3, 1))),
        dict(X=X, M=5, init=np.arange(5.0)),                      # indices must be integers
        dict(X=X, M=5, init=np.array([0, 1, 2, 3, 50])),          # index out of range
        dict(X=X, M=5, init=np.array([-1, 1, 2, 3, 4])),
        dict(X=np.where(np.arange(150).reshape(50, 3) == 7, np.nan, X), M=5),          # non-finite values
        dict(X=np.where(np.arange(150).reshape(50, 3) == 9, np.inf, X), M=5),
        dict(X=X, M=5, init=np.full((5, 3), np.nan)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            kmeans_inducing(**kw)


def test_dgp_refuses_a_bad_integer_z_before_the_device():
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian
    X = np.random.default_rng(1).standard_normal((20, 2))
    with pytest.raises(ValueError):
        DGP(X, np.zeros((20, 1)), 21, [RBF(2), RBF(2)], Gaussian())
    with pytest.raises(ValueError):
        DGP(X, np.zeros((20, 1)), np.int64(1), [RBF(2), RBF(2)], Gaussian())


def test_valid_arguments_reach_the_device_or_its_absence():
    """with valid arguments the call goes on to the context: without a GPU that is the library's "no CPU fallback" error"""
    import torch
    from doubly_stochastic_dgp import _lib
    from doubly_stochastic_dgp.layer_initializations import kmeans_inducing
    X = np.random.default_rng(0).standard_normal((50, 3))
    for call in (lambda: kmeans_inducing(X, 5), lambda: kmeans_inducing(X, 5, init=np.arange(5)),
                 lambda: kmeans_inducing(X, 5, init=X[:5], iter=1)):
        if torch.cuda.is_available():
            assert call().shape == (5, 3)
        else:
            with pytest.raises(_lib.DsdgpError, match="no CPU fallback"):
                call()
