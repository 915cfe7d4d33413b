"""Host logic of DGP_Base.sample_functions that needs no device: what it refuses, it refuses with NotImplementedError before a device
is touched; the basis sampler is the documented sequence of draws; the library's host mirror binds the new calls."""
import numpy as np
import pytest

from doubly_stochastic_dgp import _lib, pathwise
from doubly_stochastic_dgp.dgp import DGP
from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian, Matern52, White
from doubly_stochastic_dgp.layers import SVGP_Layer
from tests import pathwise_reference as PR


def _data(D=2, n=12, M=5):
    rng = np.random.RandomState(0)
    X = rng.randn(n, D)
    return X, rng.randn(n, 1), X[:M].copy()


def test_input_propagation_is_refused():
    X, Y, Z = _data()
    model = DGP(X, Y, Z, [RBF(2), RBF(2)], Gaussian())
    model.layers[0].input_prop_dim = 1
    with pytest.raises(NotImplementedError, match="input_prop_dim"):
        model.sample_functions(2, 16)


def test_other_models_and_layers_are_refused():
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed, DGP_Heinonen, DGP_SGPMC
    X, Y, Z = _data()
    for cls in (DGP_Collapsed, DGP_Heinonen, DGP_SGPMC):
        model = object.__new__(cls)                       # the refusal reads the type alone
        with pytest.raises(NotImplementedError, match=cls.__name__):
            pathwise.PathwiseFunctions(model, 2, 16)
    model = DGP(X, Y, Z, [RBF(2), RBF(2)], Gaussian())

    class Other(SVGP_Layer):
        pass
    model.layers[1].__class__ = Other
    with pytest.raises(NotImplementedError, match="layer 1 is a Other"):
        model.sample_functions(2, 16)


def test_kernels_outside_the_spectral_table_are_refused():
    X, Y, Z = _data()
    model = DGP(X, Y, Z, [RBF(2), RBF(2)], Gaussian())
    model.layers[0].kern = White(2)
    with pytest.raises(NotImplementedError):
        model.sample_functions(2, 16)
    with pytest.raises(NotImplementedError):
        pathwise.sample_basis("matern32", 2, 4, 1.0, np.random.default_rng(0))


def test_the_basis_sampler_is_the_documented_sequence():
    for kind, ls in (("rbf", 0.7), ("matern52", [0.5, 2.0, 1.0])):
        Om = pathwise.sample_basis(kind, 3, 9, ls, np.random.default_rng(5))
        rng = np.random.default_rng(5)
        g = rng.standard_normal((3, 9))
        if kind == "matern52":
            g = g * np.sqrt(5.0 / rng.chisquare(5, size=9))[None, :]
        want = g / np.broadcast_to(np.asarray(ls, dtype=np.float64).reshape(-1), (3,))[:, None]
        assert np.array_equal(Om, want) and Om.flags.c_contiguous
        assert np.array_equal(Om, PR.sample_basis(kind, 3, 9, ls, np.random.default_rng(5)))


def test_the_host_mirror_binds_the_new_calls():
    for name in ("dsdgp_pathwise_eval", "dsdgp_pathwise_scratch_bytes", "dsdgp_pathwise_weights"):
        assert name in _lib.EXPORTED_SYMBOLS
    assert callable(getattr(DGP, "sample_functions"))
