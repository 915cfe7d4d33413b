"""-m "not gpu": pins the yardsticks of the kernel-expectation and collapsed-layer tests (tests/psi_reference.py,
tests/collapsed_reference.py) on the case tables, and the host logic of SGPR_Layer / DGP_Collapsed that needs no device.

The closed forms against an independent rule: a tensor Gauss-Hermite quadrature over the input density at D <= 2, inside the range in
which the H = 100 rule is exact (l >= 0.5, s <= 0.3; a 1-D rule is exact to 3e-16 there, while at l = 0.1, s = 0.6 even H = 200 is 7 %
off).  At s = 0 psi2 = psi1^T psi1 and the collapsed bound is Titsias' bound with Qff formed densely.  A condition on the cases, not a
measurement: the float64 evaluation of every collapsed case stays within 1e-8 (relative) of the long-double one — a case that breaks
this is ill-conditioned and has to be replaced, not given a looser bar."""
import ctypes
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose

from tests import collapsed_reference as CR
from tests import psi_cases as PC
from tests import psi_reference as R


@pytest.mark.parametrize("name", PC.QUADRATURE)
def test_closed_forms_match_gauss_hermite_quadrature(name):
    c = PC.quadrature_inputs(name)
    assert c["mu"].shape[1] <= 2 and np.all(c["ls"] >= 0.5) and np.all(c["s"] <= 0.3)
    _, p1, p2 = R.psi(c["mu"], c["s"], c["Z"], c["variance"], c["ls"], dtype=R.LD)
    q1, q2 = R.quadrature(c["mu"], c["s"], c["Z"], c["variance"], c["ls"], H=100)
    n = c["mu"].shape[0]
    assert np.max(np.abs(q1 - p1.astype(np.float64))) <= 1e-13 * c["variance"]
    assert np.max(np.abs(q2 - p2.astype(np.float64))) <= 1e-13 * n * c["variance"] ** 2


@pytest.mark.parametrize("name", PC.NAMES)
def test_float64_sequence_is_close_to_long_double(name):
    tr, f = PC.truth(name), PC.float64(name)
    c = PC.inputs(name)
    n, v = c["mu"].shape[0], c["variance"]
    assert f["psi0"] == n * v and float(tr["psi0"]) == n * v
    nan1, nan2 = np.isnan(tr["psi1"]), np.isnan(tr["psi2"])
    assert np.array_equal(np.isnan(f["psi1"]), nan1) and np.array_equal(np.isnan(f["psi2"]), nan2)
    if name in PC.NEGVAR:
        assert nan2.all() and not nan1.any()          # l^2 + s > 0 > l^2 + 2 s: psi1 finite, every entry of psi2 is fed by the bad row
    else:
        assert not nan1.any() and not nan2.any()
        assert np.max(np.abs(f["psi1"] - tr["psi1"])) <= 64 * 2.0 ** -53 * v
        assert np.max(np.abs(f["psi2"] - tr["psi2"])) <= 64 * 2.0 ** -53 * n * v * v
        assert np.array_equal(f["psi2"], f["psi2"].T)
    if name == "far":
        assert np.all(f["psi1"][:, 0] == 0.0) and np.all(f["psi2"][0] == 0.0) and not np.any(np.signbit(f["psi2"][0]))


@pytest.mark.parametrize("name", ["zero", "null"])
def test_zero_variance_gives_the_gram_products(name):
    c, tr = PC.inputs(name), PC.truth(name)
    K = CR.rbf(c["mu"], c["Z"], c["variance"], c["ls"], R.LD)
    n = c["mu"].shape[0]
    assert np.max(np.abs(tr["psi1"] - K)) <= 2.0 ** -60
    assert np.max(np.abs(tr["psi2"] - K.T @ K)) <= n * 2.0 ** -58


@pytest.mark.parametrize("name", CR.NAMES)
def test_collapsed_cases_are_well_conditioned(name):
    hi, lo = CR.state(name, CR.LD), CR.state(name, np.float64)
    rel = abs(float(lo["bound"] - hi["bound"])) / abs(float(hi["bound"]))
    print(name, "bound", float(hi["bound"]), "float64 relative error", rel)
    assert rel <= 1e-8
    c = CR.inputs(name)
    Z = c["Z"]
    if Z.shape[0] > 1:                                  # the inducing inputs are at least l / 2 apart (collapsed_reference.inputs)
        d = np.sqrt(np.sum((Z[:, None, :] - Z[None, :, :]) ** 2, axis=2)) + 1e9 * np.eye(Z.shape[0])
        assert d.min() >= 0.5 * float(c["ls"][0])


@pytest.mark.parametrize("name", [n for n in CR.NAMES if CR.inputs(n)["s"] is None])
def test_collapsed_bound_is_the_dense_titsias_bound_at_zero_variance(name):
    c = CR.inputs(name)
    dense = CR.titsias_dense(c["mu"], c["Y"], c["Z"], c["variance"], c["ls"], c["noise"], CR.JITTER)
    assert_allclose(float(CR.state(name, CR.LD)["bound"]), dense, rtol=1e-9)


def test_collapsed_prediction_at_z_equal_x_is_the_exact_gp():
    # tests/test_collapsed.py:30-54: with Z = X the sparse posterior is the exact one
    rng = np.random.RandomState(3)
    X = rng.uniform(size=(12, 1)) * 3
    Y = np.sin(3 * X) + 0.1 * rng.randn(12, 1)
    Xs = rng.uniform(size=(5, 1)) * 3
    st = CR.collapsed(X, None, X, 1.0, 0.8, Y, 0.1, 1e-9, dtype=CR.LD)
    lml, mean, cov = CR.exact_gp(X, Y, 1.0, 0.8, 0.1, Xs)
    m, v = CR.predict(st, Xs, full_cov=True)
    assert_allclose(float(st["bound"]), lml, rtol=1e-6)
    assert_allclose(m.astype(np.float64), mean, atol=1e-6)
    assert_allclose(v[:, :, 0].astype(np.float64), cov, atol=1e-6)
    md, vd = CR.predict(st, Xs, full_cov=False)
    assert np.array_equal(md, m) and np.max(np.abs((vd[:, 0] - np.diag(v[:, :, 0])).astype(np.float64))) <= 1e-15


# ---------------------------------------------------------------------------------------------------------------- host logic
def _two_layer_dgp(minibatch_size=None):
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian
    rng = np.random.RandomState(0)
    X, Y = rng.randn(30, 2), rng.randn(30, 1)
    return DGP(X, Y, X[:7].copy(), [RBF(2), RBF(2, lengthscales=0.8)], Gaussian(variance=0.1), minibatch_size=minibatch_size)


def test_library_exports_the_new_entry_points():
    from doubly_stochastic_dgp import _lib
    if not os.path.exists(_lib.lib_path()):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.lib_path())
    for name in ("dsdgp_rbf_expectations", "dsdgp_scale_copy", "dsdgp_collapsed_bound", "dsdgp_collapsed_var"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_sgpr_layer_refuses_what_has_no_closed_form():
    from doubly_stochastic_dgp.gpflow_compat import RBF, Identity, Linear, Matern52, White, Zero
    from doubly_stochastic_dgp.layers import Collapsed_Layer, SGPR_Layer
    Z = np.zeros((3, 2))
    with pytest.raises(NotImplementedError, match="plain RBF"):
        SGPR_Layer(Matern52(2), Z, 1, Zero())
    with pytest.raises(NotImplementedError, match="White"):
        SGPR_Layer(RBF(2) + White(2, variance=1e-3), Z, 1, Zero())
    for mf in (Identity(), Linear(np.ones((2, 1)))):
        with pytest.raises(NotImplementedError, match="only Zero is consistent"):
            SGPR_Layer(RBF(2), Z, 1, mf)
    layer = SGPR_Layer(RBF(2), Z, 1, Zero())
    assert isinstance(layer, Collapsed_Layer) and layer.KL() == 0.0 and layer.num_inducing == 3
    with pytest.raises(RuntimeError, match="set_data"):
        layer.build_likelihood()
    with pytest.raises(NotImplementedError):
        Collapsed_Layer().build_likelihood()


def test_dgp_collapsed_refuses_minibatches_other_likelihoods_and_training():
    from doubly_stochastic_dgp.gpflow_compat import RBF, Bernoulli, Gaussian, Zero
    from doubly_stochastic_dgp.layers import SGPR_Layer, SVGP_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    from doubly_stochastic_dgp.training import AdamOptimizer, NatGradOptimizer
    rng = np.random.RandomState(1)
    X, Y = rng.randn(20, 2), rng.randn(20, 1)
    top = SGPR_Layer(RBF(2), X[:5].copy(), 1, Zero())
    with pytest.raises(ValueError, match="minibatch_size"):
        DGP_Collapsed(X, Y, Gaussian(), [top], minibatch_size=10)
    with pytest.raises(NotImplementedError, match="Gaussian"):
        DGP_Collapsed(X, np.sign(Y), Bernoulli(), [top])
    with pytest.raises(ValueError, match="last layer"):
        DGP_Collapsed(X, Y, Gaussian(), [SVGP_Layer(RBF(2), X[:5].copy(), 1, Zero())])
    model = DGP_Collapsed(X, Y, Gaussian(), [top], minibatch_size=None)
    with pytest.raises(NotImplementedError, match="reverse pass"):
        model.train_step(0.01)
    with pytest.raises(NotImplementedError, match="reverse pass"):
        AdamOptimizer(0.01).minimize(model, maxiter=1)
    with pytest.raises(NotImplementedError, match="reverse pass"):
        NatGradOptimizer(1.0).minimize(model, var_list=[])
    with pytest.raises(ValueError, match="whole training set"):
        model.compute_log_likelihood(X, Y)


def test_from_dgp_shares_the_inner_layers():
    from doubly_stochastic_dgp.layers import SGPR_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    dgp = _two_layer_dgp(minibatch_size=10)
    model = DGP_Collapsed.from_dgp(dgp)
    assert len(model.layers) == 2 and model.layers[0] is dgp.layers[0] and isinstance(model.layers[1], SGPR_Layer)
    assert model.layers[1].kern is dgp.layers[1].kern and model.layers[1].feature is dgp.layers[1].feature
    assert model.likelihood.likelihood is dgp.likelihood.likelihood
    assert model.minibatch_size is None and model.X_data.shape == (30, 2) and len(dgp.layers) == 2
    dgp.layers[0].q_mu = np.ones((7, 2))                       # one object: a write through either model is seen by both
    assert np.array_equal(model.layers[0].q_mu.value, np.ones((7, 2)))


def test_dgp_collapsed_refuses_the_scoring_methods_built_on_a_full_engine():
    """DGP_Base.evaluate / predict_quantiles / calibration / classification_report run the base class's engine over ALL layers; a
    collapsed model has none (its inner engine ends one layer early, and at the 1 -> 1 -> 1 widths of init_layers_linear it would
    score the inner layer without any shape complaining).  They refuse, before any device is looked for."""
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    rng = np.random.RandomState(2)
    X, Y = rng.randn(20, 1), rng.randn(20, 1)
    model = DGP_Collapsed.from_dgp(DGP(X, Y, X[:6].copy(), [RBF(1), RBF(1)], Gaussian(variance=0.1)))
    assert model.layers[0].num_outputs == model.layers[1].num_outputs == 1
    for call in (lambda: model.evaluate(X, Y, 2), lambda: model.predict_quantiles(X, 2), lambda: model.calibration(X, Y, 2),
                 lambda: model.classification_report(X, Y, 2), lambda: model.engine(), lambda: model.next_minibatch()):
        with pytest.raises(NotImplementedError, match="no device engine over all layers"):
            call()
    assert callable(model.inner_engine)
    top = model.layers[-1]
    assert top._model() is model and model not in list(top.__dict__.values())       # a weak reference, not a parameter of the layer
    assert len(list(model.parameters())) > 0                                          # walking the parameters terminates
