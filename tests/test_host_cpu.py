"""CPU-side tests (-m "not gpu"): the C-ABI library loads and exports every symbol of include/dsdgp.h, the host mirror
reproduces the reference's construction logic (layer_initializations.py:16-52, layers.py:123-165, dgp.py:42-59), and the
product path refuses to run without the HIP device (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest
from numpy.testing import assert_allclose

from oracle import dgp_oracle as O
from tests.helpers import kern_spec, product_kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_or_skip():
    from doubly_stochastic_dgp import _lib
    if not os.path.exists(_lib.lib_path()):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_cabi_exports_every_declared_symbol():
    _lib = _lib_or_skip()
    header = open(os.path.join(ROOT, "include", "dsdgp.h")).read()
    declared = set(re.findall(r"\b(dsdgp_[a-z0-9_]+)\s*\(", header))
    declared -= {"dsdgp_status"}
    lib = ctypes.CDLL(_lib.lib_path())          # dlopen only: no compute call without a GPU
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, missing
    assert set(_lib.EXPORTED_SYMBOLS) <= declared
    # the verification accessor of tests/test_gpu_factor_direct.py: header, ctypes mirror, library and the call-site table agree
    assert "dsdgp_model_layer_matrix" in declared and "dsdgp_model_layer_matrix" in _lib.EXPORTED_SYMBOLS
    assert "`dsdgp_model_layer_matrix`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, code in (("LU", _lib.MAT_LU), ("LUINV", _lib.MAT_LUINV), ("LUINVT", _lib.MAT_LUINVT), ("KUINV", _lib.MAT_KUINV)):
        assert re.search(r"\bDSDGP_MAT_%s = %d\b" % (name, code), header), name
    assert lib.dsdgp_version() >= 100


def test_struct_layout_matches_header():
    _lib = _lib_or_skip()
    # the ctypes mirrors against the sizes the C side was compiled with (LP64): dsdgp_layer_desc = 18*4 + 8 + 8*8 (round 6: + kvar_identity, reserved0)
    lib = ctypes.CDLL(_lib.lib_path())
    assert ctypes.sizeof(_lib.LayerDesc) == lib.dsdgp_sizeof_layer_desc() == 144
    assert ctypes.sizeof(_lib.ModelDesc) == lib.dsdgp_sizeof_model_desc() == 56 + 16 * 144
    assert ctypes.sizeof(_lib.KernelSpec) == 40


def test_no_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from doubly_stochastic_dgp import _lib
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian
    X = np.random.randn(20, 2)
    m = DGP(X, X[:, :1], X[:5], [RBF(2)], Gaussian())
    with pytest.raises(_lib.DsdgpError, match="no CPU fallback"):
        m.compute_log_likelihood()


@pytest.mark.parametrize("dims", [(3, 3, 3), (8, 4, 4), (2, 5, 5), (6, 3, 1)])
@pytest.mark.parametrize("white", [False, True])
def test_init_layers_linear_matches_reference_logic(dims, white):
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import Gaussian
    rng = np.random.RandomState(0)
    X, Y = rng.randn(40, dims[0]), rng.randn(40, 2)
    Z = X[:12].copy()
    specs = [kern_spec("rbf", d, 1.0 + 0.1 * i, 0.9) for i, d in enumerate(dims)]
    lds = O.init_layers_linear(X, Y, Z, specs, white=white)
    model = DGP(X, Y, Z, [product_kernel(s) for s in specs], Gaussian(), white=white)
    assert len(model.layers) == len(lds)
    for l, layer in zip(lds, model.layers):
        assert layer.mean_function.kind == l["mean"].kind
        assert_allclose(layer.feature.Z.value, l["Z"], rtol=1e-12, atol=1e-12)
        assert_allclose(layer.q_sqrt.value, l["q_sqrt"], rtol=1e-9, atol=1e-12)
        assert layer.q_mu.shape == l["q_mu"].shape and not layer.q_mu.value.any()
        if l["mean"].kind == "linear":
            assert_allclose(layer.mean_function.A.value, l["mean"].A, rtol=1e-12, atol=1e-12)
            assert layer.mean_function.A.trainable is False
    assert model.layers[-1].num_outputs == 2 and model.num_data == 40


def test_parameter_semantics():
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian, Matern52, White
    X = np.random.RandomState(1).randn(10, 2)
    lik = Gaussian()
    lik.variance = 0.01                                            # tests/test_dgp.py:40
    assert lik.variance.value == 0.01
    k = Matern52(2, lengthscales=0.5) + White(2, variance=1e-5)
    assert k.input_dim == 2
    m = DGP(X, X[:, :1], X, [RBF(2), k], lik, num_samples=2)
    q = np.random.randn(10, 1)
    m.layers[-1].q_mu = q                                          # tests/test_dgp.py:91
    assert np.array_equal(m.layers[-1].q_mu.value, q)
    assert np.array_equal(m.layers[-1].q_mu.read_value(), q)
    m.likelihood.likelihood.variance = 0.05                        # using_natural_gradients.ipynb:99
    assert m.likelihood.likelihood.variance.value == 0.05
    m.layers[0].q_sqrt = m.layers[0].q_sqrt.value * 1e-5           # demo_regression_UCI.ipynb:183
    assert m.layers[0].q_sqrt.value.max() < 1e-4
    m.layers[0].q_mu.set_trainable(False)
    assert m.layers[0].q_mu.trainable is False


def test_minibatch_epochs_cover_data():
    from doubly_stochastic_dgp.dgp import Minibatch
    mb = Minibatch(103, 10, seed=0)
    seen = np.concatenate([mb.next_indices() for _ in range(31)])   # 310 = 3 epochs + 1
    assert seen.shape == (310,)
    for e in range(3):
        assert sorted(seen[e * 103:(e + 1) * 103]) == list(range(103))
    mb2 = Minibatch(103, 10, seed=0)
    assert np.array_equal(mb2.next_indices(), seen[:10])            # deterministic


def test_positive_transform_roundtrip():
    from doubly_stochastic_dgp.gpflow_compat import positive_backward, positive_forward
    y = np.array([1e-5, 0.01, 1.0, 50.0])
    assert_allclose(positive_forward(positive_backward(y)), y, rtol=1e-12)
    assert_allclose(positive_forward(positive_backward(y)), O.positive_forward(O.NP, O.positive_backward_np(y)), rtol=1e-14)


def test_mvhermgauss_matches_oracle_quad_points():
    # [UPSTREAM] gpflow.quadrature.mvhermgauss as consumed by DGP_Quad (dgp.py:143-157)
    from doubly_stochastic_dgp.utils import mvhermgauss
    from oracle import dgp_oracle as O
    x, w = mvhermgauss(5, 3)
    assert x.shape == (125, 3) and w.shape == (125,)
    zs, wq = O.quad_points(5, [1, 2])
    np.testing.assert_allclose(np.concatenate([zs[0][:, 0, :], zs[1][:, 0, :]], 1), x * 2 ** 0.5, rtol=0, atol=0)
    np.testing.assert_allclose(wq, w * np.pi ** -1.5, rtol=1e-15)
    # exact for polynomials: E[z1^2 z2^4] under N(0, I) = 1 * 3
    z = x * 2 ** 0.5
    np.testing.assert_allclose(np.sum(wq * z[:, 0] ** 2 * z[:, 1] ** 4), 3.0, rtol=1e-12)


def test_shard_terms_rejects_empty_minibatch():
    from doubly_stochastic_dgp.distributed import shard_terms
    assert shard_terms(7372, 1000, 8) == (7372 / 8000.0, 0.125)
    with pytest.raises(ValueError):
        shard_terms(100, 0, 1)


def test_minibatch_span_epoch_is_bumped_by_every_regeneration():
    """A minibatch that straddles an epoch boundary regenerates the permutation inside next_indices(); the spans that follow
    must announce a NEW epoch so that the device copy of the permutation is refreshed (N % B != 0 is the normal case, e.g.
    7372 / 1000)."""
    from doubly_stochastic_dgp.dgp import Minibatch
    N, B = 25, 10
    mb, ref = Minibatch(N, B, seed=3), Minibatch(N, B, seed=3)
    uploaded_epoch, perm_dev = None, None
    for _ in range(40):
        want = ref.next_indices()                      # the plain stream of indices (ground truth)
        span = mb.next_span()
        if span is not None:
            perm, start, epoch = span
            if epoch != uploaded_epoch:                # what DGP_Base.next_minibatch does with its device copy
                perm_dev, uploaded_epoch = perm.copy(), epoch
            got = perm_dev[start:start + B]
        else:
            got = mb.next_indices()
        assert np.array_equal(got, want)


def test_multiclass_targets_are_validated():
    from doubly_stochastic_dgp.gpflow_compat import Gaussian, MultiClass
    from doubly_stochastic_dgp.utils import BroadcastingLikelihood
    lik = BroadcastingLikelihood(MultiClass(3))
    lik.check_targets(np.array([[0.0], [2.0], [1.0]]))
    for bad in (np.array([[3.0]]), np.array([[-1.0]]), np.array([[0.5]]), np.array([[np.nan]]), np.eye(3)):
        with pytest.raises(ValueError):
            lik.check_targets(bad)
    BroadcastingLikelihood(Gaussian()).check_targets(np.array([[0.3, -7.0]]))   # real-valued targets: nothing to check


def test_bernoulli_is_a_built_likelihood():
    """Bernoulli() (tests/test_dgp.py:48-54 of the reference) is accepted; its targets only need to be finite (N, D)."""
    from doubly_stochastic_dgp.gpflow_compat import Bernoulli
    from doubly_stochastic_dgp.utils import BroadcastingLikelihood
    lik = BroadcastingLikelihood(Bernoulli())
    assert lik.needs_broadcasting and lik.bernoulli
    lik.check_targets(np.array([[-1.0], [1.0], [0.0]]))
    with pytest.raises(ValueError):
        lik.check_targets(np.array([[np.nan]]))
    with pytest.raises(NotImplementedError):
        Bernoulli(invlink="logit")


def test_poisson_exponential_student_t_gamma_beta_are_built_likelihoods():
    """The further GPflow 1.1.1 likelihoods BroadcastingLikelihood (utils.py:54-121) can wrap here: accepted with their upstream
    constructor signatures; other links and other likelihood classes still fail loudly."""
    from doubly_stochastic_dgp import _lib
    from doubly_stochastic_dgp.gpflow_compat import Beta, Exponential, Gamma, Likelihood, Poisson, StudentT
    from doubly_stochastic_dgp.utils import BroadcastingLikelihood
    for lik, want in ((Poisson(binsize=2.0), (_lib.LIK_POISSON, 1.0, 2.0)), (Exponential(), (_lib.LIK_EXPONENTIAL, 1.0, 1.0)),
                      (StudentT(scale=0.7, deg_free=4.0), (_lib.LIK_STUDENT_T, 0.7, 4.0)), (Gamma(shape=1.5), (_lib.LIK_GAMMA, 1.5, 1.0)),
                      (Beta(scale=2.5), (_lib.LIK_BETA, 2.5, 1.0))):
        b = BroadcastingLikelihood(lik)
        assert b.needs_broadcasting and b.generic and not b.bernoulli
        k, p0, p1 = b.generic_args()
        assert (k, p1) == (want[0], want[2]) and abs(p0 - want[1]) < 1e-12
        b.check_targets(np.array([[0.0], [3.0]]))
        with pytest.raises(ValueError):
            b.check_targets(np.array([[np.inf]]))
    assert StudentT().scale.trainable and abs(float(StudentT().scale.value) - 1.0) < 1e-12 and StudentT().deg_free == 3.0
    with pytest.raises(NotImplementedError):
        Poisson(invlink="square")
    with pytest.raises(NotImplementedError):
        Exponential(invlink=np.square)
    Poisson(invlink=np.exp)

    assert abs(float(Gamma().shape.value) - 1.0) < 1e-12 and Gamma().shape.trainable and Beta().scale.trainable
    with pytest.raises(NotImplementedError):
        Beta(invlink="logit")

    class Ordinal(Likelihood):
        pass
    with pytest.raises(NotImplementedError):
        BroadcastingLikelihood(Ordinal())
