"""-m gpu: the collapsed bound and its prediction on the device (layers.SGPR_Layer, model_zoo.DGP_Collapsed; csrc/psi.hip,
csrc/collapsed.hip) against tests/collapsed_reference.py and against the two identities of the reference's own tests
(tests/test_collapsed.py:30-54 and :57-104).

Bars.  Against the long-double reference: 8 max(e64, 2^-50), e64 the distance of the same operation sequence in float64 — in units of
the sum of the magnitudes of the bound's terms for the bound, of max |Y| for the predictive mean and of the kernel variance for the
predictive variance.  First identity (one layer, Z = X, against the exact GP): the reference's own atol = rtol = 1e-5, under
settings.temp_jitter(1e-9) (the formula itself is 4e-9 / 2e-8 from the exact value there; at the default 1e-6 it is 4 - 5e-6, only a
factor 2 inside the bar).  Second identity (two layers: DGP_Quad after one natural-gradient step with gamma = 1 on the last layer lands
on the collapsed bound): rtol 1e-7, the reference's default assert_allclose and the bar of the one-layer instance
(tests/test_gpu_parity.py::test_natgrad_gamma1_gives_collapsed_bound)."""
import numpy as np
import pytest
from numpy.testing import assert_allclose

from tests import collapsed_reference as CR

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _layer(c, DY):
    from doubly_stochastic_dgp.gpflow_compat import RBF, Zero
    from doubly_stochastic_dgp.layers import SGPR_Layer
    D = c["mu"].shape[1]
    return SGPR_Layer(RBF(D, variance=c["variance"], lengthscales=float(c["ls"][0])), c["Z"], DY, Zero())


@pytest.mark.parametrize("name", CR.NAMES)
def test_bound_and_prediction_match_the_reference(name):
    c = CR.inputs(name)
    hi, lo = CR.state(name, CR.LD), CR.state(name, np.float64)
    DY = c["Y"].shape[1]
    layer = _layer(c, DY)
    layer.set_data(c["mu"], c["s"], c["Y"], c["noise"])
    bound, terms = layer.bound_terms()
    unit = float(np.sum(np.abs(hi["terms"])))
    e64 = abs(float(lo["bound"] - hi["bound"])) / unit
    err = abs(float(bound - hi["bound"])) / unit
    print("%s: bound %.17g (truth %.17g); error %.3g, e64 %.3g (units of sum |terms| = %.3g)" % (name, bound, float(hi["bound"]), err, e64, unit))
    assert np.all(np.abs(terms - hi["terms"].astype(np.float64)) <= 1e-9 * unit)
    assert bound == ((((terms[0] + terms[1]) + terms[2]) + terms[3]) + terms[4]) + terms[5]
    assert err <= 8.0 * max(e64, 2.0 ** -50)
    assert _same_bits(layer.build_likelihood(), bound)
    ymax, v = float(np.max(np.abs(c["Y"]))), c["variance"]
    for full_cov in (False, True):
        mh, vh = CR.predict(hi, c["Xs"], full_cov)
        ml, vl = CR.predict(lo, c["Xs"], full_cov)
        m, var = layer.conditional_ND(c["Xs"], full_cov=full_cov)
        assert m.shape == mh.shape and var.shape == vh.shape
        em, ev = float(np.max(np.abs(ml - mh))) / ymax, float(np.max(np.abs(vl - vh))) / v
        dm, dv = float(np.max(np.abs(m - mh))) / ymax, float(np.max(np.abs(var - vh))) / v
        print("  full_cov=%s: mean %.3g (e64 %.3g), var %.3g (e64 %.3g)" % (full_cov, dm, em, dv, ev))
        assert dm <= 8.0 * max(em, 2.0 ** -50)
        assert dv <= 8.0 * max(ev, 2.0 ** -50)
        for d in range(1, DY):                      # one covariance, a copy per output
            assert _same_bits(var[..., d], var[..., 0])
        m2, var2 = layer.conditional_ND(c["Xs"], full_cov=full_cov)
        assert _same_bits(m2, m) and _same_bits(var2, var)


def test_a_failed_factorisation_raises_cholesky_error():
    from doubly_stochastic_dgp._lib import CholeskyError
    from doubly_stochastic_dgp import settings
    c = dict(CR.inputs("n40"))
    c["Z"] = np.repeat(c["Z"][:1], 5, axis=0)          # five identical inducing inputs, a negative jitter: Kuu is indefinite
    layer = _layer(c, 1)
    with settings.temp_jitter(-1e-3):
        with pytest.raises(CholeskyError):
            layer.set_data(c["mu"], None, c["Y"], c["noise"])


@pytest.mark.parametrize("N,D,DY,ls,seed", [(4, 3, 2, 0.1, 100), (40, 1, 1, 0.8, 3)])
def test_single_layer_at_z_equal_x_is_the_exact_gp(N, D, DY, ls, seed):
    """tests/test_collapsed.py:30-54 with its own bars."""
    from doubly_stochastic_dgp import settings
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian, Zero
    from doubly_stochastic_dgp.layers import SGPR_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(N, D)) * (1.0 if N == 4 else 3.0)
    Y = rng.uniform(size=(N, DY)) if N == 4 else np.sin(3 * X) + 0.1 * rng.randn(N, 1)
    Xs = rng.uniform(size=(5, D)) * (1.0 if N == 4 else 3.0)
    lik = Gaussian()
    lik.variance = 0.1
    model = DGP_Collapsed(X, Y, lik, [SGPR_Layer(RBF(D, lengthscales=ls), X, DY, Zero())])
    with settings.temp_jitter(1e-9):
        L = model.compute_log_likelihood()
        mean, var = model.predict_f_full_cov(Xs, 1)
    lml, mean_exact, cov_exact = CR.exact_gp(X, Y, 1.0, ls, 0.1, Xs)
    print("bound %.12g exact %.12g; mean %.3g, var %.3g" % (L, lml, np.max(np.abs(mean[0] - mean_exact)),
                                                            np.max(np.abs(var[0] - cov_exact[:, :, None]))))
    assert mean.shape == (1, 5, DY) and var.shape == (1, 5, 5, DY)
    assert_allclose(L, lml, atol=1e-5, rtol=1e-5)
    assert_allclose(mean[0], mean_exact, atol=1e-5, rtol=1e-5)
    assert_allclose(var[0], np.tile(cov_exact[:, :, None], [1, 1, DY]), atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("M,seed", [(9, 0), (20, 1)])
def test_two_layers_natgrad_gamma1_lands_on_the_collapsed_bound(M, seed):
    """tests/test_collapsed.py:57-104 at N = 7: D_X = 1, the inducing inputs on a grid spaced >= l / 2, last-layer l = 0.7 (M = 9) and 0.6
    (M = 20), the first layer's q_sqrt scaled so that the inner variance at the data stays <= 0.3 (the range in which the H = 100 rule
    is exact).  The first layer's q is set in whitened form, q_mu = Lu a and q_sqrt = 0.3 Lu with |a| small, so that its KL term —
    which both sides take from the same call — stays of the size of the data terms and cannot dilute the relative difference.  The sum
    over rows of marginal expectations does not care that the quadrature shares one z across rows.  reparameterize integrates over
    var + settings.jitter, so the collapsed side is fed set_data(mean, var + jitter, ...), and the inner KL is subtracted.
    Measured on an MI355X: relative difference 2.9e-16 (M = 9, inner KL 7.0 of a bound of -12.1) and 6.4e-14 (M = 20, inner KL 15.7 of
    a bound of -23.2)."""
    from doubly_stochastic_dgp import settings
    from doubly_stochastic_dgp.dgp import DGP_Quad
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian
    from doubly_stochastic_dgp.layer_initializations import init_layers_linear
    from doubly_stochastic_dgp.layers import SGPR_Layer
    from doubly_stochastic_dgp.training import NatGradOptimizer
    rng = np.random.RandomState(seed)
    N, lik_var = 7, 0.1
    X = rng.uniform(size=(N, 1)) * 2.0
    Y = np.sin(2.0 * X) + 0.1 * rng.randn(N, 1)
    Z = np.linspace(-2.0, 4.0, M)[:, None]            # spacing 0.75 (M = 9) and 0.32 (M = 20); last-layer l / 2 = 0.35 and 0.3
    assert Z[1, 0] - Z[0, 0] >= 0.3
    kerns = [RBF(1, lengthscales=0.6), RBF(1, lengthscales=0.7 if M == 9 else 0.6)]
    layers = init_layers_linear(X, Y, Z, kerns)
    lik = Gaussian()
    lik.variance = lik_var
    m_ng = DGP_Quad(X, Y, lik, layers, H=100)
    d = (Z - Z.T) / 0.6
    Lu = np.linalg.cholesky(np.exp(-0.5 * d * d) + settings.jitter * np.eye(M))
    m_ng.layers[0].q_mu = Lu @ (0.3 * rng.randn(M, 1))
    m_ng.layers[0].q_sqrt = 0.3 * Lu[None]
    last = m_ng.layers[-1]
    NatGradOptimizer(1.0).minimize(m_ng, var_list=[[last.q_mu, last.q_sqrt]], maxiter=1)
    L_ng = m_ng.compute_log_likelihood()
    mean, var = m_ng.layers[0].conditional_ND(X)
    assert np.max(var) <= 0.3
    top = SGPR_Layer(last.kern, last.feature.Z.read_value(), 1, last.mean_function)
    top.set_data(mean, var + settings.jitter, Y, lik_var)
    KL = m_ng.layers[0].KL()
    L_col = top.build_likelihood() - KL
    print("M = %d: natgrad %.15g collapsed %.15g relative difference %.3g; inner KL %.3g, inner variance <= %.3g" %
          (M, L_ng, L_col, abs(L_ng - L_col) / abs(L_ng), KL, np.max(var)))
    assert KL <= M          # 0.5 M (0.09 - 1 - log 0.09) + 0.5 |a|^2 = 0.75 M + 0.045 M in expectation
    assert_allclose(L_col, L_ng, rtol=1e-7)


def _three_layer():
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian
    rng = np.random.RandomState(5)
    N, D, M = 50, 2, 8
    X = rng.randn(N, D)
    Y = np.sin(X[:, :1]) + 0.1 * rng.randn(N, 1)
    dgp = DGP(X, Y, X[:M].copy(), [RBF(D, lengthscales=1.2), RBF(D, lengthscales=1.0), RBF(D, variance=1.4, lengthscales=0.9)],
              Gaussian(variance=0.2))
    for layer in dgp.layers:
        layer.q_mu = 0.5 * rng.randn(*layer.q_mu.shape)
    zs = [rng.randn(1, N, D), rng.randn(1, N, D)]
    return dgp, X, Y, zs, rng.randn(9, D)


def test_from_dgp_matches_the_reference_on_the_engines_own_statistics():
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    dgp, X, Y, zs, Xs = _three_layer()
    model = DGP_Collapsed.from_dgp(dgp)
    L = model.compute_log_likelihood(zs=zs)
    assert _same_bits(model.compute_log_likelihood(zs=zs), L)
    _, ms, vs = model.inner_layers_propagate(X, S=1, zs=zs)
    assert ms[-1].shape == (1, 50, 2) and len(ms) == 2
    # the model's value has the bits of the layer-level composition it is made of
    top = model.layers[-1]
    top.set_data(ms[-1][0], vs[-1][0], Y, 0.2)
    KL = sum(layer.KL() for layer in model.layers[:-1])
    assert _same_bits(top.build_likelihood() - KL, L)
    Zl = top.feature.Z.value
    hi = CR.collapsed(ms[-1][0], vs[-1][0], Zl, 1.4, 0.9, Y, 0.2, 1e-6, dtype=CR.LD)
    lo = CR.collapsed(ms[-1][0], vs[-1][0], Zl, 1.4, 0.9, Y, 0.2, 1e-6, dtype=np.float64)
    unit = float(np.sum(np.abs(hi["terms"]))) + abs(KL)
    e64 = abs(float(lo["bound"] - hi["bound"])) / unit
    err = abs(float(L - (hi["bound"] - KL))) / unit
    print("from_dgp: %.17g, reference %.17g; error %.3g, e64 %.3g" % (L, float(hi["bound"] - KL), err, e64))
    assert err <= 8.0 * max(e64, 2.0 ** -50)
    # the inner layers are shared: a write through the DGP is seen by the collapsed model
    dgp.layers[0].q_mu = dgp.layers[0].q_mu.value * 0.5
    assert model.compute_log_likelihood(zs=zs) != L


def test_parameters_trained_by_the_shared_dgp_reach_the_collapsed_model():
    """from_dgp shares layer objects; what the DGP's own engine trains afterwards lives on the device until somebody reads it.  The
    collapsed model pulls it before every evaluation: after a training step of the DGP its bound moves, to the bits of a collapsed
    model built from the DGP after the step."""
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    dgp, X, Y, zs, Xs = _three_layer()
    model = DGP_Collapsed.from_dgp(dgp)
    before = model.compute_log_likelihood(zs=zs)
    dgp.train_step(0.05, sync=True)
    dgp.train_step(0.05, sync=True)
    after = model.compute_log_likelihood(zs=zs)
    fresh = DGP_Collapsed.from_dgp(dgp).compute_log_likelihood(zs=zs)
    print("bound before the DGP's steps %.15g, after %.15g, from a fresh view %.15g" % (before, after, fresh))
    assert after != before
    assert _same_bits(after, fresh)


def test_predictions_run_and_repeat():
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    dgp, X, Y, zs, Xs = _three_layer()
    model = DGP_Collapsed.from_dgp(dgp)
    S = 3
    rng = np.random.RandomState(6)
    zt = [rng.randn(S, 9, 2), rng.randn(S, 9, 2), rng.randn(S, 9, 1)]
    m1, v1 = model._build_predict(Xs, S=S, zs=zt)
    assert m1.shape == (S, 9, 1) and v1.shape == (S, 9, 1) and np.all(v1 > 0.0)
    # with one inner layer the statistics of the training set depend on no draw: explicit draws for X* pin every bit
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian
    two = DGP_Collapsed.from_dgp(DGP(X, Y, X[:8].copy(), [RBF(2), RBF(2, lengthscales=0.9)], Gaussian(variance=0.2)))
    a1, b1 = two._build_predict(Xs, S=S, zs=zt[1:])
    a2, b2 = two._build_predict(Xs, S=S, zs=zt[1:])
    assert a1.shape == (S, 9, 1) and _same_bits(a1, a2) and _same_bits(b1, b2)
    mean, var = model.predict_y(Xs, S)
    assert mean.shape == (S, 9, 1) and np.all(np.isfinite(mean)) and np.all(var > 0.2)
    dens = model.predict_density(Xs, np.zeros((9, 1)), S)
    assert dens.shape == (9, 1) and np.all(np.isfinite(dens))
    Fs, Fmeans, Fvars = model.predict_all_layers(Xs, S)
    assert [f.shape for f in Fs] == [(S, 9, 2), (S, 9, 2), (S, 9, 1)] and len(Fmeans) == len(Fvars) == 3
    mf, vf = model.predict_f_full_cov(Xs, 2)
    assert mf.shape == (2, 9, 1) and vf.shape == (2, 9, 9, 1)
