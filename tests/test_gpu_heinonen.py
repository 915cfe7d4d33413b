"""-m gpu: model_zoo.DGP_Heinonen and a DGP_Collapsed with a GPR_Layer on top.  The reference's two identities
(tests/test_zoo_models.py) at its shapes (N = 6, D_X = 3, D_Y = 2, Matern52, jitter 1e-12) and its own tolerance (1e-4): with
q_mu = 0 and an Identity mean the model is exact GP regression on X (compared with tests/dense_reference.py's GPR), and with any q_mu it
is this repository's DGP with Z = X, white=True, a collapsed q_sqrt, the second layer's inducing inputs at the first layer's mean and one
natural-gradient step of size 1.  In both, predict_y, predict_density, predict_f and predict_f_full_cov agree.  Then the gradients:
DGP_Heinonen's against the reference, a DGP_Collapsed([SVGP_Layer, GPR_Layer]) with inner=True against central differences of the
device's own bound at one entry per block, and a short ScipyOptimizer fit of each that does not decrease its objective."""
import numpy as np
import pytest

from tests import dense_reference as DR
from tests import gram_grad_reference as GR

pytestmark = pytest.mark.gpu
LD = np.longdouble
TOL = 1e-4
N, D_X, D_Y = 6, 3, 2


def _data(seed):
    rng = np.random.default_rng(seed)
    return rng, rng.uniform(size=(N, D_X)), rng.standard_normal((N, D_Y)), rng.standard_normal((N, D_Y))


def _heinonen(X, Y, lik_var, q_mu=None, var0=1.0):
    from doubly_stochastic_dgp.gpflow_compat import Gaussian, Identity, Matern52, Zero
    from doubly_stochastic_dgp.layers import GPMC_Layer, GPR_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_Heinonen
    layer0 = GPMC_Layer(Matern52(D_X, lengthscales=0.5, variance=var0), X.copy(), D_X, Identity())
    layer1 = GPR_Layer(Matern52(D_X, lengthscales=0.5), Zero(), D_Y)
    model = DGP_Heinonen(X, Y, Gaussian(variance=lik_var), [layer0, layer1])
    if q_mu is not None:
        model.layers[0].q_mu = q_mu
    return model


def _predictions(model, Xs, Ys):
    mean, var = model.predict_y(Xs, 1)
    dens = model.predict_density(Xs, Ys, 1)
    fm, fv = model.predict_f(Xs, 1)
    ffm, ffv = model.predict_f_full_cov(Xs, 1)
    return dict(mean=mean[0], var=var[0], density=dens, f_mean=fm[0], f_var=fv[0], full_mean=ffm[0], full_cov=ffv[0])


def test_constructor_checks():
    from doubly_stochastic_dgp.gpflow_compat import Bernoulli, Gaussian, Matern52, Zero
    from doubly_stochastic_dgp.layers import GPR_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_Heinonen
    rng, X, Y, _ = _data(0)
    good = _heinonen(X, Y, 0.1)
    with pytest.raises(ValueError):
        DGP_Heinonen(X, Y, Gaussian(), good.layers[:1])
    with pytest.raises(ValueError):
        DGP_Heinonen(X, Y, Gaussian(), [good.layers[1], good.layers[1]])
    with pytest.raises(NotImplementedError):
        DGP_Heinonen(X, Y, Bernoulli(), good.layers)
    with pytest.raises(ValueError):
        DGP_Heinonen(X, Y, Gaussian(), good.layers, minibatch_size=3)
    Fs, ms, vs = good.inner_layers_propagate(X)
    assert Fs[0].shape == (1, N, D_X) and np.array_equal(Fs[0], ms[0]) and np.all(vs[0] == 0.0)


def test_vs_single_layer():
    from doubly_stochastic_dgp import settings
    rng, X, Y, Ys = _data(1)
    lik_var, ls = 0.01, np.array([0.5])
    with settings.temp_jitter(1e-12):
        got = _predictions(_heinonen(X, Y, lik_var, var0=1e-1), X, Ys)
    r, _ = DR.gpr(GR.MATERN52, X, Y, 1.0, ls, False, None, lik_var, None, Xnew=X, dtype=LD)
    f_mean, f_var, cov = (np.asarray(r[k], dtype=np.float64) for k in ("mean", "var", "cov"))
    y_var = f_var + lik_var
    dens = -0.5 * np.log(2 * np.pi * y_var) - 0.5 * (Ys - f_mean) ** 2 / y_var
    for k, want in (("mean", f_mean), ("var", y_var), ("density", dens), ("f_mean", f_mean), ("f_var", f_var), ("full_mean", f_mean),
                    ("full_cov", np.tile(cov[:, :, None], [1, 1, D_Y]))):
        np.testing.assert_allclose(got[k], want, atol=TOL, rtol=TOL, err_msg=k)


def test_vs_DGP2():
    from doubly_stochastic_dgp import settings
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import Gaussian, Matern52, Zero
    from doubly_stochastic_dgp.training import NatGradOptimizer
    rng, X, Y, Ys = _data(2)
    q_mu, lik_var = rng.standard_normal((N, D_X)), 0.1
    with settings.temp_jitter(1e-12):
        dgp = DGP(X, Y, X, [Matern52(D_X, lengthscales=0.5), Matern52(D_X, lengthscales=0.5)], Gaussian(variance=lik_var),
                  mean_function=Zero(), white=True)
        dgp.layers[0].q_mu = q_mu
        dgp.layers[0].q_sqrt = dgp.layers[0].q_sqrt.read_value() * 1e-24
        _, ms, _ = dgp.predict_all_layers(X, 1)
        dgp.layers[1].feature.Z = ms[0][0].copy()                # the inducing inputs in the right place
        NatGradOptimizer(gamma=1).minimize(dgp, var_list=[[dgp.layers[1].q_mu, dgp.layers[1].q_sqrt]], maxiter=1)
        want = _predictions(dgp, X, Ys)
        got = _predictions(_heinonen(X, Y, lik_var, q_mu), X, Ys)
    for k in want:
        np.testing.assert_allclose(got[k], want[k], atol=TOL, rtol=TOL, err_msg=k)


def test_gradients_match_the_reference():
    from doubly_stochastic_dgp import settings
    rng, X, Y, _ = _data(3)
    q_mu, lik_var, ls = 0.5 * rng.standard_normal((N, D_X)), 0.1, np.array([0.5])
    model = _heinonen(X, Y, lik_var, q_mu)
    ref = lambda dt: DR.log_density((GR.MATERN52, GR.MATERN52), X, Y, q_mu, 1.0, ls, settings.jitter, 1.0, ls, False, lik_var,
                                    mean0="identity", dtype=dt)
    (val, grad, parts), (_, grad64, parts64) = ref(LD), ref(np.float64)
    bound, pairs, adj = model.compute_log_likelihood_gradients()
    top, lik = model.layers[1], model.likelihood.likelihood
    assert [p for p, _ in pairs] == [model.layers[0].q_mu, top.kern.variance, top.kern.lengthscales, lik.variance]
    assert all(g.shape == p.shape for p, g in pairs)
    assert bound == model.compute_log_likelihood() and model.compute_log_prior() == model.layers[0].log_prior()
    assert abs(bound - float(parts["bound"][0])) <= 1e-10 * abs(float(parts["bound"][0]))
    assert abs(model.compute_log_density() - float(val)) <= 1e-10 * abs(float(val))
    # the gradients: the device against the truth, measured in the float64 reference's own distance from it (at least 1e-12 relative)
    wants = [(grad + np.asarray(q_mu, dtype=LD), grad64 + q_mu), (parts["variance"], parts64["variance"]),
             (parts["lengthscales"], parts64["lengthscales"]), (parts["lik_variance"], parts64["lik_variance"])]
    for (p, g), (tr, f64) in zip(pairs, wants):
        tr, f64 = np.asarray(tr, dtype=LD).reshape(p.shape), np.asarray(f64, dtype=np.float64).reshape(p.shape)
        scale = float(np.max(np.abs(tr)))
        err, e64 = float(np.max(np.abs(g - tr))), float(np.max(np.abs(f64 - tr)))
        print("max error %.3g, float64 reference %.3g, scale %.3g" % (err, e64, scale))
        assert err <= max(8.0 * e64, 1e-12 * scale)
    logp, dpairs = model.compute_log_density_gradients()
    assert logp == model.compute_log_density() and np.array_equal(dpairs[0][1], pairs[0][1] - q_mu)
    assert np.max(np.abs(adj["X_mean"] - parts["X_mean"].astype(np.float64))) <= 1e-9 * float(np.max(np.abs(parts["X_mean"])))


def _collapsed_gpr_model(rng):
    from doubly_stochastic_dgp.gpflow_compat import Gaussian, Identity, Matern52, RBF, White, Zero
    from doubly_stochastic_dgp.layers import GPR_Layer, SVGP_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    n, M, D, DY = 30, 5, 2, 1
    X = rng.standard_normal((n, D))
    Y = np.sin(X @ rng.standard_normal((D, DY))) + 0.2 * rng.standard_normal((n, DY))
    inner = SVGP_Layer(RBF(D, lengthscales=1.2), X[:M].copy(), D, Identity())
    inner.q_mu = 0.3 * rng.standard_normal((M, D))
    top = GPR_Layer(Matern52(D, variance=1.1, lengthscales=0.9) + White(D, variance=0.05), Zero(), DY)
    return DGP_Collapsed(X, Y, Gaussian(variance=0.2), [inner, top]), inner, top


def test_collapsed_model_over_a_gpr_layer_has_the_gradients_of_its_bound():
    """DGP_Collapsed([SVGP_Layer, GPR_Layer]), inner=True: one entry per block against central differences of the device's own bound
    (h = 1e-5; the bound's rounding over 2 h and the truncation both stay below 1e-6 (1 + |g|), as in tests/test_gpu_dense_layers.py).
    One inner layer: its marginal means do not depend on the draws, so every evaluation sees the same function."""
    from doubly_stochastic_dgp.gpflow_compat import split_kernel
    model, inner, top = _collapsed_gpr_model(np.random.default_rng(4))
    bound, pairs, adj = model.compute_log_likelihood_gradients(inner=True)
    assert abs(bound - model.compute_log_likelihood()) <= 1e-12 * abs(bound)
    assert np.all(adj["X_var"] == 0.0)
    stat, wk = split_kernel(top.kern)
    head = [stat.variance, stat.lengthscales, wk.variance, model.likelihood.likelihood.variance]
    assert [p for p, _ in pairs[:4]] == head and not hasattr(top, "feature")
    grads = {id(p): g for p, g in pairs}
    h = 1e-5
    for what, p, idx in (("top variance", stat.variance, ()), ("top lengthscale", stat.lengthscales, ()), ("white", wk.variance, ()),
                         ("noise", head[3], ()), ("inner q_mu", inner.q_mu, (2, 1)), ("inner Z", inner.feature.Z, (1, 0)),
                         ("inner lengthscale", inner.kern.lengthscales, ())):
        base = np.array(p.value, dtype=np.float64)
        vals = []
        for s in (-1.0, 1.0):
            v = base.copy()
            v[idx] += s * h
            p.assign(v)
            vals.append(model.compute_log_likelihood())
        p.assign(base)
        fd, g = (vals[1] - vals[0]) / (2 * h), float(np.asarray(grads[id(p)])[idx])
        print("%s: gradient %.10g, central difference %.10g" % (what, g, fd))
        assert abs(fd - g) <= 1e-6 * (1.0 + abs(g)), what


def test_scipy_optimizer_does_not_decrease_either_objective():
    from doubly_stochastic_dgp.training import CollapsedAdamOptimizer, ScipyOptimizer
    model, inner, top = _collapsed_gpr_model(np.random.default_rng(5))
    before = model.compute_log_likelihood()
    res = ScipyOptimizer().minimize(model, maxiter=5)
    after = model.compute_log_likelihood()
    print("collapsed over GPR_Layer: %.6f -> %.6f (%d variables)" % (before, after, res.x.size))
    assert res.x.size == 4 and after >= before
    res = ScipyOptimizer().minimize(model, maxiter=3, inner=True)
    assert res.x.size > 4 and model.compute_log_likelihood() >= after
    b = CollapsedAdamOptimizer(1e-3).minimize(model, maxiter=2)
    assert np.isfinite(b)
    rng, X, Y, _ = _data(6)
    hein = _heinonen(X, Y, 0.1, 0.5 * rng.standard_normal((N, D_X)))
    before = hein.compute_log_density()
    res = ScipyOptimizer().minimize(hein, maxiter=5)
    after = hein.compute_log_density()
    print("DGP_Heinonen (MAP): %.6f -> %.6f (%d variables)" % (before, after, res.x.size))
    assert res.x.size == N * D_X + 3 and after >= before and after == -res.fun
    with pytest.raises(NotImplementedError):
        CollapsedAdamOptimizer().minimize(hein, maxiter=1)
