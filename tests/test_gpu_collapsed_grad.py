"""-m gpu: the gradients of the collapsed bound on the device (SGPR_Layer.bound_gradients, DGP_Collapsed.compute_log_likelihood_gradients,
training.ScipyOptimizer) against tests/psi_grad_reference.py.

Bars, by the project's rule (tests/test_gpu_psi_grad.py): the truth is the long-double reference, e64 the distance of the same
operation sequence in float64 from it, mag the sum of the magnitudes of the terms added into an entry; every entry of every gradient is
within 8 max(e64, 2^-50 mag) of the truth.  The inducing inputs keep a distance from one another (tests/collapsed_reference.py says why:
at a cond(Kuu) of 1e7 the float64 sequence's own error is the luck of one order of operations)."""
import numpy as np
import pytest

from tests import collapsed_reference as CR
from tests import psi_grad_reference as R

pytestmark = pytest.mark.gpu

LD = np.longdouble
#          N   M  D  DY  s>0   ARD  seed
CASES = {
    "n40": (40, 6, 2, 2, True, True, 31),
    "n70": (70, 17, 3, 1, True, False, 32),            # a second tile row of inducing inputs, two row splits, one lengthscale
    "novar": (40, 6, 2, 2, False, True, 33),           # X_var = None
}
_CACHE = {}


def _case(name):
    if name not in _CACHE:
        N, M, D, DY, noisy, ard, seed = CASES[name]
        rng = np.random.default_rng(seed)
        mu = rng.standard_normal((N, D))
        s = rng.uniform(0.05, 0.3, (N, D)) if noisy else None
        Z = CR.spaced_points(rng, M, D, 0.5)
        Y = np.sin(mu @ rng.standard_normal((D, DY))) + 0.2 * rng.standard_normal((N, DY))
        ls = rng.uniform(0.8, 1.3, D) if ard else np.array([1.0])
        c = dict(mu=mu, s=s, Z=Z, variance=1.3, ls=ls, ard=ard, Y=Y, noise=0.2)
        a = (mu, s, Z, 1.3, ls, ard, Y, 0.2, CR.JITTER)
        c["truth"] = R.collapsed_grad(*a, dtype=LD)
        c["f64"] = R.collapsed_grad(*a, dtype=np.float64)
        _CACHE[name] = c
    return _CACHE[name]


def _ratio(dev, tr, f64, mag):
    dev, tr, f64, mag = (np.atleast_1d(np.asarray(a)) for a in (dev, tr, f64, mag))
    err = np.abs(dev.reshape(tr.shape) - tr).astype(np.float64)
    bar = 8.0 * np.maximum(np.abs(f64 - tr).astype(np.float64), 2.0 ** -50 * mag.astype(np.float64))
    return float(np.max(err / bar))


def _check(got, truth, f64, keys=R.GRAD_KEYS, label=""):
    (_, tg, mag), (_, fg, _) = truth, f64
    figs = {k: _ratio(got[k], tg[k], fg[k], mag[k]) for k in keys}
    print(label, {k: "%.3g" % v for k, v in figs.items()}, "(x bar)")
    for k, v in figs.items():
        assert v <= 1.0, (k, v)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _layer(c):
    from doubly_stochastic_dgp.gpflow_compat import RBF, Zero
    from doubly_stochastic_dgp.layers import SGPR_Layer
    D = c["mu"].shape[1]
    kern = RBF(D, variance=c["variance"], lengthscales=c["ls"] if c["ard"] else float(c["ls"][0]), ARD=c["ard"])
    return SGPR_Layer(kern, c["Z"].copy(), c["Y"].shape[1], Zero())


@pytest.mark.parametrize("name", tuple(CASES))
def test_bound_gradients_match_the_truth(name):
    c = _case(name)
    layer = _layer(c)
    layer.set_data(c["mu"], c["s"], c["Y"], c["noise"])
    g = layer.bound_gradients()
    assert set(g) == {"bound"} | set(R.GRAD_KEYS) and g["X_var"].shape == c["mu"].shape
    assert g["bound"] == layer.build_likelihood()
    assert abs(g["bound"] - float(c["truth"][0])) <= 1e-10 * abs(float(c["truth"][0]))
    _check(g, c["truth"], c["f64"], label=name)
    again = layer.bound_gradients(on_device=True)              # a second call, left on the device: the same bits
    for k in g:
        assert _same_bits(again[k].cpu().numpy().reshape(np.shape(g[k])), g[k]), k


def test_one_layer_model_returns_the_parameters_and_the_input_adjoints():
    from doubly_stochastic_dgp.gpflow_compat import Gaussian
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    c = _case("novar")
    layer = _layer(c)
    lik = Gaussian(variance=c["noise"])
    model = DGP_Collapsed(c["mu"], c["Y"], lik, [layer])
    bound, pairs, adj = model.compute_log_likelihood_gradients()
    assert bound == model.compute_log_likelihood()
    assert [p for p, _ in pairs] == [layer.feature.Z, layer.kern.variance, layer.kern.lengthscales, lik.variance]
    for p, g in pairs:
        assert g.shape == p.shape
    got = dict(zip(("Z", "variance", "lengthscales", "lik_variance"), (g for _, g in pairs)), **adj)
    _check(got, c["truth"], c["f64"], label="one layer")


def test_two_layer_model_from_dgp():
    """the last layer's inputs are the inner layer's marginal means and variances (from the device: the reference is given them)"""
    from doubly_stochastic_dgp.dgp import DGP
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    rng = np.random.default_rng(34)
    N, M, D = 40, 6, 2
    X = rng.standard_normal((N, D))
    Y = np.sin(X @ rng.standard_normal((D, 1))) + 0.2 * rng.standard_normal((N, 1))
    Z = CR.spaced_points(rng, M, D, 0.5)
    dgp = DGP(X, Y, Z, [RBF(D, lengthscales=1.1), RBF(D, variance=1.2, lengthscales=0.9)], Gaussian(variance=0.15))
    model = DGP_Collapsed.from_dgp(dgp)
    _, ms, vs = model.inner_layers_propagate(X, S=1)
    top = model.layers[-1]
    a = (ms[-1][0], vs[-1][0], top.feature.Z.value, 1.2, np.array([0.9]), False, Y, 0.15, CR.JITTER)
    truth, f64 = R.collapsed_grad(*a, dtype=LD), R.collapsed_grad(*a, dtype=np.float64)
    bound, pairs, adj = model.compute_log_likelihood_gradients()
    assert bound == model.compute_log_likelihood()
    KL = sum(layer.KL() for layer in model.layers[:-1])
    assert abs((bound + KL) - float(truth[0])) <= 1e-10 * abs(float(truth[0]))
    got = dict(zip(("Z", "variance", "lengthscales", "lik_variance"), (g for _, g in pairs)), **adj)
    assert adj["X_mean"].shape == (N, D) and adj["X_var"].shape == (N, D)
    _check(got, truth, f64, label="two layers")


def test_inducing_inputs_at_the_data_give_the_gradients_of_exact_gp_regression():
    """Z = X, zero input variance, no jitter: the collapsed bound is the exact log marginal likelihood, and so are its gradients in the
    kernel variance, the lengthscale and the noise"""
    from doubly_stochastic_dgp import settings
    from doubly_stochastic_dgp.gpflow_compat import RBF, Zero
    from doubly_stochastic_dgp.layers import SGPR_Layer
    rng = np.random.default_rng(35)
    N, D, DY, v, ls, noise = 12, 2, 2, 1.3, np.array([1.0]), 0.2
    X = CR.spaced_points(rng, N, D, 1.1)
    Y = np.sin(X @ rng.standard_normal((D, DY))) + 0.2 * rng.standard_normal((N, DY))
    lml, exact = R.exact_gp_grad(X, Y, v, ls, noise, dtype=LD)
    _, f64, _ = R.collapsed_grad(X, None, X, v, ls, False, Y, noise, 0.0, dtype=np.float64)
    _, _, mag = R.collapsed_grad(X, None, X, v, ls, False, Y, noise, 0.0, dtype=LD)
    layer = SGPR_Layer(RBF(D, variance=v, lengthscales=1.0), X.copy(), DY, Zero())
    with settings.temp_jitter(0.0):
        layer.set_data(X, None, Y, noise)
        g = layer.bound_gradients()
    assert abs(g["bound"] - float(lml)) <= 1e-10 * abs(float(lml))
    for k in ("variance", "lengthscales", "lik_variance"):
        fig = _ratio(g[k], exact[k], f64[k], mag[k])
        print(k, "%.3g (x bar)" % fig)
        assert fig <= 1.0, (k, fig)


def test_scipy_optimizer_fits_the_one_layer_model():
    """sparse GP regression, complete: Z, the kernel and the noise from a poor start.  On the CPU, L-BFGS-B on the float64 reference
    objective from this start stops on the projected gradient (gtol = 1e-4, ftol out of the way) after 88 iterations: maxiter = 400
    is well outside."""
    from doubly_stochastic_dgp.gpflow_compat import RBF, Gaussian, Zero
    from doubly_stochastic_dgp.layers import SGPR_Layer
    from doubly_stochastic_dgp.model_zoo import DGP_Collapsed
    from doubly_stochastic_dgp.training import ScipyOptimizer
    rng = np.random.default_rng(7)
    N, M, D, DY, gtol = 40, 6, 2, 2, 1e-4
    X = rng.standard_normal((N, D))
    Y = np.sin(X @ rng.standard_normal((D, DY))) + 0.2 * rng.standard_normal((N, DY))
    kern, lik = RBF(D, lengthscales=2.0), Gaussian(variance=1.0)
    top = SGPR_Layer(kern, X[0:2 * M:2].copy(), DY, Zero())
    model = DGP_Collapsed(X, Y, lik, [top])
    twin = DGP_Collapsed(X, Y, lik, [SGPR_Layer(kern, top.feature, DY, Zero())])       # shares the kernel, Z and the likelihood
    before = model.compute_log_likelihood()
    res = ScipyOptimizer(options={"ftol": 1e-13, "gtol": gtol}).minimize(model, maxiter=400)
    after = model.compute_log_likelihood()
    print("bound %.6f -> %.6f in %d iterations, %d evaluations: %s" % (before, after, res.nit, res.nfev, res.message))
    assert after >= before and after == -res.fun
    assert res.success and res.status == 0 and res.nit < 400
    # the reference's gradient, in unconstrained space, at the device's final parameters
    v, l, s2 = float(kern.variance.value), float(np.asarray(kern.lengthscales.value).reshape(-1)[0]), float(lik.variance.value)
    _, g, _ = R.collapsed_grad(X, None, top.feature.Z.value, v, np.array([l]), False, Y, s2, CR.JITTER, dtype=LD)
    chain = -np.expm1(-(np.array([v, l, s2]) - 1e-6))
    gu = np.concatenate([np.asarray(g["Z"], dtype=np.float64).reshape(-1),
                         np.array([float(g["variance"]), float(g["lengthscales"][0]), float(g["lik_variance"])]) * chain])
    print("reference's unconstrained gradient at the end: max |g| = %.3g" % np.max(np.abs(gu)))
    assert np.max(np.abs(gu)) < 10.0 * gtol
    # a model that shares the parameters sees the new values
    assert twin.compute_log_likelihood() == after
    # a parameter that is not trainable keeps its bits; the others move
    kern.lengthscales.set_trainable(False)
    lik.variance.assign(0.5)
    keep, Zb = np.array(kern.lengthscales.value).copy(), np.array(top.feature.Z.value).copy()
    res2 = ScipyOptimizer().minimize(model, maxiter=3)
    assert res2.x.size == M * D + 2
    assert np.array_equal(np.asarray(kern.lengthscales.value), keep) and not np.array_equal(top.feature.Z.value, Zb)
    assert float(lik.variance.value) != 0.5
